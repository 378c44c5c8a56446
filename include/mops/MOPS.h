// MOPS.h -- C++ operator API of the MI355X trajectory engine.
//
// Source-compatible mirror of the reference's public API for the trajectory
// path and the fixed-depth image remapping (YosefQiu/MOPS include/api/MOPS.h:20-148,
// settings structs src/Core/MPASOVisualizer.h:20-103, data model setters
// src/Core/MPASOGrid.cpp:82-188, src/Core/MPASOSolution.cpp:1145-1210):
// same names, argument meaning and error behaviour, implemented on the C ABI
// (include/mops_traj.h) -- the GPU engine is the only backend.
//
// Differences a caller can observe:
//   * vec3 is a plain {x, y, z} struct; the reference's backends rewrite
//     p.x() into p.x with a macro (BackendCompat.hpp:188-191) -- define
//     MOPS_COMPAT_ACCESSOR_MACROS before including this header to get the
//     same macros;
//   * derived fields are computed on the GPU and kept in HBM; nothing is
//     cached on disk (the reference's cache is keyed only by timestep, Q11).
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "mops_traj.h"

struct vec2 { double x, y; };
struct vec3 { double x, y, z; };
struct vec2i { int x, y; };
using SphericalCoord = vec2;
using CartesianCoord = vec3;

#ifdef MOPS_COMPAT_ACCESSOR_MACROS
#define x() x
#define y() y
#define z() z
#endif

namespace MOPS {

enum class CalcDirection : int { kForward, kBackward, kCount };
enum class CalcMethodType : int { kRK4, kEuler, kCount };
enum class CalcPositionType : int { kCenter, kVertx, kPoint, kCount };
enum class CalcAttributeType : int { kZonalMerimoal, kVelocity, kZTop, kTemperature, kSalinity, kAll, kCount };
enum class VisualizeType : int { kFixedLayer, kFixedDepth };
enum class SaveType : int { kVTI, kPNG, kNone, kCount };
// Extension: the layer rule of the fixed-depth remapping (mops_traj.h MOPS_LAYER_*)
enum class LayerRule : int { kReference = MOPS_LAYER_REFERENCE, kBracket = MOPS_LAYER_BRACKET };
enum class GridAttributeType : int {
    kCellSize, kEdgeSize, kVertexSize, kMaxEdgesSize, kVertLevels, kVertLevelsP1, kVertexCoord, kCellCoord,
    kEdgeCoord, kVertexLatLon, kVerticesOnCell, kVerticesOnEdge, kCellsOnVertex, kCellsOnCell,
    kNumberVertexOnCell, kCellsOnEdge, kEdgesOnCell, kCellWeight, krefBottomDepth, kCount
};
enum class AttributeType : int {
    kZonalVelocity, kMeridionalVelocity, kVelocity, kNormalVelocity, kZTop, kLayerThickness, kBottomDepth, kCount
};

#define ONE_SECOND 1
#define ONE_MINUTE 60
#define ONE_HOUR 60 * 60
#define ONE_DAY 60 * 60 * 24
#define ONE_MONTH 60 * 60 * 24 * 30
#define ONE_YEAR 60 * 60 * 24 * 30 * 12

struct TrajectoryLine {
    int lineID;
    std::vector<CartesianCoord> points;
    std::vector<CartesianCoord> velocity;
    std::vector<double> temperature;
    std::vector<double> salinity;
    CartesianCoord lastPoint;
    double duration;
    double timestamp;
    double depth;
};

// ImageBuffer (src/Common/ImageBuffer.hpp:10-64): the members a caller reads.  Row-major
// [height][width][4] (x, y, z, alpha); a written pixel has alpha 1.
template <typename T>
class ImageBuffer {
  public:
    ImageBuffer() = default;
    ImageBuffer(int w, int h) : mWidth(w), mHeight(h) { mPixels.resize((size_t)mWidth * mHeight * 4, (T)0); }
    int getIndex(const int i, const int j) const {
        if (i < 0 || i >= mHeight || j < 0 || j >= mWidth) return -1;
        return (i * mWidth + j) * 4;
    }
    vec3 getPixel(const int i, const int j) const {
        const int index = getIndex(i, j);
        if (index == -1) return vec3{-1, -1, -1};
        return vec3{(double)mPixels[index + 0], (double)mPixels[index + 1], (double)mPixels[index + 2]};
    }
    std::vector<T> getChannel(int channel) const {
        std::vector<T> out;
        if (channel < 0 || channel > 3) return out;
        out.reserve((size_t)mWidth * mHeight);
        for (size_t k = 0; k < (size_t)mWidth * mHeight; ++k) out.push_back(mPixels[4 * k + channel]);
        return out;
    }
    int getWidth() const { return mWidth; }
    int getHeight() const { return mHeight; }

    std::vector<T> mPixels;

  protected:
    int mWidth = 0;
    int mHeight = 0;
};

// VisualizationSettings (src/Core/MPASOVisualizer.h:20-42); layerRule is this engine's one extension
struct VisualizationSettings {
    vec2 imageSize;  // x = width, y = height
    vec2 LonRange;
    vec2 LatRange;
    vec2 DepthRange{0.0, 0.0};
    double FixedLatitude;
    union {
        double FixedDepth;
        double FixedLayer;
    };
    int tile_index;
    CalcAttributeType CalcType = CalcAttributeType::kZonalMerimoal;
    CalcPositionType PositionType = CalcPositionType::kPoint;
    VisualizeType VisType = VisualizeType::kFixedDepth;
    SaveType saveType = SaveType::kNone;
    double TimeStep;
    LayerRule layerRule = LayerRule::kReference;
    // MOPS_RunRemappingSection's great-circle path (this engine's extension): waypoints (x = lat, y = lon) in
    // degrees; its rows span DepthRange, or the grid's reference bottom depths while DepthRange is (0, 0)
    std::vector<vec2> SectionPath;
    // MOPS_RunEddyCensus (this engine's extension): the Okubo-Weiss threshold in standard deviations of the layer
    // (the census takes -EddyThreshold * sigma) and the fewest cells an eddy may have
    double EddyThreshold = 0.2;
    int EddyMinCells = 4;
    VisualizationSettings() = default;
};

// One row of MOPS_RunEddyCensus's table (mops_eddy_table, mops_traj.h): lat / lon in degrees and the radius of
// the circle of `area` (metres) are formed on the host from `centre` and `area`.
struct Eddy {
    int index = 0;
    double lat = 0.0, lon = 0.0, radius = 0.0, area = 0.0;
    int polarity = 0;  // +1 / -1: the sign of the vorticity
    double circulation = 0.0;
    int n_cells = 0, root = 0, core_cell = 0;
    double ow_min = 0.0;
    CartesianCoord centre{};
};

struct EddyCensus {
    double threshold = 0.0;        // the Okubo-Weiss threshold used
    std::vector<Eddy> eddies;      // ascending root cell
    std::vector<int> labels;       // [nCells]: the eddy index of every cell, or -1
    ImageBuffer<double> image;     // {eddy index, polarity, 0, 1} on the config's window
};

struct TrajectorySettings {
    size_t deltaT;
    size_t simulationDuration;
    size_t recordT;
    float depth;
    std::vector<float> particle_depths;
    std::string fileName;
    CalcDirection directionType = CalcDirection::kForward;
    CalcMethodType methodType = CalcMethodType::kEuler;
    bool hasPerParticleDepths() const { return !particle_depths.empty(); }
    // This engine's extension (default: the reference's output, quirk Q9).  True: MOPS_RunPathLine samples the
    // first two double attributes, in name order, that both active solutions carry (Kernel::PathLine's
    // current_attrs, MPASOVisualizerKernels.cpp:1288-1324) and fills TrajectoryLine::temperature / salinity with
    // the attributes of those names (zeros for a name that is not sampled).  MOPS_RunStreamLine ignores it.
    bool sampleAttributes = false;
    // This engine's extension (default: the reference's RK4, quirk Q1, in which a stage point across a cell edge
    // fails IsInMesh and kills the particle).  True, with methodType kRK4: MOPS_RunPathLine locates each of RK4
    // stages 2-4 by the step's own one-hop walk from the step's cell and evaluates it in the cell found
    // (MOPS_RK4_RELOCATE, mops_traj.h); a particle whose stages never leave its cell gets the same bytes.  With
    // kEuler it has no effect (Euler has no stages).  MOPS_RunStreamLine with it and kRK4, and MOPS_RunPathLine
    // with it, kRK4 and sampleAttributes, follow the reference's error convention: Error() and an empty list.
    bool relocateStages = false;
    // This engine's extension, the layer mode (mops_traj_advance_layer, mops_traj.h; default -1: the depth mode).
    // >= 0: MOPS_RunStreamLine / MOPS_RunPathLine advect within that model layer -- the Wachspress-weighted vertex
    // velocity of the layer (TBBKernel::CalcVelocity), w = 0, a particle dying where that velocity is shorter than
    // 1e-12 -- and `depth` is still carried, because the records keep their radius.  relocateStages then applies
    // to streamlines as well.  A layer outside [0, nVertLevels), or sampleAttributes with it, follows the
    // reference's error convention: Error() and an empty list.
    int fixedLayer = -1;
    // This engine's extension, a horizontal random walk on top of the advection (mops_diffusion, mops_traj.h;
    // default 0: none, the same bytes as before).  diffusivity: the eddy diffusivity Kh in m^2/s; randomSeed: the
    // 64-bit key of the counter-based generator; randomEpoch: a counter word the caller owns, so that successive
    // calls with one seed draw different deviates.  Particle i of the call draws with id i: a run is reproducible
    // to the bit.  With diffusivity > 0, MOPS_RunStreamLine without fixedLayer and MOPS_RunPathLine with
    // sampleAttributes, and a negative or non-finite diffusivity always, follow the reference's error convention:
    // Error() and an empty list.
    double diffusivity = 0.0;
    unsigned long long randomSeed = 0;
    unsigned int randomEpoch = 0;
};

struct SamplingSettings {
    void setSampleRange(const vec2i& n) { sampleRange = n; }
    void setGeoBox(const vec2& lat, const vec2& lon) { sampleLatitudeRange = lat; sampleLongitudeRange = lon; }
    void setDepth(double d) { sampleDepth = d; }
    void setSamplingRegion(const vec2i& n, const vec2& lat, const vec2& lon, double d) {
        sampleRange = n; sampleLatitudeRange = lat; sampleLongitudeRange = lon; sampleDepth = d;
    }
    void atCellCenter(bool b) { bAtCellCenter = b; }
    vec2i getSampleRange() const { return sampleRange; }
    vec2 getLatitudeRange() const { return sampleLatitudeRange; }
    vec2 getLongitudeRange() const { return sampleLongitudeRange; }
    bool isAtCellCenter() const { return bAtCellCenter; }
    double getDepth() const { return sampleDepth; }

  private:
    vec2i sampleRange{0, 0};
    vec2 sampleLatitudeRange{0, 0};
    vec2 sampleLongitudeRange{0, 0};
    double sampleDepth = 0.0;
    bool bAtCellCenter = false;
};

// MPASOGrid: the members the trajectory path reads (MPASOGrid.h), 1-based size_t connectivity.
class MPASOGrid {
  public:
    void setGridAttribute(GridAttributeType type, int val);
    void setGridAttributesVec3(GridAttributeType type, const std::vector<vec3>& vec);
    void setGridAttributesVec2(GridAttributeType type, const std::vector<vec2>& vec);
    void setGridAttributesInt(GridAttributeType type, const std::vector<size_t>& vec);
    void setGridAttributesFloat(GridAttributeType type, const std::vector<float>& vec);
    bool checkAttribute() const;

    int mCellsSize = 0, mEdgesSize = 0, mMaxEdgesSize = 0, mVertexSize = 0, mVertLevels = 0, mVertLevelsP1 = 0;
    std::vector<vec3> vertexCoord_vec, cellCoord_vec, edgeCoord_vec;
    std::vector<vec2> vertexLatLon_vec;
    std::vector<size_t> verticesOnCell_vec, verticesOnEdge_vec, cellsOnVertex_vec, cellsOnCell_vec,
        numberVertexOnCell_vec, cellsOnEdge_vec, edgesOnCell_vec;
    std::vector<float> cellWeight_vec;
    std::string mCachedDataDir;
    std::vector<double> cellRefBottomDepth_vec;  // refBottomDepth: the default rows of MOPS_RunRemappingSection
};

// SolutionID (MPASOSolution.h:12-16); timestep is value-initialised here
struct SolutionID {
    std::string timeStamp;
    int timestep = 0;
};

// MPASOSolution: raw per-cell fields of one snapshot (MPASOSolution.h).
class MPASOSolution {
  public:
    void setAttribute(GridAttributeType type, int val);
    void setAttributesDouble(AttributeType type, const std::vector<double>& vec);
    void setAttributesVec3(AttributeType type, const std::vector<vec3>& vec);
    void setTimestep(int t) { mTimesteps = t; }  // like the reference, does not touch mID
    // 32-bit FNV-1a of "<timeStamp>_<timestep>" (MPASOSolution.h:74-86)
    int getID() const {
        const std::string key = mID.timeStamp + "_" + std::to_string(mID.timestep);
        uint32_t h = 2166136261u;
        for (unsigned char c : key) h = (h ^ c) * 16777619u;
        return static_cast<int>(h);
    }
    std::string getTimeStamp() const { return mTimeStamp; }
    bool checkAttribute() const;

    int mCellsSize = 0, mEdgesSize = 0, mMaxEdgesSize = 0, mVertexSize = 0, mTimesteps = 0, mVertLevels = 0,
        mVertLevelsP1 = 0;
    SolutionID mID;
    std::string mTimeStamp;
    std::vector<double> cellLayerThickness_vec, cellBottomDepth_vec, cellSurfaceHeight_vec, cellZTop_vec,
        cellZonalVelocity_vec, cellMeridionalVelocity_vec, cellVertVelocity_vec, cellNormalVelocity_vec;
    std::vector<vec3> cellCenterVelocity_vec;
    std::map<std::string, std::vector<double>> mDoubleAttributes;
};

void MOPS_Init(const char* device = "gpu");
void MOPS_Begin();
void MOPS_AddGridMesh(std::shared_ptr<MPASOGrid> grid);
void MOPS_AddAttribute(int solID, std::shared_ptr<MPASOSolution> sol);
void MOPS_End();
void MOPS_ActiveAttribute(int t1, std::optional<int> t2 = std::nullopt);
std::vector<TrajectoryLine> MOPS_RunStreamLine(TrajectorySettings* config, std::vector<CartesianCoord>& sample_points);
std::vector<TrajectoryLine> MOPS_RunPathLine(TrajectorySettings* config, std::vector<CartesianCoord>& sample_points);
// MOPSApp::runRemapping (MOPSApp.cpp:171-196): the fixed-depth images of the active front solution --
// image 0 the ENU velocity, image 1 the first two double attributes when there are at least two
std::vector<ImageBuffer<double>> MOPS_RunRemapping(VisualizationSettings* config);
// Extension (the reference's only plot helper for lines is matplotlib, tutorial/pyMOPSAPI.py:132-289): the
// particle density map of `lines` (what MOPS_RunStreamLine / MOPS_RunPathLine return) on the window config
// gives -- imageSize, LatRange, LonRange -- binned on the GPU (mops_density_accumulate, mops_traj.h): every
// point of every line lands in the pixel MOPS_RunRemapping's image has at its lat / lon.  One image
// {count, mean, sum} (alpha 1), NaN where no sample fell, usable with SaveToPNG and SaveVTI.  value: ""
// (count only), "speed" (|velocity|), "temperature" or "salinity" (the lines' vectors of that name).
// Invalid inputs (null config, image size below 1, unknown value, empty or non-finite ranges, a longitude
// range above 360): Error() and an empty image.
ImageBuffer<double> MOPS_RunDensity(const std::vector<TrajectoryLine>& lines, VisualizationSettings* config,
                                    const std::string& value = "");
// Extension ("flow-map lattices and FTLE", mops_traj.h): one seed per pixel of config's window -- imageSize,
// LatRange, LonRange -- row major, (imageSize.y * imageSize.x) points, the positions MOPS_RunRemapping's image
// has its pixels at, formed on the GPU (mops_flowmap_lattice).  Run them as a pathline or streamline and give
// the lines, in this order, to MOPS_RunFTLE.  Invalid inputs (null config, image size below 1): Error() and
// an empty vector.
std::vector<CartesianCoord> MOPS_LatticeSeeds(VisualizationSettings* config);
// Extension: the finite-time Lyapunov exponent image of `lines` seeded by MOPS_LatticeSeeds(config) and given
// in lattice order (lines.size() == imageSize.y * imageSize.x): the flow map is points[0] -> lastPoint of each
// line.  No death array is passed: a dead line has a zero lastPoint (RemoveNaNTrajectoriesAndReindex), which
// is not valid; so is a line without points.  One image {ftle, lambda_max, lambda_min} (alpha 1), NaN where a
// pixel has no valid stencil, usable with SaveToPNG and SaveVTI.  horizon > 0: the integration time in the unit
// the exponent is wanted per.  Columns wrap iff LonRange.y - LonRange.x == 360.  Invalid inputs (null config,
// image size below 1, a line count other than the lattice's, horizon <= 0 or not finite): Error() and an empty
// image.
ImageBuffer<double> MOPS_RunFTLE(const std::vector<TrajectoryLine>& lines, VisualizationSettings* config,
                                 double horizon);
// Extension ("path integrals and LAVD", mops_traj.h): the Lagrangian-averaged vorticity deviation over the active
// front / back pair.  One particle per pixel of config's window (the lattice of MOPS_LatticeSeeds) at
// config->FixedDepth runs one pathline with traj's deltaT, simulationDuration, recordT, direction and method; each
// solution's vorticity deviation -- its vorticity minus the area-weighted mean of its level, kept per solution
// id -- is the single sampled attribute, and the sampled line is summed with the rectangle rule: slot j, sampled
// at the start of step (j+1)*ri - 1, times recordT seconds.  Made of mops_flowmap_lattice,
// mops_velocity_gradient, mops_cell_area, mops_level_mean, mops_cell_to_vertex_signed, mops_run_pathline_attrs,
// mops_path_integral_abs over the returned attribute lines and mops_path_integral_image.  One image {LAVD, mean
// |deviation| in 1/s over K * recordT seconds, 0} (alpha 1), NaN where the particle died (land included), usable
// with SaveToPNG and SaveVTI; it overlays the velocity, density, FTLE and eddy images of the same window.  kRK4
// leaves a mostly-NaN map (quirk Q1).  Invalid inputs (a null argument, no back solution, fixedLayer >= 0,
// relocateStages, diffusivity other than 0, an image size below 1, settings without a step or a record): Error()
// and an empty image.
ImageBuffer<double> MOPS_RunLAVD(VisualizationSettings* config, TrajectorySettings* traj);
// Extension ("vertical sections", mops_traj.h): a depth-by-distance image of the active front solution along the
// great-circle legs through config->SectionPath (mops_section_points, mops_remap_section): imageSize = (columns,
// rows), rows over config->DepthRange, or over the grid's cellRefBottomDepth_vec front / back while DepthRange
// is (0, 0).  {image0} or, with double attributes, {image0, image1}: image0 = {zonal, meridional, across} (alpha
// 1; channels 0 and 1 are the fixed-latitude curtain's pixel, across is positive to the left of the direction of
// travel), image1 = the first two double attributes in name order, {attr0, attr1 or 0, 0}, blended in depth as
// the velocity is.  NaN where a pixel fails.  Invalid inputs (null config, no solution, image size below 1,
// fewer than two waypoints or columns, a bad waypoint or leg, no depth range): Error() and an empty vector.
std::vector<ImageBuffer<double>> MOPS_RunRemappingSection(VisualizationSettings* config);
// The volume transport in Sverdrups (1e6 m^3/s) through image0 of MOPS_RunRemappingSection(config): the across
// channel times ds * dz over the non-NaN pixels, one fixed-order FP64 sum on the host (mops_section_transport).
// Invalid inputs: Error() and NaN.
double MOPS_SectionTransport(const ImageBuffer<double>& image, VisualizationSettings* config);
// Extension ("velocity gradient", mops_traj.h): the relative vorticity and the Okubo-Weiss parameter of the
// active front solution at config->FixedDepth, one image {vorticity, okubo_weiss, 0} (alpha 1).  It is image 1 of
// the fixed-depth remapping with the two signed vertex arrays (mops_velocity_gradient, then
// mops_cell_to_vertex_signed; kept per solution id) as its attributes: MOPS_RunRemapping's window, FixedDepth
// and layerRule, so it overlays the velocity, density and FTLE images.  NaN where a pixel fails.  Invalid inputs
// (null config, no solution, image size below 1): Error() and an empty vector.
std::vector<ImageBuffer<double>> MOPS_RunEddyMap(VisualizationSettings* config);
// Extension ("eddy census", mops_traj.h): the eddies of the active front solution at layer config->FixedLayer
// (truncated and clamped into the levels as VisualizeFixedLayer does) as objects: the connected sets of at least
// config->EddyMinCells cells whose Okubo-Weiss parameter lies below -config->EddyThreshold standard deviations
// (population, over the layer's finite values, FP64 on the host) of the layer, split by the sign of their
// vorticity (mops_velocity_gradient, mops_eddy_classify, mops_label_components, mops_eddy_count,
// mops_eddy_table).  The image is built from the cell map of the fixed-layer remapping on the config's window:
// channels 0 and 1 are NaN where the fixed-layer image is NaN or the pixel's cell is in no eddy, so it overlays
// every other image of the window.  Invalid inputs (null config, no solution, image size below 1, a
// non-finite EddyThreshold, EddyMinCells < 1, no finite Okubo-Weiss value): Error() and an empty result.
EddyCensus MOPS_RunEddyCensus(VisualizationSettings* config);
void MOPS_GenerateSamplePoints(SamplingSettings* config, std::vector<CartesianCoord>& sample_points);

// SaveToPNG (src/Common/ImageBuffer.hpp:91-136) for the double image (the one instantiation the reference
// uses): one channel (default 3, alpha) through the Viridis map -- NaN pixels transparent -- into an 8-bit
// RGBA PNG.  The colouring runs on the GPU (mops_colormap_image), the file is written by
// mops_write_png_rgba8 (stored deflate blocks: the decoded pixels are the reference's, the bytes are not
// stb's).  false for a channel outside 0..3, an empty image or a failed write.
bool SaveToPNG(const ImageBuffer<double>& buffer, const std::string& filename, int channel = 3);

// TypeToStr (src/IO/VTKFileManager.hpp:12-20)
inline std::string TypeToStr(VisualizeType type) {
    switch (type) {
        case VisualizeType::kFixedLayer: return "fixed_layer_";
        case VisualizeType::kFixedDepth: return "fixed_depth_";
    }
    return "unknown_";
}

// VTKFileManager::SaveVTI (src/IO/VTKFileManager.hpp:25-138), both overloads, without VTK: the file is
// outputName + "_" + TypeToStr(VisType) + std::to_string(k) + ".vti" with k = FixedDepth / FixedLayer
// ("..._fixed_depth_10.000000.vti"), origin (LonRange.x, LatRange.x, k), spacing (range / (size - 1)) and
// z spacing k (single image, one 3-component array "ImageScalars") or 1 (image list, three one-component
// arrays per image named from attribute_names, then "attr_<i>").  Written by mops_write_image[s]_vti.
class VTKFileManager {
  public:
    static void SaveVTI(ImageBuffer<double>* img, VisualizationSettings* config, std::string outputName = "output");
    static void SaveVTI(const std::vector<ImageBuffer<double>>& img_list, VisualizationSettings* config,
                        const std::vector<std::string>& attribute_names, const std::string& outputName = "output");
};

// MPASOVisualizer::VisualizeFixedLayer (src/Core/MPASOVisualizer.h:114, MPASOVisualizer.cpp:17-20 ->
// Kernel::VisualizeFixedLayer, MPASOVisualizerKernels.cpp:141-236).  The reference's static takes the
// MPASOField and a runtime context; this one reads the global app's mesh and active front solution, as
// MOPS_RunRemapping does.  Writes {zonal, meridional, 0}
// (alpha 1) at layer ClampLayer((int)config->FixedLayer, nVertLevels) into the pixels of *img that lie inside
// imageSize (ImageBuffer::setPixel's bounds check).  MOPS_RunRemapping itself stays fixed-depth whatever
// VisType says, as in the reference (MOPSApp.cpp:192).
class MPASOVisualizer {
  public:
    static void VisualizeFixedLayer(VisualizationSettings* config, ImageBuffer<double>* img);
};

// Extension (the reference has no teardown): releases the mesh and fields held in HBM by the
// global app.  Call it before the HIP runtime shuts down; nothing is freed from a static
// destructor at exit.
void MOPS_Finalize();

void MOPS_ResetTiming();
void MOPS_PrintTimingSummary();
void MOPS_PrintTimingDetailed();
double MOPS_GetCategoryTime(const char* category);
double MOPS_GetTotalTime();

// MPASOVisualizer::removeNaNTrajectoriesAndReindex (TrajectoryCommon.h:57-129), host form
std::vector<TrajectoryLine> RemoveNaNTrajectoriesAndReindex(std::vector<TrajectoryLine>& lines);

}  // namespace MOPS
