// mops_api.cpp -- the MOPS:: C++ operator API (include/mops/MOPS.h) on top
// of the C ABI.  Mirrors the reference's MOPS.cpp / MOPSApp.cpp state machine
// (src/Core/MOPS.cpp:10-71, src/Core/MOPSApp.cpp:34-337): one global app,
// Init -> Begin -> AddGridMesh -> AddAttribute* -> End -> ActiveAttribute ->
// RunStreamLine / RunPathLine / RunRemapping.  Every computation goes to the HIP
// engine; this file only marshals host containers.
#include "mops/MOPS.h"
#include "mops_io.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>

namespace MOPS {
static_assert(sizeof(CartesianCoord) == 3 * sizeof(double), "CartesianCoord is packed xyz (host <-> device copies)");
namespace {

void Error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::fprintf(stderr, "[Error]: ");
    std::vfprintf(stderr, fmt, ap);
    std::fprintf(stderr, "\n");
    va_end(ap);
}

// ---- TimerManager (src/Utils/Timer.hpp:17-216, categories only) ----------
struct Timing {
    std::map<std::string, double> by_category;
    std::vector<std::pair<std::string, double>> records;
    void add(const std::string& name, const std::string& cat, double ms) {
        by_category[cat] += ms;
        records.emplace_back(name, ms);
    }
};
Timing g_timing;

struct ScopedTimer {
    std::string name, cat;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ScopedTimer(std::string n, std::string c) : name(std::move(n)), cat(std::move(c)) {}
    ~ScopedTimer() {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        g_timing.add(name, cat, ms);
    }
};

enum class State { Idle, Configuring, Ready };

struct App {
    State state = State::Idle;
    std::shared_ptr<MPASOGrid> grid;
    std::map<int, std::shared_ptr<MPASOSolution>> sols;
    mops_mesh* mesh = nullptr;
    std::map<int, mops_field*> fields;
    mops_field* front = nullptr;
    mops_field* back = nullptr;
    int front_id = 0;  // the solution behind `front` (its attributes feed the remapping)
    int back_id = 0;   // the solution behind `back` (attribute sampling along pathlines)
    std::map<int, double*> eddy;  // solID -> vorticity | okubo_weiss vertex arrays [2][V*L] (MOPS_RunEddyMap)
    std::map<int, double*> lavd;  // solID -> the vorticity deviation's vertex array [V*L] (MOPS_RunLAVD)

    void release() {
        for (auto& kv : eddy) (void)hipFree(kv.second);
        eddy.clear();
        for (auto& kv : lavd) (void)hipFree(kv.second);
        lavd.clear();
        for (auto& kv : fields) mops_field_destroy(kv.second);
        fields.clear();
        if (mesh) mops_mesh_destroy(mesh);
        mesh = nullptr;
        front = back = nullptr;
    }
    // No device frees here: g_app is destroyed during static destruction, when the
    // HIP runtime may already be torn down.  Device state is released by MOPS_Init
    // (re-initialisation) and MOPS_Finalize; whatever is left at exit is reclaimed
    // with the process.
    ~App() = default;
};
App g_app;

void check(mops_status st, const char* what) {
    if (st != MOPS_OK) throw std::runtime_error(std::string(what) + ": " + mops_last_error());
}

mops_field* make_field(const MPASOSolution& s) {
    mops_snapshot_desc d{};
    d.timestep = s.mTimesteps;
    d.h_layer_thickness = s.cellLayerThickness_vec.empty() ? nullptr : s.cellLayerThickness_vec.data();
    d.h_bottom_depth = s.cellBottomDepth_vec.empty() ? nullptr : s.cellBottomDepth_vec.data();
    d.h_surface_height = s.cellSurfaceHeight_vec.empty() ? nullptr : s.cellSurfaceHeight_vec.data();
    d.h_zonal_velocity = s.cellZonalVelocity_vec.empty() ? nullptr : s.cellZonalVelocity_vec.data();
    d.h_meridional_velocity = s.cellMeridionalVelocity_vec.empty() ? nullptr : s.cellMeridionalVelocity_vec.data();
    d.h_vert_velocity_top = s.cellVertVelocity_vec.empty() ? nullptr : s.cellVertVelocity_vec.data();
    d.h_normal_velocity = s.cellNormalVelocity_vec.empty() ? nullptr : s.cellNormalVelocity_vec.data();
    mops_field* f = nullptr;
    check(mops_field_create(g_app.mesh, &d, nullptr, &f), "mops_field_create");
    return f;
}

std::vector<TrajectoryLine> run(TrajectorySettings* config, std::vector<CartesianCoord>& pts, bool pathline,
                                const char* stage) {
    if (config == nullptr || g_app.front == nullptr || (pathline && g_app.back == nullptr)) {
        Error("[%s] invalid inputs", stage);  // MPASOVisualizerKernels.cpp:659-662
        return {};
    }
    if (pts.empty()) return {};
    if (config->deltaT == 0 || config->recordT == 0 || config->simulationDuration == 0) {
        Error("[%s] invalid trajectory settings", stage);  // :666-669
        return {};
    }
    // TrajectorySettings::relocateStages (with kRK4 only: Euler has no stages)
    const bool relocate = config->relocateStages && config->methodType == CalcMethodType::kRK4;
    // TrajectorySettings::fixedLayer: the layer mode (mops_run_trajectories_layer), where relocateStages applies to
    // streamlines too
    const int layer = config->fixedLayer;
    if (layer >= 0) {
        if ((size_t)layer >= (size_t)g_app.grid->mVertLevels) {
            Error("[%s] fixedLayer %d outside [0, %d)", stage, layer, (int)g_app.grid->mVertLevels);
            return {};
        }
        if (config->sampleAttributes) {
            Error("[%s] sampleAttributes is not supported with fixedLayer", stage);
            return {};
        }
    }
    if (layer < 0 && relocate && !pathline) {
        Error("[%s] relocateStages is for pathlines only", stage);
        return {};
    }
    if (layer < 0 && relocate && config->sampleAttributes) {
        Error("[%s] sampleAttributes is not supported with relocateStages", stage);
        return {};
    }
    // TrajectorySettings::diffusivity: the random walk (mops_run_trajectories_diffuse / _layer_diffuse)
    const double kh = config->diffusivity;
    if (!(kh >= 0.0) || !std::isfinite(kh)) {
        Error("[%s] diffusivity must be finite and >= 0", stage);
        return {};
    }
    if (kh > 0.0 && layer < 0 && !pathline) {
        Error("[%s] diffusivity needs fixedLayer for streamlines", stage);
        return {};
    }
    if (kh > 0.0 && config->sampleAttributes) {
        Error("[%s] sampleAttributes is not supported with diffusivity", stage);
        return {};
    }
    const mops_diffusion dif{kh, (uint64_t)config->randomSeed, (uint32_t)config->randomEpoch, 0, nullptr};
    const int64_t n = (int64_t)pts.size();
    const bool per_particle = config->hasPerParticleDepths() && config->particle_depths.size() == pts.size();
    std::vector<float> depths(pts.size(), config->depth);  // BuildEffectiveDepths (TrajectoryCommon.h:29-41)
    if (per_particle) depths = config->particle_depths;
    mops_traj_cfg cfg{(int64_t)config->deltaT, (int64_t)config->simulationDuration, (int64_t)config->recordT,
                      config->directionType == CalcDirection::kForward ? MOPS_FORWARD : MOPS_BACKWARD,
                      config->methodType == CalcMethodType::kEuler ? MOPS_EULER
                                                                   : (relocate ? MOPS_RK4_RELOCATE : MOPS_RK4)};
    const int64_t K = mops_traj_num_records(&cfg), steps = mops_traj_num_steps(&cfg);
    std::vector<TrajectoryLine> lines((size_t)n);
    for (int64_t i = 0; i < n; ++i) {  // InitTrajectoryLines (:43-55)
        auto& l = lines[(size_t)i];
        l.lineID = (int)i;
        l.points = {pts[(size_t)i]};
        l.lastPoint = pts[(size_t)i];
        l.duration = (double)config->simulationDuration;
        l.timestamp = (double)config->deltaT;
        l.depth = depths[(size_t)i];
    }
    if (K <= 0 || steps <= 0) {
        Error("[%s] invalid integration steps", stage);  // :709-712 returns the seed-only lines
        return lines;
    }
    const int64_t P = K + 1;
    std::vector<double> hp((size_t)(n * P * 3)), hv((size_t)(n * P * 3)), ht((size_t)(n * P)), hs((size_t)(n * P)),
        hl((size_t)(n * 3));
    if (kh > 0.0) {
        if (layer >= 0)
            check(mops_run_trajectories_layer_diffuse(g_app.mesh, g_app.front, pathline ? g_app.back : nullptr, &cfg,
                                                      layer, &dif, n, reinterpret_cast<const double*>(pts.data()),
                                                      depths.data(), config->depth, nullptr, hp.data(), hv.data(),
                                                      ht.data(), hs.data(), hl.data(), nullptr, nullptr, nullptr,
                                                      nullptr),
                  "mops_run_trajectories_layer_diffuse");
        else
            check(mops_run_trajectories_diffuse(g_app.mesh, g_app.front, g_app.back, &cfg, &dif, n,
                                                reinterpret_cast<const double*>(pts.data()), depths.data(),
                                                config->depth, nullptr, hp.data(), hv.data(), ht.data(), hs.data(),
                                                hl.data(), nullptr, nullptr, nullptr, nullptr),
                  "mops_run_trajectories_diffuse");
    } else if (layer >= 0) {
        check(mops_run_trajectories_layer(g_app.mesh, g_app.front, pathline ? g_app.back : nullptr, &cfg, layer, n,
                                          reinterpret_cast<const double*>(pts.data()), depths.data(), config->depth,
                                          nullptr, hp.data(), hv.data(), ht.data(), hs.data(), hl.data(), nullptr,
                                          nullptr, nullptr, nullptr),
              "mops_run_trajectories_layer");
    } else if (pathline && config->sampleAttributes) {
        // TrajectorySettings::sampleAttributes: the first two names, in std::map order, that both solutions carry
        // (the reference's size() > 1 gate, MPASOVisualizerKernels.cpp:1093, is not kept: one name is enough)
        const auto fs = g_app.sols.find(g_app.front_id), bs = g_app.sols.find(g_app.back_id);
        std::vector<std::string> names;
        if (fs != g_app.sols.end() && bs != g_app.sols.end() && fs->second && bs->second)
            for (const auto& kv : fs->second->mDoubleAttributes)
                if (names.size() < 2 && bs->second->mDoubleAttributes.count(kv.first)) names.push_back(kv.first);
        const size_t VL = (size_t)g_app.grid->mVertexSize * g_app.grid->mVertLevels,
                     CL = (size_t)g_app.grid->mCellsSize * g_app.grid->mVertLevels;
        const int na = (int)names.size();
        struct DevBuf {
            void* p = nullptr;
            ~DevBuf() { (void)hipFree(p); }
        } buf;  // 2 na vertex arrays | one cell staging array
        auto hip = [](hipError_t e, const char* what) {
            if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
        };
        const double* d_fa[2] = {nullptr, nullptr};
        const double* d_ba[2] = {nullptr, nullptr};
        if (na > 0) {
            hip(hipMalloc(&buf.p, (2 * (size_t)na * VL + CL) * sizeof(double)), "MOPS_RunPathLine: hipMalloc");
            double* base = static_cast<double*>(buf.p);
            double* d_cell = base + 2 * (size_t)na * VL;
            for (int k = 0; k < 2 * na; ++k) {  // mDoubleAttributes_CtoV (MOPSApp.cpp:119-127) of both solutions
                const auto& sol = (k < na) ? fs->second : bs->second;
                const auto& vec = sol->mDoubleAttributes.at(names[(size_t)(k % na)]);
                if (vec.size() != CL)
                    throw std::runtime_error("MOPS_RunPathLine: attribute " + names[(size_t)(k % na)] +
                                             " is not [nCells*nVertLevels]");
                double* d_v = base + (size_t)k * VL;
                hip(hipMemcpy(d_cell, vec.data(), CL * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy attribute");
                check(mops_cell_to_vertex_attr(g_app.mesh, d_cell, d_v, nullptr), "mops_cell_to_vertex_attr");
                hip(hipDeviceSynchronize(), "mops_cell_to_vertex_attr");
                (k < na ? d_fa : d_ba)[k % na] = d_v;
            }
        }
        std::vector<double> ha((size_t)(std::max(na, 1) * n * P));
        if (na > 0)
            check(mops_run_pathline_attrs(g_app.mesh, g_app.front, g_app.back, &cfg, n,
                                          reinterpret_cast<const double*>(pts.data()), depths.data(), config->depth,
                                          nullptr, hp.data(), hv.data(), ht.data(), hs.data(), hl.data(), nullptr, nullptr,
                                          nullptr, na, d_fa, d_ba, ha.data(), nullptr),
                  "mops_run_pathline_attrs");
        else
            check(mops_run_trajectories(g_app.mesh, g_app.front, g_app.back, &cfg, n,
                                        reinterpret_cast<const double*>(pts.data()), depths.data(), config->depth, nullptr,
                                        hp.data(), hv.data(), ht.data(), hs.data(), hl.data(), nullptr, nullptr, nullptr,
                                        nullptr),
                  "mops_run_trajectories");
        // temperature / salinity by NAME (map order puts salinity first); zeros for a name that is not sampled
        std::fill(ht.begin(), ht.end(), 0.0);
        std::fill(hs.begin(), hs.end(), 0.0);
        for (int a = 0; a < na; ++a) {
            std::vector<double>* dst = names[(size_t)a] == "temperature" ? &ht : (names[(size_t)a] == "salinity" ? &hs : nullptr);
            if (dst) std::copy(ha.begin() + (size_t)a * n * P, ha.begin() + (size_t)(a + 1) * n * P, dst->begin());
        }
    } else {
        check(mops_run_trajectories(g_app.mesh, g_app.front, pathline ? g_app.back : nullptr, &cfg, n,
                                    reinterpret_cast<const double*>(pts.data()), depths.data(), config->depth, nullptr,
                                    hp.data(), hv.data(), ht.data(), hs.data(), hl.data(), nullptr, nullptr, nullptr,
                                    nullptr),
              "mops_run_trajectories");
    }
    for (int64_t i = 0; i < n; ++i) {  // FinalizeTrajectoryLines[WithAttrs] + RemoveNaN (device-side)
        auto& l = lines[(size_t)i];
        l.points.resize((size_t)P);
        l.velocity.resize((size_t)P);
        l.temperature.resize((size_t)P);
        l.salinity.resize((size_t)P);
        for (int64_t j = 0; j < P; ++j) {
            const size_t q = (size_t)((i * P + j) * 3);
            l.points[(size_t)j] = {hp[q], hp[q + 1], hp[q + 2]};
            l.velocity[(size_t)j] = {hv[q], hv[q + 1], hv[q + 2]};
            l.temperature[(size_t)j] = ht[(size_t)(i * P + j)];
            l.salinity[(size_t)j] = hs[(size_t)(i * P + j)];
        }
        l.lastPoint = {hl[(size_t)(3 * i)], hl[(size_t)(3 * i + 1)], hl[(size_t)(3 * i + 2)]};
    }
    return lines;
}

}  // namespace

// ---- data model setters (MPASOGrid.cpp:82-188, MPASOSolution.cpp:1145-1210) ----
void MPASOGrid::setGridAttribute(GridAttributeType type, int val) {
    switch (type) {
        case GridAttributeType::kCellSize: mCellsSize = val; break;
        case GridAttributeType::kEdgeSize: mEdgesSize = val; break;
        case GridAttributeType::kVertexSize: mVertexSize = val; break;
        case GridAttributeType::kMaxEdgesSize: mMaxEdgesSize = val; break;
        case GridAttributeType::kVertLevels: mVertLevels = val; break;
        case GridAttributeType::kVertLevelsP1: mVertLevelsP1 = val; break;
        default: Error("[MPASOGrid]::Invalid GridAttributeType"); break;
    }
}
void MPASOGrid::setGridAttributesVec3(GridAttributeType type, const std::vector<vec3>& vec) {
    switch (type) {
        case GridAttributeType::kVertexCoord: vertexCoord_vec = vec; break;
        case GridAttributeType::kCellCoord: cellCoord_vec = vec; break;
        case GridAttributeType::kEdgeCoord: edgeCoord_vec = vec; break;
        default: std::cout << "Error: Invalid GridAttributeType" << std::endl;
    }
}
void MPASOGrid::setGridAttributesVec2(GridAttributeType type, const std::vector<vec2>& vec) {
    if (type == GridAttributeType::kVertexLatLon) vertexLatLon_vec = vec;
    else std::cout << "Error: Invalid GridAttributeType" << std::endl;
}
void MPASOGrid::setGridAttributesInt(GridAttributeType type, const std::vector<size_t>& vec) {
    switch (type) {
        case GridAttributeType::kVerticesOnCell: verticesOnCell_vec = vec; break;
        case GridAttributeType::kVerticesOnEdge: verticesOnEdge_vec = vec; break;
        case GridAttributeType::kCellsOnVertex: cellsOnVertex_vec = vec; break;
        case GridAttributeType::kCellsOnCell: cellsOnCell_vec = vec; break;
        case GridAttributeType::kNumberVertexOnCell: numberVertexOnCell_vec = vec; break;
        case GridAttributeType::kCellsOnEdge: cellsOnEdge_vec = vec; break;
        case GridAttributeType::kEdgesOnCell: edgesOnCell_vec = vec; break;
        default: std::cout << "Error: Invalid GridAttributeType" << std::endl;
    }
}
void MPASOGrid::setGridAttributesFloat(GridAttributeType type, const std::vector<float>& vec) {
    if (type == GridAttributeType::kCellWeight) cellWeight_vec = vec;
    else std::cout << "Error: Invalid GridAttributeType" << std::endl;
}
bool MPASOGrid::checkAttribute() const {  // MPASOGrid.cpp:516-598
    return mCellsSize != 0 && mVertexSize != 0 && mMaxEdgesSize != 0 && mVertLevels != 0 && mVertLevelsP1 != 0 &&
           !cellCoord_vec.empty() && !vertexCoord_vec.empty() && !verticesOnCell_vec.empty() &&
           !cellsOnVertex_vec.empty() && !cellsOnCell_vec.empty() && !numberVertexOnCell_vec.empty();
}

void MPASOSolution::setAttribute(GridAttributeType type, int val) {
    switch (type) {
        case GridAttributeType::kCellSize: mCellsSize = val; break;
        case GridAttributeType::kEdgeSize: mEdgesSize = val; break;
        case GridAttributeType::kVertexSize: mVertexSize = val; break;
        case GridAttributeType::kMaxEdgesSize: mMaxEdgesSize = val; break;
        case GridAttributeType::kVertLevels: mVertLevels = val; break;
        case GridAttributeType::kVertLevelsP1: mVertLevelsP1 = val; break;
        default: std::cerr << "[Error]: Invalid GridAttributeType" << std::endl; break;
    }
}
void MPASOSolution::setAttributesDouble(AttributeType type, const std::vector<double>& vec) {
    switch (type) {
        case AttributeType::kZTop: cellZTop_vec = vec; break;
        case AttributeType::kLayerThickness: cellLayerThickness_vec = vec; break;
        case AttributeType::kBottomDepth: cellBottomDepth_vec = vec; break;
        case AttributeType::kZonalVelocity: cellZonalVelocity_vec = vec; break;
        case AttributeType::kMeridionalVelocity: cellMeridionalVelocity_vec = vec; break;
        case AttributeType::kNormalVelocity: cellNormalVelocity_vec = vec; break;
        default: std::cerr << "[Error]: Invalid AttributeType" << std::endl; break;
    }
}
void MPASOSolution::setAttributesVec3(AttributeType type, const std::vector<vec3>& vec) {
    if (type == AttributeType::kVelocity) cellCenterVelocity_vec = vec;
    else std::cerr << "[Error]: Invalid AttributeType" << std::endl;
}
bool MPASOSolution::checkAttribute() const {  // MPASOSolution.cpp:1212-1232
    if (cellZTop_vec.empty() && cellLayerThickness_vec.empty()) {
        std::cerr << "[MPASOSolution]::Error: Invalid ZTop Attribute" << std::endl;
        return false;
    }
    return true;
}

// ---- public API (MOPS.cpp) -------------------------------------------------
void MOPS_Init(const char* device) {
    (void)device;
    g_app.release();
    g_app = App();
    hipDeviceProp_t prop{};
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
        std::cout << " [ system information ]\nDevice selected : " << prop.name << " (" << prop.gcnArchName
                  << ", HIP engine)\n";
    g_app.grid = std::make_shared<MPASOGrid>();
}

void MOPS_Finalize() {
    g_app.release();
    g_app.sols.clear();
    g_app.state = State::Idle;
}

void MOPS_Begin() { g_app.state = State::Configuring; }

void MOPS_AddGridMesh(std::shared_ptr<MPASOGrid> grid) {
    ScopedTimer t("Preprocessing::addGrid", "Preprocessing");
    g_app.grid = std::move(grid);
}

void MOPS_AddAttribute(int solID, std::shared_ptr<MPASOSolution> sol) {
    ScopedTimer t("Preprocessing::addSol", "Preprocessing");
    if (g_app.sols.count(solID)) return;  // MOPSApp.cpp:82-87
    auto& g = *g_app.grid;
    sol->mCellsSize = g.mCellsSize;       // :92-98
    sol->mEdgesSize = g.mEdgesSize;
    sol->mMaxEdgesSize = g.mMaxEdgesSize;
    sol->mVertexSize = g.mVertexSize;
    g.mVertLevels = sol->mVertLevels;
    g.mVertLevelsP1 = sol->mVertLevelsP1;
    g_app.sols[solID] = std::move(sol);
}

void MOPS_End() {
    if (g_app.state != State::Configuring) {  // MOPS.cpp:31-46
        std::cerr << " [ MOPS is not configuring ]\n";
        std::exit(1);
    }
    bool ok = g_app.grid && g_app.grid->checkAttribute();
    for (auto& kv : g_app.sols) ok = ok && kv.second && kv.second->checkAttribute();
    if (!ok) {
        std::cerr << " [ MOPS is not configured ]\n";
        std::exit(1);
    }
    g_app.state = State::Ready;
    ScopedTimer t("Preprocessing::upload", "Preprocessing");
    const auto& g = *g_app.grid;
    mops_mesh_desc d{};
    d.n_cells = g.mCellsSize;
    d.n_vertices = g.mVertexSize;
    d.max_edges = g.mMaxEdgesSize;
    d.n_vert_levels = g.mVertLevels;
    d.h_n_edges_on_cell = reinterpret_cast<const uint64_t*>(g.numberVertexOnCell_vec.data());
    d.h_vertices_on_cell = reinterpret_cast<const uint64_t*>(g.verticesOnCell_vec.data());
    d.h_cells_on_cell = reinterpret_cast<const uint64_t*>(g.cellsOnCell_vec.data());
    d.h_cells_on_vertex = reinterpret_cast<const uint64_t*>(g.cellsOnVertex_vec.data());
    d.h_cell_coord = reinterpret_cast<const double*>(g.cellCoord_vec.data());
    d.h_vertex_coord = reinterpret_cast<const double*>(g.vertexCoord_vec.data());
    g_app.release();
    check(mops_mesh_create(&d, nullptr, &g_app.mesh), "mops_mesh_create");
    // a solution with edge-normal velocity only (AttributeType::kNormalVelocity) is reconstructed by
    // the RBF path (MPASOSolution::calcCellCenterVelocity), which needs the mesh's edges
    bool rbf = false;
    for (auto& kv : g_app.sols)
        rbf = rbf || ((kv.second->cellZonalVelocity_vec.empty() || kv.second->cellMeridionalVelocity_vec.empty()) &&
                      !kv.second->cellNormalVelocity_vec.empty());
    if (rbf)
        check(mops_mesh_set_edges(g_app.mesh, (int64_t)g.edgeCoord_vec.size(),
                                  reinterpret_cast<const uint64_t*>(g.edgesOnCell_vec.data()),
                                  reinterpret_cast<const uint64_t*>(g.cellsOnEdge_vec.data()),
                                  reinterpret_cast<const double*>(g.edgeCoord_vec.data()), nullptr),
              "mops_mesh_set_edges");
    for (auto& kv : g_app.sols) g_app.fields[kv.first] = make_field(*kv.second);
    if (!g_app.fields.empty()) {  // addField: first map entry
        g_app.front = g_app.fields.begin()->second;
        g_app.front_id = g_app.fields.begin()->first;
    }
}

void MOPS_ActiveAttribute(int t1, std::optional<int> t2) {  // MOPSApp.cpp:145-169
    g_app.front = g_app.back = nullptr;
    auto it = g_app.fields.find(t1);
    if (it == g_app.fields.end()) {
        Error("[MOPSApp]::activeAttribute: solID %d not found", t1);
        return;
    }
    if (t2.has_value()) {
        auto it2 = g_app.fields.find(t2.value());
        if (it2 == g_app.fields.end()) {
            Error("[MOPSApp]::activeAttribute: solID %d not found", t2.value());
            return;
        }
        g_app.back = it2->second;
        g_app.back_id = t2.value();
    }
    g_app.front = it->second;
    g_app.front_id = t1;
}

std::vector<TrajectoryLine> MOPS_RunStreamLine(TrajectorySettings* config, std::vector<CartesianCoord>& sample_points) {
    ScopedTimer t("GPUKernel::StreamLine", "GPUKernel");
    return run(config, sample_points, false, "MI355X::StreamLine");
}

std::vector<TrajectoryLine> MOPS_RunPathLine(TrajectorySettings* config, std::vector<CartesianCoord>& sample_points) {
    ScopedTimer t("GPUKernel::PathLine", "GPUKernel");
    if (g_app.front == nullptr || g_app.back == nullptr) {  // MOPSApp.cpp:259-271
        Error("[MOPSApp]::Sol_Front or Sol_Back is nullptr, please activeAttribute first");
        std::exit(-1);
    }
    auto lines = run(config, sample_points, true, "MI355X::PathLine");
    for (size_t i = 0; i < sample_points.size() && i < lines.size(); ++i)  // :287-290
        sample_points[i] = lines[i].lastPoint;
    return lines;
}

std::vector<ImageBuffer<double>> MOPS_RunRemapping(VisualizationSettings* config) {
    ScopedTimer t("GPUKernel::Remapping", "GPUKernel");
    if (config == nullptr || g_app.mesh == nullptr || g_app.front == nullptr) {  // MPASOVisualizerKernels.cpp:240-243
        Error("[MI355X::VisualizeFixedDepth] invalid inputs");
        return {};
    }
    const auto sit = g_app.sols.find(g_app.front_id);
    static const std::map<std::string, std::vector<double>> none;
    const auto& attrs = (sit == g_app.sols.end() || !sit->second) ? none : sit->second->mDoubleAttributes;
    const int n_attr = (int)attrs.size();
    const int W = (int)config->imageSize.x, H = (int)config->imageSize.y;
    const int n_img = mops_remap_num_images(n_attr);
    std::vector<ImageBuffer<double>> img_vec;  // MOPSApp.cpp:173-185
    for (int k = 0; k < n_img; ++k) img_vec.emplace_back(W > 0 ? W : 0, H > 0 ? H : 0);
    if (W <= 0 || H <= 0) {
        Error("[MI355X::VisualizeFixedDepth] invalid image size");
        return img_vec;
    }
    mops_remap_cfg cfg{};
    cfg.width = W; cfg.height = H;
    cfg.min_lat = config->LatRange.x; cfg.max_lat = config->LatRange.y;
    cfg.min_lon = config->LonRange.x; cfg.max_lon = config->LonRange.y;
    cfg.fixed_depth = config->FixedDepth;
    cfg.layer_rule = (int32_t)config->layerRule;
    const size_t px = (size_t)W * H * 4, VL = (size_t)g_app.grid->mVertexSize * g_app.grid->mVertLevels,
                 CL = (size_t)g_app.grid->mCellsSize * g_app.grid->mVertLevels;
    const bool two = n_attr > 1;
    // one allocation: images | two vertex attribute arrays | one cell attribute staging array
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    } buf;
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    hip(hipMalloc(&buf.p, (px * n_img + (two ? 2 * VL + CL : 0)) * sizeof(double)), "MOPS_RunRemapping: hipMalloc");
    double* d_img = static_cast<double*>(buf.p);
    double* d_attr[2] = {nullptr, nullptr};
    if (two) {  // mDoubleAttributes_CtoV: the first two attributes in std::map name order
        double* d_cell = d_img + px * n_img + 2 * VL;
        auto it = attrs.begin();
        for (int k = 0; k < 2; ++k, ++it) {
            if (it->second.size() != CL)
                throw std::runtime_error("MOPS_RunRemapping: attribute " + it->first + " is not [nCells*nVertLevels]");
            d_attr[k] = d_img + px * n_img + (size_t)k * VL;
            hip(hipMemcpy(d_cell, it->second.data(), CL * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy attribute");
            check(mops_cell_to_vertex_attr(g_app.mesh, d_cell, d_attr[k], nullptr), "mops_cell_to_vertex_attr");
            hip(hipDeviceSynchronize(), "mops_cell_to_vertex_attr");
        }
    }
    check(mops_remap_fixed_depth(g_app.mesh, g_app.front, &cfg, n_attr, d_attr[0], d_attr[1], d_img, nullptr, nullptr,
                                 nullptr),
          "mops_remap_fixed_depth");
    for (int k = 0; k < n_img; ++k)
        hip(hipMemcpy(img_vec[(size_t)k].mPixels.data(), d_img + px * k, px * sizeof(double), hipMemcpyDeviceToHost),
            "hipMemcpy image");
    return img_vec;
}

std::vector<ImageBuffer<double>> MOPS_RunEddyMap(VisualizationSettings* config) {
    ScopedTimer t("GPUKernel::EddyMap", "GPUKernel");
    const int W = config ? (int)config->imageSize.x : 0, H = config ? (int)config->imageSize.y : 0;
    if (config == nullptr || g_app.mesh == nullptr || g_app.front == nullptr || W <= 0 || H <= 0) {
        Error("[MI355X::EddyMap] invalid inputs");
        return {};
    }
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    const size_t px = (size_t)W * H * 4, VL = (size_t)g_app.grid->mVertexSize * g_app.grid->mVertLevels,
                 CL = (size_t)g_app.grid->mCellsSize * g_app.grid->mVertLevels;
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    };
    auto cached = g_app.eddy.find(g_app.front_id);
    if (cached == g_app.eddy.end()) {  // the signed vertex arrays of this solution, once
        DevBuf cell, vert;  // vorticity | okubo_weiss per cell; the same per vertex
        hip(hipMalloc(&cell.p, 2 * CL * sizeof(double)), "MOPS_RunEddyMap: hipMalloc");
        hip(hipMalloc(&vert.p, 2 * VL * sizeof(double)), "MOPS_RunEddyMap: hipMalloc");
        double* d_cell = static_cast<double*>(cell.p);
        double* d_vert = static_cast<double*>(vert.p);
        check(mops_velocity_gradient(g_app.mesh, g_app.front, d_cell, nullptr, nullptr, d_cell + CL, nullptr),
              "mops_velocity_gradient");
        for (int k = 0; k < 2; ++k)
            check(mops_cell_to_vertex_signed(g_app.mesh, d_cell + (size_t)k * CL, d_vert + (size_t)k * VL, nullptr),
                  "mops_cell_to_vertex_signed");
        hip(hipDeviceSynchronize(), "MOPS_RunEddyMap");
        cached = g_app.eddy.emplace(g_app.front_id, d_vert).first;
        vert.p = nullptr;
    }
    mops_remap_cfg cfg{};
    cfg.width = W; cfg.height = H;
    cfg.min_lat = config->LatRange.x; cfg.max_lat = config->LatRange.y;
    cfg.min_lon = config->LonRange.x; cfg.max_lon = config->LonRange.y;
    cfg.fixed_depth = config->FixedDepth;
    cfg.layer_rule = (int32_t)config->layerRule;
    DevBuf img;  // image 0 (the velocity) | image 1 {vorticity, okubo_weiss, 0, 1}
    hip(hipMalloc(&img.p, 2 * px * sizeof(double)), "MOPS_RunEddyMap: hipMalloc");
    double* d_img = static_cast<double*>(img.p);
    check(mops_remap_fixed_depth(g_app.mesh, g_app.front, &cfg, 2, cached->second, cached->second + VL, d_img, nullptr,
                                 nullptr, nullptr),
          "mops_remap_fixed_depth");
    std::vector<ImageBuffer<double>> out;
    out.emplace_back(W, H);
    hip(hipMemcpy(out[0].mPixels.data(), d_img + px, px * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy image");
    return out;
}

namespace {

// (width, height, waypoints [n][2], depth range) of a section; false after Error() for invalid inputs
bool section_inputs(const VisualizationSettings* config, const char* who, int& W, int& H, std::vector<double>& way,
                    double& d0, double& d1) {
    if (config == nullptr || (int)config->imageSize.x <= 0 || (int)config->imageSize.y <= 0) {
        Error("[MI355X::%s] invalid inputs", who);
        return false;
    }
    W = (int)config->imageSize.x; H = (int)config->imageSize.y;
    way.clear();
    for (const vec2& p : config->SectionPath) { way.push_back(p.x); way.push_back(p.y); }
    d0 = config->DepthRange.x; d1 = config->DepthRange.y;
    if (d0 == 0.0 && d1 == 0.0) {
        if (g_app.grid == nullptr || g_app.grid->cellRefBottomDepth_vec.empty()) {
            Error("[MI355X::%s] refBottomDepth is empty", who);
            return false;
        }
        d0 = g_app.grid->cellRefBottomDepth_vec.front(); d1 = g_app.grid->cellRefBottomDepth_vec.back();
    }
    return true;
}

}  // namespace

std::vector<ImageBuffer<double>> MOPS_RunRemappingSection(VisualizationSettings* config) {
    ScopedTimer t("GPUKernel::Section", "GPUKernel");
    int W = 0, H = 0;
    double d0 = 0.0, d1 = 0.0;
    std::vector<double> way;
    if (!section_inputs(config, "Section", W, H, way, d0, d1)) return {};
    if (g_app.mesh == nullptr || g_app.front == nullptr) {
        Error("[MI355X::Section] invalid inputs");
        return {};
    }
    std::vector<double> pts(3 * (size_t)W), nrm(3 * (size_t)W), dist((size_t)W);
    if (mops_section_points((int32_t)(way.size() / 2), way.data(), W, pts.data(), nrm.data(), dist.data()) != MOPS_OK) {
        Error("[MI355X::Section] %s", mops_last_error());
        return {};
    }
    const auto sit = g_app.sols.find(g_app.front_id);
    static const std::map<std::string, std::vector<double>> none;
    const auto& attrs = (sit == g_app.sols.end() || !sit->second) ? none : sit->second->mDoubleAttributes;
    const int n_attr = attrs.size() > 2 ? 2 : (int)attrs.size();
    const int n_img = n_attr > 0 ? 2 : 1;
    const size_t px = (size_t)W * H * 4, VL = (size_t)g_app.grid->mVertexSize * g_app.grid->mVertLevels,
                 CL = (size_t)g_app.grid->mCellsSize * g_app.grid->mVertLevels;
    // one allocation: images | the vertex attribute arrays | one cell attribute staging array
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    } buf;
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    hip(hipMalloc(&buf.p, (px * n_img + (n_attr ? n_attr * VL + CL : 0)) * sizeof(double)),
        "MOPS_RunRemappingSection: hipMalloc");
    double* d_img = static_cast<double*>(buf.p);
    double* d_attr[2] = {nullptr, nullptr};
    if (n_attr) {  // the first attributes in std::map name order, as MOPS_RunRemapping's
        double* d_cell = d_img + px * n_img + (size_t)n_attr * VL;
        auto it = attrs.begin();
        for (int k = 0; k < n_attr; ++k, ++it) {
            if (it->second.size() != CL)
                throw std::runtime_error("MOPS_RunRemappingSection: attribute " + it->first +
                                         " is not [nCells*nVertLevels]");
            d_attr[k] = d_img + px * n_img + (size_t)k * VL;
            hip(hipMemcpy(d_cell, it->second.data(), CL * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy attribute");
            check(mops_cell_to_vertex_attr(g_app.mesh, d_cell, d_attr[k], nullptr), "mops_cell_to_vertex_attr");
            hip(hipDeviceSynchronize(), "mops_cell_to_vertex_attr");
        }
    }
    check(mops_remap_section(g_app.mesh, g_app.front, W, H, d0, d1, pts.data(), nrm.data(), n_attr, d_attr[0], d_attr[1],
                             d_img, n_attr ? d_img + px : nullptr, nullptr, nullptr),
          "mops_remap_section");
    std::vector<ImageBuffer<double>> img_vec;
    for (int k = 0; k < n_img; ++k) {
        img_vec.emplace_back(W, H);
        hip(hipMemcpy(img_vec[(size_t)k].mPixels.data(), d_img + px * k, px * sizeof(double), hipMemcpyDeviceToHost),
            "hipMemcpy image");
    }
    return img_vec;
}

double MOPS_SectionTransport(const ImageBuffer<double>& image, VisualizationSettings* config) {
    ScopedTimer t("Section::Transport", "GPUKernel");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    int W = 0, H = 0;
    double d0 = 0.0, d1 = 0.0;
    std::vector<double> way;
    if (!section_inputs(config, "SectionTransport", W, H, way, d0, d1)) return nan;
    if (image.mPixels.size() != (size_t)W * H * 4) {
        Error("[MI355X::SectionTransport] the image is not imageSize");
        return nan;
    }
    std::vector<double> pts(3 * (size_t)W), nrm(3 * (size_t)W), dist((size_t)W);
    double sv = nan, area = 0.0;
    if (mops_section_points((int32_t)(way.size() / 2), way.data(), W, pts.data(), nrm.data(), dist.data()) != MOPS_OK ||
        mops_section_transport(W, H, image.mPixels.data(), dist.data(), d0, d1, &sv, &area) != MOPS_OK) {
        Error("[MI355X::SectionTransport] %s", mops_last_error());
        return nan;
    }
    return sv;
}

ImageBuffer<double> MOPS_RunDensity(const std::vector<TrajectoryLine>& lines, VisualizationSettings* config,
                                    const std::string& value) {
    ScopedTimer t("GPUKernel::Density", "GPUKernel");
    const int W = config ? (int)config->imageSize.x : 0, H = config ? (int)config->imageSize.y : 0;
    const int kind = value.empty() ? MOPS_DENSITY_COUNT : value == "speed" ? MOPS_DENSITY_SPEED : MOPS_DENSITY_VALUES;
    if (config == nullptr || W <= 0 || H <= 0 ||
        (kind == MOPS_DENSITY_VALUES && value != "temperature" && value != "salinity")) {
        Error("[MI355X::Density] invalid inputs");
        return ImageBuffer<double>(W > 0 ? W : 0, H > 0 ? H : 0);
    }
    mops_remap_cfg cfg{};
    cfg.width = W; cfg.height = H;
    cfg.min_lat = config->LatRange.x; cfg.max_lat = config->LatRange.y;
    cfg.min_lon = config->LonRange.x; cfg.max_lon = config->LonRange.y;
    const int64_t acc_bytes = mops_density_bytes(W, H);
    ImageBuffer<double> img(W, H);
    if (acc_bytes < 0) {
        Error("[MI355X::Density] invalid image size");
        return ImageBuffer<double>();
    }
    // lines [n][P][C] (C = 6 with the velocity behind the point for "speed"), shorter lines padded with NaN
    // points, which the binning skips; values [n][P]
    const size_t n = lines.size();
    size_t P = 0;
    for (const auto& ln : lines) P = std::max(P, ln.points.size());
    const size_t C = kind == MOPS_DENSITY_SPEED ? 6 : 3;
    const double nan = std::nan("");
    std::vector<double> pts(n * P * C, nan), val(kind == MOPS_DENSITY_VALUES ? n * P : 0, nan);
    for (size_t i = 0; i < n; ++i) {
        const auto& ln = lines[i];
        const auto& v = value == "temperature" ? ln.temperature : ln.salinity;
        for (size_t k = 0; k < ln.points.size(); ++k) {
            double* o = &pts[(i * P + k) * C];
            std::memcpy(o, &ln.points[k], 3 * sizeof(double));
            if (kind == MOPS_DENSITY_SPEED && k < ln.velocity.size()) std::memcpy(o + 3, &ln.velocity[k], 3 * sizeof(double));
            if (kind == MOPS_DENSITY_VALUES && k < v.size()) val[i * P + k] = v[k];
        }
    }
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    } buf;
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    // one allocation: image | accumulator | points | values
    const size_t px = (size_t)W * H * 4;
    hip(hipMalloc(&buf.p, px * sizeof(double) + (size_t)acc_bytes + (pts.size() + val.size() + 1) * sizeof(double)),
        "MOPS_RunDensity: hipMalloc");
    double* d_img = static_cast<double*>(buf.p);
    void* d_acc = d_img + px;
    double* d_pts = d_img + px + (size_t)acc_bytes / sizeof(double);
    double* d_val = d_pts + pts.size();
    hip(hipMemset(d_acc, 0, (size_t)acc_bytes), "MOPS_RunDensity: hipMemset");
    if (!pts.empty()) hip(hipMemcpy(d_pts, pts.data(), pts.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy points");
    if (!val.empty()) hip(hipMemcpy(d_val, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy values");
    mops_status st = mops_density_accumulate(&cfg, (int64_t)n, 0, (int64_t)P, d_pts, (int64_t)C, (int64_t)(C * P), 1, nullptr,
                                             kind, kind == MOPS_DENSITY_VALUES ? d_val : nullptr, 1, (int64_t)P, d_acc,
                                             nullptr);
    if (st == MOPS_OK) st = mops_density_image(&cfg, d_acc, 1, d_img, nullptr);
    if (st == MOPS_ERR_INVALID) {  // (the window: an empty or non-finite range)
        Error("[MI355X::Density] %s", mops_last_error());
        return ImageBuffer<double>();
    }
    check(st, "mops_density_accumulate");
    hip(hipMemcpy(img.mPixels.data(), d_img, px * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy image");
    return img;
}

std::vector<CartesianCoord> MOPS_LatticeSeeds(VisualizationSettings* config) {
    ScopedTimer t("GPUKernel::LatticeSeeds", "GPUKernel");
    const int W = config ? (int)config->imageSize.x : 0, H = config ? (int)config->imageSize.y : 0;
    if (config == nullptr || W <= 0 || H <= 0 || (int64_t)W * H >= (1LL << 31)) {
        Error("[MI355X::LatticeSeeds] invalid inputs");
        return {};
    }
    mops_remap_cfg cfg{};
    cfg.width = W; cfg.height = H;
    cfg.min_lat = config->LatRange.x; cfg.max_lat = config->LatRange.y;
    cfg.min_lon = config->LonRange.x; cfg.max_lon = config->LonRange.y;
    static_assert(sizeof(CartesianCoord) == 3 * sizeof(double), "CartesianCoord is three doubles");
    std::vector<CartesianCoord> seeds((size_t)W * H);
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    } buf;
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    hip(hipMalloc(&buf.p, seeds.size() * sizeof(CartesianCoord)), "MOPS_LatticeSeeds: hipMalloc");
    check(mops_flowmap_lattice(&cfg, static_cast<double*>(buf.p), nullptr), "mops_flowmap_lattice");
    hip(hipMemcpy(seeds.data(), buf.p, seeds.size() * sizeof(CartesianCoord), hipMemcpyDeviceToHost), "hipMemcpy seeds");
    return seeds;
}

ImageBuffer<double> MOPS_RunFTLE(const std::vector<TrajectoryLine>& lines, VisualizationSettings* config,
                                 double horizon) {
    ScopedTimer t("GPUKernel::FTLE", "GPUKernel");
    const int W = config ? (int)config->imageSize.x : 0, H = config ? (int)config->imageSize.y : 0;
    if (config == nullptr || W <= 0 || H <= 0 || (int64_t)W * H >= (1LL << 31) || lines.size() != (size_t)W * H ||
        !std::isfinite(horizon) || !(horizon > 0.0)) {
        Error("[MI355X::FTLE] invalid inputs");
        return ImageBuffer<double>();
    }
    mops_remap_cfg cfg{};
    cfg.width = W; cfg.height = H;
    cfg.min_lat = config->LatRange.x; cfg.max_lat = config->LatRange.y;
    cfg.min_lon = config->LonRange.x; cfg.max_lon = config->LonRange.y;
    const int wrap = (config->LonRange.y - config->LonRange.x == 360.0) ? 1 : 0;
    // seeds | last points, [n][3] each; a line without points keeps zeros, which are not valid
    const size_t n = lines.size();
    std::vector<double> host(6 * n, 0.0);
    for (size_t i = 0; i < n; ++i) {
        if (lines[i].points.empty()) continue;
        std::memcpy(&host[3 * i], &lines[i].points[0], 3 * sizeof(double));
        std::memcpy(&host[3 * (n + i)], &lines[i].lastPoint, 3 * sizeof(double));
    }
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    } buf;
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    // one allocation: image | seeds | last points
    const size_t px = n * 4;
    hip(hipMalloc(&buf.p, (px + host.size()) * sizeof(double)), "MOPS_RunFTLE: hipMalloc");
    double* d_img = static_cast<double*>(buf.p);
    double* d_seeds = d_img + px;
    hip(hipMemcpy(d_seeds, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy lines");
    check(mops_ftle_image(&cfg, d_seeds, d_seeds + 3 * n, nullptr, horizon, wrap, d_img, nullptr), "mops_ftle_image");
    ImageBuffer<double> img(W, H);
    hip(hipMemcpy(img.mPixels.data(), d_img, px * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy image");
    return img;
}

namespace {

// The vorticity deviation of solution `id` as a signed vertex array [V*L] on the device, once per solution id:
// mops_velocity_gradient's vorticity, minus mops_level_mean of it under mops_cell_area's weights (one IEEE
// subtraction per element, on the host), through mops_cell_to_vertex_signed.
const double* lavd_vertex_attr(int id, mops_field* field) {
    auto cached = g_app.lavd.find(id);
    if (cached != g_app.lavd.end()) return cached->second;
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    } cell, vert;  // vorticity [C*L] | area [C] | mean [L] | wsum [L]; the vertex array
    const size_t C = g_app.grid->mCellsSize, L = g_app.grid->mVertLevels, CL = C * L,
                 VL = (size_t)g_app.grid->mVertexSize * L;
    hip(hipMalloc(&cell.p, (CL + C + 2 * L) * sizeof(double)), "MOPS_RunLAVD: hipMalloc");
    hip(hipMalloc(&vert.p, VL * sizeof(double)), "MOPS_RunLAVD: hipMalloc");
    double* d_vort = static_cast<double*>(cell.p);
    double* d_area = d_vort + CL;
    double* d_mean = d_area + C;
    check(mops_velocity_gradient(g_app.mesh, field, d_vort, nullptr, nullptr, nullptr, nullptr), "mops_velocity_gradient");
    check(mops_cell_area(g_app.mesh, d_area, nullptr), "mops_cell_area");
    check(mops_level_mean((int64_t)C, (int32_t)L, d_vort, d_area, d_mean, d_mean + L, nullptr), "mops_level_mean");
    std::vector<double> vort(CL), mean(L);
    hip(hipMemcpy(vort.data(), d_vort, CL * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy vorticity");
    hip(hipMemcpy(mean.data(), d_mean, L * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy mean");
    for (size_t c = 0; c < C; ++c)
        for (size_t l = 0; l < L; ++l) vort[c * L + l] = vort[c * L + l] - mean[l];
    hip(hipMemcpy(d_vort, vort.data(), CL * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy deviation");
    check(mops_cell_to_vertex_signed(g_app.mesh, d_vort, static_cast<double*>(vert.p), nullptr),
          "mops_cell_to_vertex_signed");
    hip(hipDeviceSynchronize(), "MOPS_RunLAVD");
    double* out = static_cast<double*>(vert.p);
    g_app.lavd.emplace(id, out);
    vert.p = nullptr;
    return out;
}

}  // namespace

ImageBuffer<double> MOPS_RunLAVD(VisualizationSettings* config, TrajectorySettings* traj) {
    ScopedTimer t("GPUKernel::LAVD", "GPUKernel");
    if (config == nullptr || traj == nullptr || g_app.mesh == nullptr || g_app.front == nullptr ||
        g_app.back == nullptr) {
        Error("[MI355X::LAVD] invalid inputs: it needs both settings and an active front / back pair");
        return ImageBuffer<double>();
    }
    if (traj->fixedLayer >= 0) {
        Error("[MI355X::LAVD] attributes are not sampled with fixedLayer");
        return ImageBuffer<double>();
    }
    if (traj->relocateStages) {
        Error("[MI355X::LAVD] attributes are not sampled with relocateStages");
        return ImageBuffer<double>();
    }
    if (!(traj->diffusivity == 0.0)) {
        Error("[MI355X::LAVD] attributes are not sampled with diffusivity > 0");
        return ImageBuffer<double>();
    }
    mops_traj_cfg cfg{(int64_t)traj->deltaT, (int64_t)traj->simulationDuration, (int64_t)traj->recordT,
                      traj->directionType == CalcDirection::kForward ? MOPS_FORWARD : MOPS_BACKWARD,
                      traj->methodType == CalcMethodType::kEuler ? MOPS_EULER : MOPS_RK4};
    const int64_t K = mops_traj_num_records(&cfg), steps = mops_traj_num_steps(&cfg);
    if (K <= 0 || steps <= 0) {
        Error("[MI355X::LAVD] invalid trajectory settings");
        return ImageBuffer<double>();
    }
    const int W = (int)config->imageSize.x, H = (int)config->imageSize.y;
    if (W <= 0 || H <= 0 || (int64_t)W * H >= (1LL << 31)) {
        Error("[MI355X::LAVD] invalid inputs");
        return ImageBuffer<double>();
    }
    mops_remap_cfg rc{};
    rc.width = W; rc.height = H;
    rc.min_lat = config->LatRange.x; rc.max_lat = config->LatRange.y;
    rc.min_lon = config->LonRange.x; rc.max_lon = config->LonRange.y;
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    } buf;  // image [n][4] | seeds [n][3] | attribute lines [n][K+1] | sums [n] | death steps [n] (int32)
    const size_t n = (size_t)W * H, P = (size_t)K + 1;
    hip(hipMalloc(&buf.p, (n * 4 + n * 3 + n * P + n) * sizeof(double) + n * sizeof(int32_t)), "MOPS_RunLAVD: hipMalloc");
    double* d_img = static_cast<double*>(buf.p);
    double* d_seeds = d_img + n * 4;
    double* d_lines = d_seeds + n * 3;
    double* d_sum = d_lines + n * P;
    int32_t* d_death = reinterpret_cast<int32_t*>(d_sum + n);
    check(mops_flowmap_lattice(&rc, d_seeds, nullptr), "mops_flowmap_lattice");
    std::vector<double> seeds(n * 3);
    hip(hipMemcpy(seeds.data(), d_seeds, seeds.size() * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy seeds");
    const double* d_fa[1] = {lavd_vertex_attr(g_app.front_id, g_app.front)};
    const double* d_ba[1] = {lavd_vertex_attr(g_app.back_id, g_app.back)};
    std::vector<double> hp(n * P * 3), lines(n * P);
    std::vector<int32_t> death(n);
    check(mops_run_pathline_attrs(g_app.mesh, g_app.front, g_app.back, &cfg, (int64_t)n, seeds.data(), nullptr,
                                  (float)config->FixedDepth, nullptr, hp.data(), nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, death.data(), 1, d_fa, d_ba, lines.data(), nullptr),
          "mops_run_pathline_attrs");
    hip(hipMemcpy(d_lines, lines.data(), lines.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy lines");
    hip(hipMemcpy(d_death, death.data(), n * sizeof(int32_t), hipMemcpyHostToDevice), "hipMemcpy death steps");
    hip(hipMemset(d_sum, 0, n * sizeof(double)), "hipMemset");
    const double record_s = std::fabs((double)cfg.record_t);
    check(mops_path_integral_abs((int64_t)n, 0, K, d_lines, 1, (int64_t)P, nullptr, record_s, d_sum, nullptr),
          "mops_path_integral_abs");
    check(mops_path_integral_image((int64_t)n, d_sum, d_death, (double)K * record_s, d_img, nullptr),
          "mops_path_integral_image");
    ImageBuffer<double> img(W, H);
    hip(hipMemcpy(img.mPixels.data(), d_img, n * 4 * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy image");
    return img;
}

EddyCensus MOPS_RunEddyCensus(VisualizationSettings* config) {
    ScopedTimer t("GPUKernel::EddyCensus", "GPUKernel");
    const int W = config ? (int)config->imageSize.x : 0, H = config ? (int)config->imageSize.y : 0;
    if (config == nullptr || g_app.mesh == nullptr || g_app.front == nullptr || W <= 0 || H <= 0) {
        Error("[MI355X::EddyCensus] invalid inputs");
        return {};
    }
    if (!std::isfinite(config->EddyThreshold) || config->EddyMinCells < 1) {
        Error("[MI355X::EddyCensus] EddyThreshold must be finite and EddyMinCells at least 1");
        return {};
    }
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    };
    const size_t C = g_app.grid->mCellsSize, L = g_app.grid->mVertLevels, CL = C * L, px = (size_t)W * H;
    const double fl = config->FixedLayer;  // VisualizeFixedLayer's ClampLayer((int)FixedLayer, L)
    const int layer = !(fl >= 1.0) ? 0 : (fl >= (double)L ? (int)L - 1 : (int)fl);
    DevBuf grad, area, ints, img, cells;  // vorticity | okubo_weiss; area; class | component | eddy_of_cell
    hip(hipMalloc(&grad.p, 2 * CL * sizeof(double)), "MOPS_RunEddyCensus: hipMalloc");
    hip(hipMalloc(&area.p, C * sizeof(double)), "MOPS_RunEddyCensus: hipMalloc");
    hip(hipMalloc(&ints.p, 3 * C * sizeof(int32_t)), "MOPS_RunEddyCensus: hipMalloc");
    hip(hipMalloc(&img.p, px * 4 * sizeof(double)), "MOPS_RunEddyCensus: hipMalloc");
    hip(hipMalloc(&cells.p, px * sizeof(int32_t)), "MOPS_RunEddyCensus: hipMalloc");
    double* d_vort = static_cast<double*>(grad.p);
    double* d_ow = d_vort + CL;
    int32_t* d_class = static_cast<int32_t*>(ints.p);
    int32_t* d_comp = d_class + C;
    int32_t* d_eddy = d_class + 2 * C;
    check(mops_velocity_gradient(g_app.mesh, g_app.front, d_vort, nullptr, nullptr, d_ow, nullptr),
          "mops_velocity_gradient");
    // sigma: the population standard deviation of the layer's finite Okubo-Weiss values, two passes in FP64
    // (the layer's column alone comes to the host: a strided copy of C doubles, not the [C*L] array)
    std::vector<double> ow(C);
    hip(hipMemcpy2D(ow.data(), sizeof(double), d_ow + layer, L * sizeof(double), sizeof(double), C,
                    hipMemcpyDeviceToHost),
        "hipMemcpy2D okubo_weiss");
    double sum = 0.0, ss = 0.0;
    size_t n = 0;
    for (size_t c = 0; c < C; ++c)
        if (std::isfinite(ow[c])) { sum += ow[c]; ++n; }
    const double mean = n ? sum / (double)n : 0.0;
    for (size_t c = 0; c < C; ++c)
        if (std::isfinite(ow[c])) ss += (ow[c] - mean) * (ow[c] - mean);
    const double threshold = n ? -config->EddyThreshold * std::sqrt(ss / (double)n) : NAN;
    if (!std::isfinite(threshold)) {
        Error("[MI355X::EddyCensus] no finite Okubo-Weiss value in the layer: no threshold");
        return {};
    }
    check(mops_eddy_classify(g_app.mesh, d_ow, d_vort, layer, threshold, d_class, nullptr), "mops_eddy_classify");
    check(mops_label_components(g_app.mesh, d_class, d_comp, nullptr, nullptr), "mops_label_components");
    check(mops_cell_area(g_app.mesh, static_cast<double*>(area.p), nullptr), "mops_cell_area");
    int64_t E = 0;
    check(mops_eddy_count(g_app.mesh, d_comp, config->EddyMinCells, d_eddy, &E, nullptr), "mops_eddy_count");
    std::vector<int32_t> root(E), n_cells(E), polarity(E), core(E);
    std::vector<double> sum_area(E), circ(E), ow_min(E), centre(3 * (size_t)E);
    check(mops_eddy_table(g_app.mesh, d_eddy, E, d_class, static_cast<double*>(area.p), d_vort, d_ow, layer,
                          root.data(), n_cells.data(), polarity.data(), core.data(), sum_area.data(), circ.data(),
                          ow_min.data(), centre.data(), nullptr),
          "mops_eddy_table");
    EddyCensus out;
    out.threshold = threshold;
    out.eddies.resize((size_t)E);
    const double deg = 180.0 / M_PI;
    for (int64_t e = 0; e < E; ++e) {
        Eddy& d = out.eddies[(size_t)e];
        d.index = (int)e;
        d.centre = {centre[3 * e], centre[3 * e + 1], centre[3 * e + 2]};
        d.lat = std::asin(d.centre.z) * deg;
        d.lon = std::atan2(d.centre.y, d.centre.x) * deg;
        d.area = sum_area[e];
        d.radius = std::sqrt(d.area / M_PI);
        d.polarity = polarity[e];
        d.circulation = circ[e];
        d.n_cells = n_cells[e];
        d.root = root[e];
        d.core_cell = core[e];
        d.ow_min = ow_min[e];
    }
    std::vector<int32_t> cls(C), eddy(C), cell(px);
    hip(hipMemcpy(cls.data(), d_class, C * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy classes");
    hip(hipMemcpy(eddy.data(), d_eddy, C * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy labels");
    out.labels.assign(eddy.begin(), eddy.end());
    // the label image from the fixed-layer remapping's cell map
    mops_remap_cfg cfg{};
    cfg.width = W; cfg.height = H;
    cfg.min_lat = config->LatRange.x; cfg.max_lat = config->LatRange.y;
    cfg.min_lon = config->LonRange.x; cfg.max_lon = config->LonRange.y;
    cfg.fixed_layer = (double)layer;
    check(mops_remap_fixed_layer(g_app.mesh, g_app.front, &cfg, static_cast<double*>(img.p),
                                 static_cast<int32_t*>(cells.p), nullptr),
          "mops_remap_fixed_layer");
    out.image = ImageBuffer<double>(W, H);
    hip(hipMemcpy(out.image.mPixels.data(), img.p, px * 4 * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy image");
    hip(hipMemcpy(cell.data(), cells.p, px * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy cells");
    for (size_t i = 0; i < px; ++i) {
        double* p = &out.image.mPixels[4 * i];
        const int32_t c = cell[i];
        const bool ok = c >= 0 && (size_t)c < C && !std::isnan(p[0]) && eddy[c] >= 0;
        p[0] = ok ? (double)eddy[c] : NAN;
        p[1] = ok ? (double)cls[c] : NAN;
        p[2] = 0.0;
        p[3] = 1.0;
    }
    return out;
}

void MPASOVisualizer::VisualizeFixedLayer(VisualizationSettings* config, ImageBuffer<double>* img) {
    ScopedTimer t("GPUKernel::FixedLayer", "GPUKernel");
    if (config == nullptr || img == nullptr || g_app.mesh == nullptr || g_app.front == nullptr) {  // :143-146
        Error("[MI355X::VisualizeFixedLayer] invalid inputs");
        return;
    }
    const int W = (int)config->imageSize.x, H = (int)config->imageSize.y;
    if (W <= 0 || H <= 0) {  // :158-161
        Error("[MI355X::VisualizeFixedLayer] invalid image size or layer metadata");
        return;
    }
    mops_remap_cfg cfg{};
    cfg.width = W; cfg.height = H;
    cfg.min_lat = config->LatRange.x; cfg.max_lat = config->LatRange.y;
    cfg.min_lon = config->LonRange.x; cfg.max_lon = config->LonRange.y;
    cfg.fixed_layer = config->FixedLayer;
    const size_t px = (size_t)W * H * 4;
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    } buf;
    if (hipMalloc(&buf.p, px * sizeof(double)) != hipSuccess) throw std::runtime_error("VisualizeFixedLayer: hipMalloc");
    check(mops_remap_fixed_layer(g_app.mesh, g_app.front, &cfg, static_cast<double*>(buf.p), nullptr, nullptr),
          "mops_remap_fixed_layer");
    std::vector<double> host(px);
    if (hipMemcpy(host.data(), buf.p, px * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        throw std::runtime_error("VisualizeFixedLayer: hipMemcpy");
    for (int i = 0; i < H && i < img->getHeight(); ++i)  // img->setPixel: in-bounds pixels only
        for (int j = 0; j < W && j < img->getWidth(); ++j)
            std::memcpy(&img->mPixels[(size_t)img->getIndex(i, j)], &host[((size_t)i * W + j) * 4], 4 * sizeof(double));
}

bool SaveToPNG(const ImageBuffer<double>& buffer, const std::string& filename, int channel) {
    const int w = buffer.getWidth(), h = buffer.getHeight();
    if (channel < 0 || channel > 3 || w <= 0 || h <= 0 || buffer.mPixels.size() < (size_t)w * h * 4) return false;  // :98
    std::vector<uint8_t> rgba((size_t)w * h * 4);
    if (mops_colormap_image(buffer.mPixels.data(), w, h, 1 << channel, rgba.data(), nullptr, nullptr) != MOPS_OK) {
        Error("SaveToPNG: %s", mops_last_error());
        return false;
    }
    return mops_write_png_rgba8(filename.c_str(), w, h, rgba.data()) == MOPS_OK;
}

namespace {
// the file name and geometry both SaveVTI overloads share (VTKFileManager.hpp:27-36, :86-90)
struct VtiGeometry {
    int W, H;
    double origin[3], spacing[3];
    std::string file;
};
VtiGeometry vti_geometry(const VisualizationSettings& c, const std::string& outputName, bool single) {
    VtiGeometry g;
    g.W = (int)c.imageSize.x; g.H = (int)c.imageSize.y;
    const double latSpacing = (c.LatRange.y - c.LatRange.x) / (c.imageSize.y - 1);
    const double lonSpacing = (c.LonRange.y - c.LonRange.x) / (c.imageSize.x - 1);
    const double k = (c.VisType == VisualizeType::kFixedDepth) ? c.FixedDepth : c.FixedLayer;
    g.origin[0] = c.LonRange.x; g.origin[1] = c.LatRange.x; g.origin[2] = k;
    g.spacing[0] = lonSpacing; g.spacing[1] = latSpacing; g.spacing[2] = single ? k : 1.0;  // :47 / :95
    g.file = outputName + "_" + TypeToStr(c.VisType) + std::to_string(k) + ".vti";
    return g;
}
}  // namespace

void VTKFileManager::SaveVTI(ImageBuffer<double>* img, VisualizationSettings* config, std::string outputName) {
    if (!config) return;
    if (!img) {  // :50-53
        Error("SaveVTI:: ImageBuffer is nullptr.....");
        return;
    }
    const VtiGeometry g = vti_geometry(*config, outputName, true);
    if (g.W != img->getWidth() || g.H != img->getHeight()) {  // :59-63 skips every pixel outside the image
        Error("SaveVTI:: imageSize %d x %d differs from the image's %d x %d", g.W, g.H, img->getWidth(), img->getHeight());
        return;
    }
    if (mops_write_image_vti(g.file.c_str(), g.W, g.H, img->mPixels.data(), g.origin, g.spacing) != MOPS_OK)
        Error("SaveVTI: %s", mops_last_error());
}

void VTKFileManager::SaveVTI(const std::vector<ImageBuffer<double>>& img_list, VisualizationSettings* config,
                             const std::vector<std::string>& attribute_names, const std::string& outputName) {
    if (!config || img_list.empty()) return;
    const VtiGeometry g = vti_geometry(*config, outputName, false);
    const size_t px = (size_t)(g.W > 0 ? g.W : 0) * (size_t)(g.H > 0 ? g.H : 0) * 4;
    std::vector<double> all;
    all.reserve(px * img_list.size());
    for (const auto& img : img_list) {
        if (img.getWidth() != g.W || img.getHeight() != g.H || img.mPixels.size() != px) {
            Error("SaveVTI:: imageSize %d x %d differs from an image's %d x %d", g.W, g.H, img.getWidth(), img.getHeight());
            return;
        }
        all.insert(all.end(), img.mPixels.begin(), img.mPixels.end());
    }
    std::vector<const char*> names;
    for (const auto& s : attribute_names) names.push_back(s.c_str());
    if (mops_write_images_vti(g.file.c_str(), (int32_t)img_list.size(), g.W, g.H, all.data(), g.origin, g.spacing,
                              names.empty() ? nullptr : names.data(), (int32_t)names.size()) != MOPS_OK)
        Error("SaveVTI: %s", mops_last_error());
}

void MOPS_GenerateSamplePoints(SamplingSettings* config, std::vector<CartesianCoord>& points) {
    if (config->isAtCellCenter()) {  // MOPSApp::generateSamplePointsAtCenter
        for (const auto& p : g_app.grid->cellCoord_vec) points.push_back(p);
        return;
    }
    // MPASOVisualizer::GenerateSamplePoint (MPASOVisualizer.cpp:120-149):
    // exclusive upper bounds, accumulated steps, r = 6371010.0f.  Like the
    // reference, the conversion pass runs over the WHOLE vector, so points the
    // caller passed in are re-converted too.
    const double minLat = config->getLatitudeRange().x, maxLat = config->getLatitudeRange().y;
    const double minLon = config->getLongitudeRange().x, maxLon = config->getLongitudeRange().y;
    const double i_step = (maxLat - minLat) / static_cast<double>(config->getSampleRange().x - 1);
    const double j_step = (maxLon - minLon) / static_cast<double>(config->getSampleRange().y - 1);
    for (double i = minLat; i < maxLat; i += i_step)
        for (double j = minLon; j < maxLon; j += j_step) points.push_back({j, i, config->getDepth()});
    const double r = 6371010.0f;
    for (size_t k = 0; k < points.size(); ++k) {
        const double lat = points[k].y * (M_PI / 180.0), lon = points[k].x * (M_PI / 180.0);
        const double ct = std::cos(lat), cp = std::cos(lon), st = std::sin(lat), sp = std::sin(lon);
        points[k] = {r * ct * cp, r * ct * sp, r * st};
    }
}

void MOPS_ResetTiming() { g_timing = Timing(); }
void MOPS_PrintTimingSummary() {
    std::cout << "==== MOPS timing summary (ms) ====\n";
    for (auto& kv : g_timing.by_category) std::cout << "  " << kv.first << ": " << kv.second << "\n";
}
void MOPS_PrintTimingDetailed() {
    std::cout << "==== MOPS timing detailed (ms) ====\n";
    for (auto& r : g_timing.records) std::cout << "  " << r.first << ": " << r.second << "\n";
}
double MOPS_GetCategoryTime(const char* category) {
    auto it = g_timing.by_category.find(category ? category : "Other");
    return it == g_timing.by_category.end() ? 0.0 : it->second;
}
double MOPS_GetTotalTime() {
    double s = 0.0;
    for (auto& kv : g_timing.by_category) s += kv.second;
    return s;
}

// RemoveNaNTrajectoriesAndReindex (src/Common/TrajectoryCommon.h:57-129): every non-empty line
// packed into one device allocation, cleaned by ONE mops_remove_nan_ragged launch, copied back.
std::vector<TrajectoryLine> RemoveNaNTrajectoriesAndReindex(std::vector<TrajectoryLine>& lines) {
    std::vector<TrajectoryLine*> keep;  // empty lines are dropped (:84-86)
    keep.reserve(lines.size());
    std::vector<int64_t> off(1, 0);
    for (auto& l : lines) {
        const size_t P = l.points.size();
        if (P == 0) continue;
        l.velocity.resize(P, CartesianCoord{0.0, 0.0, 0.0});  // :88-90
        l.temperature.resize(P, 0.0);
        l.salinity.resize(P, 0.0);
        keep.push_back(&l);
        off.push_back(off.back() + (int64_t)P);
    }
    const int64_t m = (int64_t)keep.size(), T = off.back();
    std::vector<TrajectoryLine> out;
    out.reserve((size_t)m);
    if (m == 0) return out;
    std::vector<double> hp((size_t)T * 3), hv((size_t)T * 3), ht((size_t)T), hs((size_t)T), hl((size_t)m * 3);
    for (int64_t i = 0; i < m; ++i) {
        const TrajectoryLine& l = *keep[(size_t)i];
        const size_t P = l.points.size(), b = (size_t)off[(size_t)i];
        std::memcpy(hp.data() + 3 * b, l.points.data(), P * sizeof(CartesianCoord));
        std::memcpy(hv.data() + 3 * b, l.velocity.data(), P * sizeof(CartesianCoord));
        std::memcpy(ht.data() + b, l.temperature.data(), P * sizeof(double));
        std::memcpy(hs.data() + b, l.salinity.data(), P * sizeof(double));
    }
    // one allocation: points | velocity | temperature | salinity | last | offsets
    const size_t bytes = (size_t)T * 64 + (size_t)m * 24 + (size_t)(m + 1) * 8;
    struct DevBuf {
        void* p = nullptr;
        ~DevBuf() { (void)hipFree(p); }
    } buf;
    auto hip = [](hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    };
    hip(hipMalloc(&buf.p, bytes), "RemoveNaNTrajectoriesAndReindex: hipMalloc");
    double* dp = static_cast<double*>(buf.p);
    double* dv = dp + 3 * T;
    double* dt = dv + 3 * T;
    double* ds = dt + T;
    double* dl = ds + T;
    int64_t* doff = reinterpret_cast<int64_t*>(dl + 3 * m);
    const hipMemcpyKind h2d = hipMemcpyHostToDevice, d2h = hipMemcpyDeviceToHost;
    hip(hipMemcpy(dp, hp.data(), (size_t)T * 24, h2d), "hipMemcpy points");
    hip(hipMemcpy(dv, hv.data(), (size_t)T * 24, h2d), "hipMemcpy velocity");
    hip(hipMemcpy(dt, ht.data(), (size_t)T * 8, h2d), "hipMemcpy temperature");
    hip(hipMemcpy(ds, hs.data(), (size_t)T * 8, h2d), "hipMemcpy salinity");
    hip(hipMemcpy(doff, off.data(), (size_t)(m + 1) * 8, h2d), "hipMemcpy offsets");
    check(mops_remove_nan_ragged(m, doff, dp, dv, dt, ds, dl, nullptr), "mops_remove_nan_ragged");
    hip(hipMemcpy(hp.data(), dp, (size_t)T * 24, d2h), "hipMemcpy points");
    hip(hipMemcpy(hv.data(), dv, (size_t)T * 24, d2h), "hipMemcpy velocity");
    hip(hipMemcpy(ht.data(), dt, (size_t)T * 8, d2h), "hipMemcpy temperature");
    hip(hipMemcpy(hs.data(), ds, (size_t)T * 8, d2h), "hipMemcpy salinity");
    hip(hipMemcpy(hl.data(), dl, (size_t)m * 24, d2h), "hipMemcpy lastPoint");
    for (int64_t i = 0; i < m; ++i) {
        TrajectoryLine& l = *keep[(size_t)i];
        const size_t P = l.points.size(), b = (size_t)off[(size_t)i];
        std::memcpy(l.points.data(), hp.data() + 3 * b, P * sizeof(CartesianCoord));
        std::memcpy(l.velocity.data(), hv.data() + 3 * b, P * sizeof(CartesianCoord));
        std::memcpy(l.temperature.data(), ht.data() + b, P * sizeof(double));
        std::memcpy(l.salinity.data(), hs.data() + b, P * sizeof(double));
        l.lastPoint = {hl[(size_t)(3 * i)], hl[(size_t)(3 * i + 1)], hl[(size_t)(3 * i + 2)]};  // :123
        l.lineID = (int)i;  // :124
        out.push_back(l);
    }
    return out;
}

}  // namespace MOPS
