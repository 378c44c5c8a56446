// census_api.cpp -- MOPS::MOPS_RunEddyCensus through the C++ API (include/mops/MOPS.h).  Reads a case written by
// tests/test_census_cpp.py in remap_api.cpp's layout and writes files into the case directory.
//
//   census_api <case_dir>
//
// case_dir/dims.txt : C V maxE L width height minLat maxLat minLon maxLon layer kSigma minCells
// inputs            : as remap_api.cpp, without attributes
// outputs           : census_image.f64 ([height][width][4] doubles), census_labels.i32 ([C]), census_table.f64
//                     (per eddy: lat lon radius area circulation ow_min and the centre's x y z),
//                     census_table.i32 (per eddy: index polarity n_cells root core_cell), threshold.f64,
//                     summary.txt: the eddy counts of a good call, of one with a zero width, with EddyMinCells 0,
//                     with a NaN EddyThreshold and with a null config
#include <cmath>
#include <cstdint>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "mops/MOPS.h"

template <class T>
static std::vector<T> load(const std::string& path, size_t n) {
    std::vector<T> v(n);
    std::ifstream f(path, std::ios::binary);
    if (!f || !f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)))) {
        std::cerr << "cannot read " << path << "\n";
        std::exit(2);
    }
    return v;
}

template <class T>
static bool dump(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return (bool)f;
}

int main(int argc, char** argv) {
    using namespace MOPS;
    if (argc < 2) {
        std::cerr << "usage: census_api <case_dir>\n";
        return 2;
    }
    const std::string dir = argv[1];
    size_t C, V, maxE, L;
    int width, height, minCells;
    double minLat, maxLat, minLon, maxLon, layer, kSigma;
    {
        std::ifstream f(dir + "/dims.txt");
        if (!(f >> C >> V >> maxE >> L >> width >> height >> minLat >> maxLat >> minLon >> maxLon >> layer >> kSigma >>
              minCells)) {
            std::cerr << "bad dims.txt\n";
            return 2;
        }
    }
    auto as_vec3 = [](const std::vector<double>& a) {
        std::vector<vec3> v(a.size() / 3);
        for (size_t i = 0; i < v.size(); ++i) v[i] = {a[3 * i], a[3 * i + 1], a[3 * i + 2]};
        return v;
    };
    MOPS_Init("gpu");
    MOPS_Begin();
    auto grid = std::make_shared<MPASOGrid>();
    grid->setGridAttribute(GridAttributeType::kCellSize, (int)C);
    grid->setGridAttribute(GridAttributeType::kVertexSize, (int)V);
    grid->setGridAttribute(GridAttributeType::kMaxEdgesSize, (int)maxE);
    grid->setGridAttributesVec3(GridAttributeType::kCellCoord, as_vec3(load<double>(dir + "/cellCoord", C * 3)));
    grid->setGridAttributesVec3(GridAttributeType::kVertexCoord, as_vec3(load<double>(dir + "/vertexCoord", V * 3)));
    grid->setGridAttributesInt(GridAttributeType::kNumberVertexOnCell, load<size_t>(dir + "/nEdgesOnCell", C));
    grid->setGridAttributesInt(GridAttributeType::kVerticesOnCell, load<size_t>(dir + "/verticesOnCell", C * maxE));
    grid->setGridAttributesInt(GridAttributeType::kCellsOnCell, load<size_t>(dir + "/cellsOnCell", C * maxE));
    grid->setGridAttributesInt(GridAttributeType::kCellsOnVertex, load<size_t>(dir + "/cellsOnVertex", V * 3));
    MOPS_AddGridMesh(grid);
    auto sol = std::make_shared<MPASOSolution>();
    sol->setTimestep(0);
    sol->setAttribute(GridAttributeType::kVertLevels, (int)L);
    sol->setAttribute(GridAttributeType::kVertLevelsP1, (int)L + 1);
    sol->setAttributesDouble(AttributeType::kLayerThickness, load<double>(dir + "/layerThickness", C * L));
    sol->setAttributesDouble(AttributeType::kBottomDepth, load<double>(dir + "/bottomDepth", C));
    sol->setAttributesDouble(AttributeType::kZonalVelocity, load<double>(dir + "/zonal", C * L));
    sol->setAttributesDouble(AttributeType::kMeridionalVelocity, load<double>(dir + "/meridional", C * L));
    sol->cellVertVelocity_vec = load<double>(dir + "/vvel", C * (L + 1));
    MOPS_AddAttribute(0, sol);
    MOPS_End();
    MOPS_ActiveAttribute(0);

    VisualizationSettings cfg;
    if (cfg.EddyThreshold != 0.2 || cfg.EddyMinCells != 4) {
        std::cerr << "bad defaults\n";
        return 3;
    }
    cfg.imageSize = {(double)width, (double)height};
    cfg.LatRange = {minLat, maxLat};
    cfg.LonRange = {minLon, maxLon};
    cfg.FixedLayer = layer;
    cfg.EddyThreshold = kSigma;
    cfg.EddyMinCells = minCells;
    const EddyCensus cen = MOPS_RunEddyCensus(&cfg);
    if (cen.labels.size() != C || cen.image.getWidth() != width || cen.image.getHeight() != height ||
        cen.image.mPixels.size() != (size_t)width * height * 4) {
        std::cerr << "bad census\n";
        return 3;
    }
    std::vector<double> td;
    std::vector<int32_t> ti;
    for (const Eddy& e : cen.eddies) {
        for (double x : {e.lat, e.lon, e.radius, e.area, e.circulation, e.ow_min, e.centre.x, e.centre.y, e.centre.z})
            td.push_back(x);
        for (int x : {e.index, e.polarity, e.n_cells, e.root, e.core_cell}) ti.push_back(x);
    }
    if (!dump(dir + "/census_image.f64", cen.image.mPixels) ||
        !dump(dir + "/census_labels.i32", std::vector<int32_t>(cen.labels.begin(), cen.labels.end())) ||
        !dump(dir + "/census_table.f64", td) || !dump(dir + "/census_table.i32", ti) ||
        !dump(dir + "/threshold.f64", std::vector<double>{cen.threshold}))
        return 4;
    auto refused = [&](VisualizationSettings* c) {
        const EddyCensus r = MOPS_RunEddyCensus(c);
        return r.eddies.empty() && r.labels.empty() && r.image.mPixels.empty();
    };
    VisualizationSettings bad = cfg;
    bad.imageSize = {0.0, (double)height};
    const bool r_size = refused(&bad);
    bad = cfg;
    bad.EddyMinCells = 0;
    const bool r_min = refused(&bad);
    bad = cfg;
    bad.EddyThreshold = std::nan("");
    const bool r_nan = refused(&bad);
    const bool r_null = refused(nullptr);
    std::ofstream s(dir + "/summary.txt");
    s << cen.eddies.size() << " " << r_size << " " << r_min << " " << r_nan << " " << r_null << "\n";
    MOPS_Finalize();
    return 0;
}
