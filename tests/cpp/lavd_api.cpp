// lavd_api.cpp -- MOPS::MOPS_RunLAVD through the C++ API (include/mops/MOPS.h).  Reads a case written by
// tests/test_lavd_cpp.py as raw little-endian arrays, writes the image back and counts the refusals.
//
//   lavd_api <case_dir>
//
// case_dir/dims.txt : C V maxE L width height minLat maxLat minLon maxLon depth deltaT duration recordT
// inputs            : nEdgesOnCell verticesOnCell cellsOnCell cellsOnVertex (u64), cellCoord vertexCoord (f64 xyz),
//                     per snapshot t = 0, 1: layerThickness_t bottomDepth_t zonal_t meridional_t vvel_t (f64)
// outputs           : lavd.f64, lavd_again.f64 [H][W][4], lavd.png (channel 0), summary.txt: the pixel count of
//                     every refused call, in order
#include <cstdio>
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

static bool dump(const std::string& path, const MOPS::ImageBuffer<double>& img) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(img.mPixels.data()), (std::streamsize)(img.mPixels.size() * 8));
    return (bool)f;
}

int main(int argc, char** argv) {
    using namespace MOPS;
    if (argc < 2) {
        std::cerr << "usage: lavd_api <case_dir>\n";
        return 2;
    }
    const std::string dir = argv[1];
    size_t C, V, maxE, L, deltaT, duration, recordT;
    int width, height;
    double minLat, maxLat, minLon, maxLon, depth;
    {
        std::ifstream f(dir + "/dims.txt");
        if (!(f >> C >> V >> maxE >> L >> width >> height >> minLat >> maxLat >> minLon >> maxLon >> depth >> deltaT >>
              duration >> recordT)) {
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
    for (int t = 0; t < 2; ++t) {
        const std::string s = "_" + std::to_string(t);
        auto sol = std::make_shared<MPASOSolution>();
        sol->setTimestep(t);
        sol->setAttribute(GridAttributeType::kVertLevels, (int)L);
        sol->setAttribute(GridAttributeType::kVertLevelsP1, (int)L + 1);
        sol->setAttributesDouble(AttributeType::kLayerThickness, load<double>(dir + "/layerThickness" + s, C * L));
        sol->setAttributesDouble(AttributeType::kBottomDepth, load<double>(dir + "/bottomDepth" + s, C));
        sol->setAttributesDouble(AttributeType::kZonalVelocity, load<double>(dir + "/zonal" + s, C * L));
        sol->setAttributesDouble(AttributeType::kMeridionalVelocity, load<double>(dir + "/meridional" + s, C * L));
        sol->cellVertVelocity_vec = load<double>(dir + "/vvel" + s, C * (L + 1));
        MOPS_AddAttribute(t, sol);
    }
    MOPS_End();
    MOPS_ActiveAttribute(0, 1);

    VisualizationSettings cfg;
    cfg.imageSize = {(double)width, (double)height};
    cfg.LatRange = {minLat, maxLat};
    cfg.LonRange = {minLon, maxLon};
    cfg.FixedDepth = depth;
    TrajectorySettings traj;
    traj.deltaT = deltaT;
    traj.simulationDuration = duration;
    traj.recordT = recordT;
    traj.methodType = CalcMethodType::kEuler;
    for (const char* name : {"/lavd.f64", "/lavd_again.f64"}) {  // the second call reuses the kept vertex arrays
        const ImageBuffer<double> img = MOPS_RunLAVD(&cfg, &traj);
        if (img.getWidth() != width || img.getHeight() != height || img.mPixels.size() != (size_t)width * height * 4) {
            std::cerr << "bad image\n";
            return 3;
        }
        if (!dump(dir + name, img)) return 4;
        if (std::string(name) == "/lavd.f64" && !SaveToPNG(img, dir + "/lavd.png", 0)) return 4;
    }
    std::ofstream s(dir + "/summary.txt");
    s << MOPS_RunLAVD(nullptr, &traj).mPixels.size() << " " << MOPS_RunLAVD(&cfg, nullptr).mPixels.size();
    traj.fixedLayer = 0;
    s << " " << MOPS_RunLAVD(&cfg, &traj).mPixels.size();
    traj.fixedLayer = -1;
    traj.relocateStages = true;
    s << " " << MOPS_RunLAVD(&cfg, &traj).mPixels.size();
    traj.relocateStages = false;
    traj.diffusivity = 5.0;
    s << " " << MOPS_RunLAVD(&cfg, &traj).mPixels.size();
    traj.diffusivity = 0.0;
    traj.recordT = 0;
    s << " " << MOPS_RunLAVD(&cfg, &traj).mPixels.size();
    traj.recordT = recordT;
    cfg.imageSize = {0.0, (double)height};
    s << " " << MOPS_RunLAVD(&cfg, &traj).mPixels.size();
    cfg.imageSize = {(double)width, (double)height};
    MOPS_ActiveAttribute(0);  // no back solution
    s << " " << MOPS_RunLAVD(&cfg, &traj).mPixels.size() << "\n";
    MOPS_Finalize();
    return 0;
}
