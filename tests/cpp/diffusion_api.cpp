// diffusion_api.cpp -- MOPS::MOPS_RunStreamLine / MOPS_RunPathLine with TrajectorySettings::diffusivity, randomSeed and
// randomEpoch through the C++ API (include/mops/MOPS.h).  Reads a case written by tests/test_diffusion_cpp.py as raw
// little-endian arrays (the layout of tests/cpp/layer_api.cpp) and writes the lines back.
//
//   diffusion_api <case_dir>
//
// case_dir/dims.txt : C V maxE L n deltaT duration recordT layer kh seed epoch
// outputs           : points_<tag>.f64 velocity_<tag>.f64 [n][K+1][3] (pathlines: last_<tag>.f64 [n][3]) for
//                     path_layer (kEuler at the layer), path_depth (kRK4 with relocateStages at the depths),
//                     stream_layer (kRK4 at the layer), path_off (kEuler at the depths, diffusivity 0 with a seed and
//                     an epoch set); errors.txt: the line counts of MOPS_RunPathLine with diffusivity -1 and NaN, of
//                     MOPS_RunStreamLine with a diffusivity and no layer, and of MOPS_RunPathLine with a diffusivity
//                     and sampleAttributes
#include <cmath>
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

int main(int argc, char** argv) {
    using namespace MOPS;
    if (argc < 2) {
        std::cerr << "usage: diffusion_api <case_dir>\n";
        return 2;
    }
    const std::string dir = argv[1];
    size_t C, V, maxE, L, n, deltaT, duration, recordT;
    int layer;
    double kh;
    unsigned long long seed;
    unsigned int epoch;
    {
        std::ifstream f(dir + "/dims.txt");
        if (!(f >> C >> V >> maxE >> L >> n >> deltaT >> duration >> recordT >> layer >> kh >> seed >> epoch)) {
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

    const std::vector<double> seeds = load<double>(dir + "/seeds", n * 3);
    TrajectorySettings cfg;
    cfg.deltaT = deltaT;
    cfg.simulationDuration = duration;
    cfg.recordT = recordT;
    cfg.depth = 0.0f;
    cfg.particle_depths = load<float>(dir + "/depths", n);
    if (cfg.diffusivity != 0.0 || cfg.randomSeed != 0 || cfg.randomEpoch != 0) {
        std::cerr << "diffusivity, randomSeed and randomEpoch must default to 0\n";
        return 3;
    }
    cfg.randomSeed = seed;
    cfg.randomEpoch = epoch;
    auto dump = [&](const std::vector<TrajectoryLine>& lines, const std::string& tag, bool pathline) {
        std::ofstream fp(dir + "/points_" + tag + ".f64", std::ios::binary),
            fv(dir + "/velocity_" + tag + ".f64", std::ios::binary);
        for (const auto& l : lines) {
            fp.write(reinterpret_cast<const char*>(l.points.data()), (std::streamsize)(l.points.size() * 24));
            fv.write(reinterpret_cast<const char*>(l.velocity.data()), (std::streamsize)(l.velocity.size() * 24));
        }
        if (pathline) {
            std::ofstream fl(dir + "/last_" + tag + ".f64", std::ios::binary);
            for (const auto& l : lines) fl.write(reinterpret_cast<const char*>(&l.lastPoint), 24);
        }
    };
    struct Run {
        const char* tag;
        bool pathline;
        CalcMethodType method;
        bool relocate;
        int layer;
        double kh;
    };
    const Run runs[4] = {{"path_layer", true, CalcMethodType::kEuler, false, layer, kh},
                         {"path_depth", true, CalcMethodType::kRK4, true, -1, kh},
                         {"stream_layer", false, CalcMethodType::kRK4, false, layer, kh},
                         {"path_off", true, CalcMethodType::kEuler, false, -1, 0.0}};
    for (const Run& r : runs) {
        if (r.pathline) MOPS_ActiveAttribute(0, 1);
        else MOPS_ActiveAttribute(0);
        cfg.methodType = r.method;
        cfg.relocateStages = r.relocate;
        cfg.fixedLayer = r.layer;
        cfg.diffusivity = r.kh;
        std::vector<CartesianCoord> pts = as_vec3(seeds);  // (MOPS_RunPathLine moves them to the last points)
        const std::vector<TrajectoryLine> lines = r.pathline ? MOPS_RunPathLine(&cfg, pts) : MOPS_RunStreamLine(&cfg, pts);
        if (lines.size() != n) {
            std::cerr << "bad line count\n";
            return 3;
        }
        dump(lines, r.tag, r.pathline);
    }
    // the Error() paths
    size_t counts[4];
    cfg.methodType = CalcMethodType::kEuler;
    cfg.relocateStages = false;
    cfg.fixedLayer = -1;
    MOPS_ActiveAttribute(0, 1);
    for (int k = 0; k < 2; ++k) {
        cfg.diffusivity = k == 0 ? -1.0 : std::nan("");
        std::vector<CartesianCoord> pts = as_vec3(seeds);
        counts[k] = MOPS_RunPathLine(&cfg, pts).size();
    }
    cfg.diffusivity = kh;
    MOPS_ActiveAttribute(0);
    {
        std::vector<CartesianCoord> pts = as_vec3(seeds);
        counts[2] = MOPS_RunStreamLine(&cfg, pts).size();
    }
    MOPS_ActiveAttribute(0, 1);
    {
        cfg.sampleAttributes = true;
        std::vector<CartesianCoord> pts = as_vec3(seeds);
        counts[3] = MOPS_RunPathLine(&cfg, pts).size();
    }
    std::ofstream(dir + "/errors.txt") << counts[0] << " " << counts[1] << " " << counts[2] << " " << counts[3] << "\n";
    MOPS_Finalize();
    return 0;
}
