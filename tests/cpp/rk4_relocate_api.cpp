// rk4_relocate_api.cpp -- MOPS::MOPS_RunPathLine with TrajectorySettings::relocateStages through the C++ API
// (include/mops/MOPS.h).  Reads a case written by tests/test_rk4_relocate_cpp.py as raw little-endian arrays and
// writes the lines back.
//
//   rk4_relocate_api <case_dir>
//
// case_dir/dims.txt : C V maxE L n deltaT duration recordT
// inputs            : nEdgesOnCell verticesOnCell cellsOnCell cellsOnVertex (u64), cellCoord vertexCoord (f64 xyz),
//                     per snapshot t = 0, 1: layerThickness_t bottomDepth_t zonal_t meridional_t vvel_t (f64),
//                     seeds (f64 [n][3]), depths (f32 [n])
// outputs           : for tag in rk4_on rk4_off euler_on euler_off (method, relocateStages): points_<tag>.f64
//                     velocity_<tag>.f64 [n][K+1][3], last_<tag>.f64 [n][3]; streamline.txt: the line counts of
//                     MOPS_RunStreamLine with (kEuler, on), (kRK4, off), (kRK4, on) and of MOPS_RunPathLine with
//                     (kRK4, on, sampleAttributes)
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
        std::cerr << "usage: rk4_relocate_api <case_dir>\n";
        return 2;
    }
    const std::string dir = argv[1];
    size_t C, V, maxE, L, n, deltaT, duration, recordT;
    {
        std::ifstream f(dir + "/dims.txt");
        if (!(f >> C >> V >> maxE >> L >> n >> deltaT >> duration >> recordT)) {
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
    if (cfg.relocateStages) {
        std::cerr << "relocateStages must default to false\n";
        return 3;
    }
    for (int run = 0; run < 4; ++run) {
        const bool rk4 = run < 2, on = (run % 2) == 0;
        cfg.methodType = rk4 ? CalcMethodType::kRK4 : CalcMethodType::kEuler;
        cfg.relocateStages = on;
        std::vector<CartesianCoord> pts = as_vec3(seeds);  // (MOPS_RunPathLine moves them to the last points)
        const std::vector<TrajectoryLine> lines = MOPS_RunPathLine(&cfg, pts);
        if (lines.size() != n) {
            std::cerr << "bad line count\n";
            return 3;
        }
        const std::string tag = std::string(rk4 ? "_rk4" : "_euler") + (on ? "_on.f64" : "_off.f64");
        std::ofstream fp(dir + "/points" + tag, std::ios::binary), fv(dir + "/velocity" + tag, std::ios::binary),
            fl(dir + "/last" + tag, std::ios::binary);
        for (const auto& l : lines) {
            fp.write(reinterpret_cast<const char*>(l.points.data()), (std::streamsize)(l.points.size() * 24));
            fv.write(reinterpret_cast<const char*>(l.velocity.data()), (std::streamsize)(l.velocity.size() * 24));
            fl.write(reinterpret_cast<const char*>(&l.lastPoint), 24);
        }
    }
    MOPS_ActiveAttribute(0);
    size_t counts[4];
    const CalcMethodType methods[3] = {CalcMethodType::kEuler, CalcMethodType::kRK4, CalcMethodType::kRK4};
    const bool flags[3] = {true, false, true};
    for (int k = 0; k < 3; ++k) {
        cfg.methodType = methods[k];
        cfg.relocateStages = flags[k];
        std::vector<CartesianCoord> pts = as_vec3(seeds);
        counts[k] = MOPS_RunStreamLine(&cfg, pts).size();
    }
    MOPS_ActiveAttribute(0, 1);
    {
        cfg.methodType = CalcMethodType::kRK4;
        cfg.relocateStages = true;
        cfg.sampleAttributes = true;
        std::vector<CartesianCoord> pts = as_vec3(seeds);
        counts[3] = MOPS_RunPathLine(&cfg, pts).size();
    }
    std::ofstream(dir + "/streamline.txt") << counts[0] << " " << counts[1] << " " << counts[2] << " " << counts[3]
                                           << "\n";
    MOPS_Finalize();
    return 0;
}
