// section_api.cpp -- MOPS::MOPS_RunRemappingSection and MOPS::MOPS_SectionTransport through the C++ API
// (include/mops/MOPS.h).  Reads a case written by tests/test_section_gpu.py in remap_api.cpp's layout and
// writes files into the case directory.
//
//   section_api <case_dir>
//
// case_dir/dims.txt : C V maxE L n_attr width height n_way  lat0 lon0  lat1 lon1 ...
// inputs            : as remap_api.cpp, and refBottomDepth [L] doubles (DepthRange stays (0, 0): the default rows)
// outputs           : section_<i>.f64 ([height][width][4] doubles of image i), section_0_ch<c>.png (c < 3),
//                     section_1_ch0.png (with attributes), summary.txt: n_images, the transport as a hexadecimal
//                     float, the image count of a one-waypoint path, the transport of a one-waypoint path
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
        std::cerr << "usage: section_api <case_dir>\n";
        return 2;
    }
    const std::string dir = argv[1];
    size_t C, V, maxE, L, n_attr, n_way;
    int width, height;
    std::vector<vec2> path;
    {
        std::ifstream f(dir + "/dims.txt");
        if (!(f >> C >> V >> maxE >> L >> n_attr >> width >> height >> n_way)) {
            std::cerr << "bad dims.txt\n";
            return 2;
        }
        for (size_t i = 0; i < n_way; ++i) {
            vec2 p{};
            if (!(f >> p.x >> p.y)) return 2;
            path.push_back(p);
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
    grid->cellRefBottomDepth_vec = load<double>(dir + "/refBottomDepth", L);
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
    for (size_t k = 0; k < n_attr; ++k)
        sol->mDoubleAttributes["a" + std::to_string(k)] = load<double>(dir + "/attr_" + std::to_string(k), C * L);
    MOPS_AddAttribute(0, sol);
    MOPS_End();
    MOPS_ActiveAttribute(0);

    VisualizationSettings cfg;
    cfg.imageSize = {(double)width, (double)height};
    cfg.SectionPath = path;
    std::vector<ImageBuffer<double>> img_vec = MOPS_RunRemappingSection(&cfg);
    if (img_vec.empty()) return 3;
    for (size_t i = 0; i < img_vec.size(); ++i) {
        std::ofstream f(dir + "/section_" + std::to_string(i) + ".f64", std::ios::binary);
        const std::vector<double>& px = img_vec[i].mPixels;
        f.write(reinterpret_cast<const char*>(px.data()), (std::streamsize)(px.size() * 8));
    }
    for (int ch = 0; ch < 3; ++ch)
        if (!SaveToPNG(img_vec[0], dir + "/section_0_ch" + std::to_string(ch) + ".png", ch)) return 4;
    if (img_vec.size() > 1 && !SaveToPNG(img_vec[1], dir + "/section_1_ch0.png", 0)) return 4;
    const double sv = MOPS_SectionTransport(img_vec[0], &cfg);
    cfg.SectionPath.resize(1);
    const size_t n_bad = MOPS_RunRemappingSection(&cfg).size();
    const double sv_bad = MOPS_SectionTransport(img_vec[0], &cfg);
    char buf[256];
    std::snprintf(buf, sizeof buf, "%zu %a %zu %s\n", img_vec.size(), sv, n_bad, sv_bad != sv_bad ? "nan" : "number");
    std::ofstream s(dir + "/summary.txt");
    s << buf;
    MOPS_Finalize();
    return 0;
}
