// remap_api.cpp -- MOPS::MOPS_RunRemapping through the C++ API (include/mops/MOPS.h), the way the
// reference's CLI drives it (CLI/main.cpp:133-149).  Reads a case written by tests/test_remap_cpp.py as
// raw little-endian arrays and writes the images back.
//
//   remap_api <case_dir>
//
// case_dir/dims.txt : C V maxE L n_attr width height minLat maxLat minLon maxLon depth
// inputs            : nEdgesOnCell verticesOnCell cellsOnCell cellsOnVertex (u64), cellCoord vertexCoord
//                     (f64 xyz), layerThickness bottomDepth zonal meridional vvel (f64),
//                     attr_0 .. attr_{n_attr-1} (f64 [C*L], named a0, a1, ... in that order)
// outputs           : images_reference.f64, images_bracket.f64 ([n_images][height][width][4]),
//                     summary.txt: n_images width height pixel(0,0).x channel-3 sum of image 0
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
        std::cerr << "usage: remap_api <case_dir>\n";
        return 2;
    }
    const std::string dir = argv[1];
    size_t C, V, maxE, L, n_attr;
    int width, height;
    double minLat, maxLat, minLon, maxLon, depth;
    {
        std::ifstream f(dir + "/dims.txt");
        if (!(f >> C >> V >> maxE >> L >> n_attr >> width >> height >> minLat >> maxLat >> minLon >> maxLon >> depth)) {
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
    for (size_t k = 0; k < n_attr; ++k)
        sol->mDoubleAttributes["a" + std::to_string(k)] = load<double>(dir + "/attr_" + std::to_string(k), C * L);
    MOPS_AddAttribute(0, sol);
    MOPS_End();
    MOPS_ActiveAttribute(0);

    VisualizationSettings cfg;
    cfg.imageSize = {(double)width, (double)height};
    cfg.LatRange = {minLat, maxLat};
    cfg.LonRange = {minLon, maxLon};
    cfg.FixedDepth = depth;
    cfg.VisType = VisualizeType::kFixedDepth;
    size_t n_images = 0;
    double first_x = 0.0, alpha_sum = 0.0;
    for (int rule = 0; rule < 2; ++rule) {
        cfg.layerRule = rule == 0 ? LayerRule::kReference : LayerRule::kBracket;
        std::vector<ImageBuffer<double>> img_vec = MOPS_RunRemapping(&cfg);
        std::ofstream f(dir + (rule == 0 ? "/images_reference.f64" : "/images_bracket.f64"), std::ios::binary);
        for (const auto& img : img_vec) {
            if (img.getWidth() != width || img.getHeight() != height || img.mPixels.size() != (size_t)width * height * 4) {
                std::cerr << "bad image shape\n";
                return 3;
            }
            f.write(reinterpret_cast<const char*>(img.mPixels.data()), (std::streamsize)(img.mPixels.size() * 8));
        }
        if (rule == 0 && !img_vec.empty()) {
            n_images = img_vec.size();
            first_x = img_vec[0].getPixel(0, 0).x;
            for (double a : img_vec[0].getChannel(3)) alpha_sum += a;
        }
    }
    std::ofstream s(dir + "/summary.txt");
    s << n_images << " " << width << " " << height << " " << (first_x != first_x ? "nan" : std::to_string(first_x)) << " "
      << alpha_sum << "\n";
    MOPS_Finalize();
    return 0;
}
