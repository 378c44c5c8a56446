// image_api.cpp -- MOPS::SaveToPNG, both MOPS::VTKFileManager::SaveVTI overloads and
// MOPS::MPASOVisualizer::VisualizeFixedLayer through the C++ API (include/mops/MOPS.h), on a
// MOPS_RunRemapping result, the way the reference's CLI drives them (CLI/main.cpp:133-187).  Reads a case
// written by tests/test_image_cpp.py in remap_api.cpp's layout and writes files into the case directory.
//
//   image_api <case_dir>
//
// case_dir/dims.txt : C V maxE L n_attr width height minLat maxLat minLon maxLon depth layer
// inputs            : as remap_api.cpp
// outputs           : cpp_<i>_ch<c>.png (image i, channel c < 3), cpp_alpha.png (image 0, the default channel),
//                     cpp_fixed_depth_<depth>.vti (the image list, two names given),
//                     cpp1_fixed_depth_<depth>.vti (image 0 alone), fixed_layer.f64 ([height][width][4]),
//                     cpp_fixed_layer_<layer>.vti (that image alone), summary.txt: n_images bad_channel_result
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
        std::cerr << "usage: image_api <case_dir>\n";
        return 2;
    }
    const std::string dir = argv[1];
    size_t C, V, maxE, L, n_attr;
    int width, height;
    double minLat, maxLat, minLon, maxLon, depth, layer;
    {
        std::ifstream f(dir + "/dims.txt");
        if (!(f >> C >> V >> maxE >> L >> n_attr >> width >> height >> minLat >> maxLat >> minLon >> maxLon >> depth >>
              layer)) {
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
    cfg.saveType = SaveType::kPNG;
    std::vector<ImageBuffer<double>> img_vec = MOPS_RunRemapping(&cfg);
    if (img_vec.empty()) return 3;
    for (size_t i = 0; i < img_vec.size(); ++i)
        for (int ch = 0; ch < 3; ++ch)  // CLI/main.cpp:169-182
            if (!SaveToPNG(img_vec[i], dir + "/cpp_" + std::to_string(i) + "_ch" + std::to_string(ch) + ".png", ch))
                return 4;
    if (!SaveToPNG(img_vec[0], dir + "/cpp_alpha.png")) return 4;
    const bool bad = SaveToPNG(img_vec[0], dir + "/cpp_bad.png", 4);
    VTKFileManager::SaveVTI(img_vec, &cfg, {"E: Zonal Velocity", "N: Meridional Velocity"}, dir + "/cpp");
    VTKFileManager::SaveVTI(&img_vec[0], &cfg, dir + "/cpp1");

    cfg.VisType = VisualizeType::kFixedLayer;
    cfg.FixedLayer = layer;
    ImageBuffer<double> layer_img(width, height);
    MPASOVisualizer::VisualizeFixedLayer(&cfg, &layer_img);
    {
        std::ofstream f(dir + "/fixed_layer.f64", std::ios::binary);
        f.write(reinterpret_cast<const char*>(layer_img.mPixels.data()), (std::streamsize)(layer_img.mPixels.size() * 8));
    }
    VTKFileManager::SaveVTI(&layer_img, &cfg, dir + "/cpp");
    std::ofstream s(dir + "/summary.txt");
    s << img_vec.size() << " " << (bad ? 1 : 0) << "\n";
    MOPS_Finalize();
    return 0;
}
