// eddy_api.cpp -- MOPS::MOPS_RunEddyMap through the C++ API (include/mops/MOPS.h).  Reads a case written by
// tests/test_eddy_cpp.py in remap_api.cpp's layout and writes files into the case directory.
//
//   eddy_api <case_dir>
//
// case_dir/dims.txt : C V maxE L width height minLat maxLat minLon maxLon depth
// inputs            : as remap_api.cpp, without attributes
// outputs           : eddy_reference.f64, eddy_bracket.f64 ([height][width][4] doubles, one per layer rule),
//                     eddy_again.f64 (the reference rule once more: the cached vertex arrays), eddy_ch<c>.png
//                     (c < 2), summary.txt: the image counts of a good call and of one with a zero width
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
        std::cerr << "usage: eddy_api <case_dir>\n";
        return 2;
    }
    const std::string dir = argv[1];
    size_t C, V, maxE, L;
    int width, height;
    double minLat, maxLat, minLon, maxLon, depth;
    {
        std::ifstream f(dir + "/dims.txt");
        if (!(f >> C >> V >> maxE >> L >> width >> height >> minLat >> maxLat >> minLon >> maxLon >> depth)) {
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
    cfg.imageSize = {(double)width, (double)height};
    cfg.LatRange = {minLat, maxLat};
    cfg.LonRange = {minLon, maxLon};
    cfg.FixedDepth = depth;
    cfg.VisType = VisualizeType::kFixedDepth;
    size_t n_good = 0;
    const char* names[3] = {"/eddy_reference.f64", "/eddy_bracket.f64", "/eddy_again.f64"};
    for (int pass = 0; pass < 3; ++pass) {
        cfg.layerRule = pass == 1 ? LayerRule::kBracket : LayerRule::kReference;
        std::vector<ImageBuffer<double>> img_vec = MOPS_RunEddyMap(&cfg);
        if (img_vec.size() != 1 || img_vec[0].getWidth() != width || img_vec[0].getHeight() != height ||
            img_vec[0].mPixels.size() != (size_t)width * height * 4) {
            std::cerr << "bad image\n";
            return 3;
        }
        n_good = img_vec.size();
        if (!dump(dir + names[pass], img_vec[0])) return 4;
        if (pass == 0)
            for (int ch = 0; ch < 2; ++ch)
                if (!SaveToPNG(img_vec[0], dir + "/eddy_ch" + std::to_string(ch) + ".png", ch)) return 4;
    }
    cfg.imageSize = {0.0, (double)height};
    const size_t n_bad = MOPS_RunEddyMap(&cfg).size();
    const size_t n_null = MOPS_RunEddyMap(nullptr).size();
    std::ofstream s(dir + "/summary.txt");
    s << n_good << " " << n_bad << " " << n_null << "\n";
    MOPS_Finalize();
    return 0;
}
