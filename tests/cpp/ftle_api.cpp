// Test driver for MOPS::MOPS_LatticeSeeds / MOPS::MOPS_RunFTLE (include/mops/MOPS.h): writes the lattice of the
// window in <dir>/dims.txt, reads n = width * height first points and last points, builds lines from them, writes
// the FTLE image as raw doubles and its channel 0 as a PNG, and checks the error convention (Error() and an empty
// result).
//   ftle_api <dir>      files: dims.txt "width height min_lat max_lat min_lon max_lon horizon", first, last
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <fstream>
#include <string>
#include <vector>

#include "mops/MOPS.h"

static std::vector<double> load(const std::string& path, size_t count) {
    std::vector<double> v(count);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(double)));
    if (!f) { std::fprintf(stderr, "short read: %s\n", path.c_str()); std::exit(2); }
    return v;
}

static void store(const std::string& path, const double* p, size_t count) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(p), (std::streamsize)(count * sizeof(double)));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = std::string(argv[1]) + "/";
    int W = 0, H = 0;
    double lat0 = 0, lat1 = 0, lon0 = 0, lon1 = 0, horizon = 0;
    {
        std::ifstream f(d + "dims.txt");
        f >> W >> H >> lat0 >> lat1 >> lon0 >> lon1 >> horizon;
        if (!f) return 2;
    }
    const size_t n = (size_t)W * H;
    MOPS::VisualizationSettings cfg;
    cfg.imageSize = {(double)W, (double)H};
    cfg.LatRange = {lat0, lat1};
    cfg.LonRange = {lon0, lon1};
    cfg.FixedDepth = 0.0;
    const auto seeds = MOPS::MOPS_LatticeSeeds(&cfg);
    if (seeds.size() != n) return 3;
    store(d + "seeds.f64", reinterpret_cast<const double*>(seeds.data()), 3 * n);
    const auto first = load(d + "first", 3 * n), last = load(d + "last", 3 * n);
    std::vector<MOPS::TrajectoryLine> lines(n);
    for (size_t i = 0; i < n; ++i) {
        lines[i].lineID = (int)i;
        lines[i].points.push_back(CartesianCoord{first[3 * i], first[3 * i + 1], first[3 * i + 2]});
        lines[i].points.push_back(CartesianCoord{last[3 * i], last[3 * i + 1], last[3 * i + 2]});
        lines[i].lastPoint = CartesianCoord{last[3 * i], last[3 * i + 1], last[3 * i + 2]};
    }
    const auto img = MOPS::MOPS_RunFTLE(lines, &cfg, horizon);
    if (img.getWidth() != W || img.getHeight() != H) return 4;
    store(d + "ftle.f64", img.mPixels.data(), img.mPixels.size());
    if (!MOPS::SaveToPNG(img, d + "ftle.png", 0)) return 5;
    // a line without points is not valid: its pixel is NaN, the image is still made
    auto holed = lines;
    holed[n / 2].points.clear();
    const auto img2 = MOPS::MOPS_RunFTLE(holed, &cfg, horizon);
    if (img2.getWidth() != W || !std::isnan(img2.mPixels[(n / 2) * 4 + 1])) return 6;
    // bad input: Error() and an empty result
    if (!MOPS::MOPS_LatticeSeeds(nullptr).empty()) return 7;
    MOPS::VisualizationSettings bad = cfg;
    bad.imageSize = {0.0, 4.0};
    if (!MOPS::MOPS_LatticeSeeds(&bad).empty()) return 8;
    if (!MOPS::MOPS_RunFTLE(lines, &bad, horizon).mPixels.empty()) return 9;
    if (!MOPS::MOPS_RunFTLE(lines, nullptr, horizon).mPixels.empty()) return 10;
    if (!MOPS::MOPS_RunFTLE(lines, &cfg, 0.0).mPixels.empty()) return 11;
    if (!MOPS::MOPS_RunFTLE(lines, &cfg, std::nan("")).mPixels.empty()) return 12;
    lines.pop_back();
    if (!MOPS::MOPS_RunFTLE(lines, &cfg, horizon).mPixels.empty()) return 13;
    return 0;
}
