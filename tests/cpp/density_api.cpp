// Test driver for MOPS::MOPS_RunDensity (include/mops/MOPS.h): reads n lines of P points each (and their
// temperature) from <dir>, bins them with value "" and "temperature", writes the two images as raw doubles and
// the count image's channel 0 as a PNG, and checks the error convention (Error() and an empty image).
//   density_api <dir>      files: dims.txt "n P width height min_lat max_lat min_lon max_lon", points, temperature
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "mops/MOPS.h"

template <typename T>
static std::vector<T> load(const std::string& path, size_t count) {
    std::vector<T> v(count);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    if (!f) { std::fprintf(stderr, "short read: %s\n", path.c_str()); std::exit(2); }
    return v;
}

static void store(const std::string& path, const std::vector<double>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(double)));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string d = std::string(argv[1]) + "/";
    size_t n = 0, P = 0;
    int W = 0, H = 0;
    double lat0 = 0, lat1 = 0, lon0 = 0, lon1 = 0;
    {
        std::ifstream f(d + "dims.txt");
        f >> n >> P >> W >> H >> lat0 >> lat1 >> lon0 >> lon1;
        if (!f) return 2;
    }
    const auto pts = load<double>(d + "points", n * P * 3);
    const auto tmp = load<double>(d + "temperature", n * P);
    std::vector<MOPS::TrajectoryLine> lines(n);
    for (size_t i = 0; i < n; ++i) {
        lines[i].lineID = (int)i;
        for (size_t k = 0; k < P; ++k) {
            const double* p = &pts[(i * P + k) * 3];
            lines[i].points.push_back(CartesianCoord{p[0], p[1], p[2]});
            lines[i].temperature.push_back(tmp[i * P + k]);
        }
    }
    MOPS::VisualizationSettings cfg;
    cfg.imageSize = {(double)W, (double)H};
    cfg.LatRange = {lat0, lat1};
    cfg.LonRange = {lon0, lon1};
    cfg.FixedDepth = 0.0;
    const auto count = MOPS::MOPS_RunDensity(lines, &cfg);
    const auto mean = MOPS::MOPS_RunDensity(lines, &cfg, "temperature");
    if (count.getWidth() != W || count.getHeight() != H || mean.getWidth() != W) return 3;
    store(d + "count.f64", count.mPixels);
    store(d + "temperature.f64", mean.mPixels);
    if (!MOPS::SaveToPNG(count, d + "count.png", 0)) return 4;
    // bad input: Error() and an empty image
    if (MOPS::MOPS_RunDensity(lines, nullptr).getWidth() != 0) return 5;
    if (MOPS::MOPS_RunDensity(lines, &cfg, "density").mPixels.size() != (size_t)W * H * 4) return 6;  // zero image
    MOPS::VisualizationSettings bad = cfg;
    bad.LonRange = {0.0, 400.0};
    if (MOPS::MOPS_RunDensity(lines, &bad).getWidth() != 0) return 7;
    bad = cfg;
    bad.imageSize = {0.0, 4.0};
    if (!MOPS::MOPS_RunDensity(lines, &bad).mPixels.empty()) return 8;
    return 0;
}
