// Stand-alone driver of the compiled reference CPU kernels (test infrastructure only).
//
//   mops_ref_driver <case file> <result file> <scratch directory>
//
// The case file (tests/ref_case.py writes it) holds a mesh, one or two snapshots and a list of operations;
// the driver fills the reference's MPASOGrid / MPASOSolution objects through their public members, runs the
// reference's own solution initialisation and kernels, and writes every output array to the result file.
// Nothing of the reference is restated here: every number in the result comes out of a reference function.
//
// Both files are little-endian containers of named arrays:
//   "MOPSREF1", u32 count, then per array: u32 name length, name, u32 dtype (0 f64, 1 i64, 2 f32, 3 i32),
//   u32 ndim, u64 dims[ndim], raw data.
#include "CPU/TBB/Kernel/MPASOVisualizerKernels.h"
#include "CPU/TBB/Kernel/TBBKernel.h"
#include "Common/TrajectoryCommon.h"
#include "Core/MPASOField.h"
#include "Core/MPASOGrid.h"
#include "Core/MPASOSolution.h"
#include "Core/MPASOVisualizer.h"
#include "Core/RuntimeContext.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

using namespace MOPS;
namespace K = MOPS::CPU::TBBBackend::Kernel;

namespace {

enum DType : uint32_t { F64 = 0, I64 = 1, F32 = 2, I32 = 3 };
const size_t kItem[] = {8, 8, 4, 4};

struct Array {
    uint32_t dtype = F64;
    std::vector<uint64_t> dims;
    std::vector<char> bytes;
    size_t count() const { size_t n = 1; for (auto d : dims) n *= d; return n; }
};

using Bag = std::map<std::string, Array>;

[[noreturn]] void die(const std::string& msg)
{
    std::fprintf(stderr, "mops_ref_driver: %s\n", msg.c_str());
    std::exit(2);
}

Bag read_bag(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) die(std::string("cannot open ") + path);
    auto get = [&](void* p, size_t n) { if (n && std::fread(p, 1, n, f) != n) die("short case file"); };
    char magic[8];
    get(magic, 8);
    if (std::memcmp(magic, "MOPSREF1", 8) != 0) die("bad magic");
    uint32_t count = 0;
    get(&count, 4);
    Bag bag;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t len = 0, ndim = 0;
        get(&len, 4);
        std::string name(len, '\0');
        get(name.data(), len);
        Array a;
        get(&a.dtype, 4);
        if (a.dtype > I32) die("bad dtype in " + name);
        get(&ndim, 4);
        a.dims.resize(ndim);
        get(a.dims.data(), 8 * ndim);
        a.bytes.resize(a.count() * kItem[a.dtype]);
        get(a.bytes.data(), a.bytes.size());
        bag[name] = std::move(a);
    }
    std::fclose(f);
    return bag;
}

void write_bag(const char* path, const Bag& bag)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) die(std::string("cannot write ") + path);
    auto put = [&](const void* p, size_t n) { if (n && std::fwrite(p, 1, n, f) != n) die("short write"); };
    put("MOPSREF1", 8);
    uint32_t count = static_cast<uint32_t>(bag.size());
    put(&count, 4);
    for (const auto& [name, a] : bag) {
        uint32_t len = static_cast<uint32_t>(name.size()), ndim = static_cast<uint32_t>(a.dims.size());
        put(&len, 4);
        put(name.data(), len);
        put(&a.dtype, 4);
        put(&ndim, 4);
        put(a.dims.data(), 8 * ndim);
        put(a.bytes.data(), a.bytes.size());
    }
    if (std::fclose(f) != 0) die("close failed");
}

const Array& need(const Bag& bag, const std::string& name, uint32_t dtype)
{
    auto it = bag.find(name);
    if (it == bag.end()) die("case lacks " + name);
    if (it->second.dtype != dtype) die("wrong dtype for " + name);
    return it->second;
}

bool has(const Bag& bag, const std::string& name) { return bag.find(name) != bag.end(); }

template <typename T>
const T* data(const Array& a) { return reinterpret_cast<const T*>(a.bytes.data()); }

std::vector<double> f64(const Bag& bag, const std::string& name)
{
    const Array& a = need(bag, name, F64);
    return std::vector<double>(data<double>(a), data<double>(a) + a.count());
}

std::vector<size_t> idx(const Bag& bag, const std::string& name)
{
    const Array& a = need(bag, name, I64);
    std::vector<size_t> v(a.count());
    for (size_t i = 0; i < v.size(); ++i) v[i] = static_cast<size_t>(data<int64_t>(a)[i]);
    return v;
}

std::vector<vec3> v3(const Bag& bag, const std::string& name)
{
    const Array& a = need(bag, name, F64);
    if (a.count() % 3) die(name + " is no [n, 3] array");
    std::vector<vec3> v(a.count() / 3);
    for (size_t i = 0; i < v.size(); ++i) v[i] = vec3(data<double>(a)[3 * i], data<double>(a)[3 * i + 1], data<double>(a)[3 * i + 2]);
    return v;
}

int64_t i64_at(const Bag& bag, const std::string& name, size_t k)
{
    const Array& a = need(bag, name, I64);
    if (k >= a.count()) die(name + " too short");
    return data<int64_t>(a)[k];
}

double f64_at(const Bag& bag, const std::string& name, size_t k)
{
    const Array& a = need(bag, name, F64);
    if (k >= a.count()) die(name + " too short");
    return data<double>(a)[k];
}

template <typename T>
Array make(uint32_t dtype, std::vector<uint64_t> dims, const T* src)
{
    Array a;
    a.dtype = dtype;
    a.dims = std::move(dims);
    a.bytes.resize(a.count() * kItem[dtype]);
    if (!a.bytes.empty()) std::memcpy(a.bytes.data(), src, a.bytes.size());
    return a;
}

Array from_f64(const std::vector<double>& v, std::vector<uint64_t> dims) { return make(F64, std::move(dims), v.data()); }

Array from_v3(const std::vector<vec3>& v)
{
    std::vector<double> flat(v.size() * 3);
    for (size_t i = 0; i < v.size(); ++i) { flat[3 * i] = v[i].x(); flat[3 * i + 1] = v[i].y(); flat[3 * i + 2] = v[i].z(); }
    return make(F64, {v.size(), 3}, flat.data());
}

Array from_int(const std::vector<int>& v, std::vector<uint64_t> dims)
{
    std::vector<int64_t> wide{v.begin(), v.end()};
    return make(I64, std::move(dims), wide.data());
}

// ---- the reference's objects ----------------------------------------------------------------------------
std::shared_ptr<MPASOGrid> build_grid(const Bag& in, const std::string& scratch)
{
    auto g = std::make_shared<MPASOGrid>();
    g->cellCoord_vec = v3(in, "mesh/cellCoord");
    g->vertexCoord_vec = v3(in, "mesh/vertexCoord");
    g->numberVertexOnCell_vec = idx(in, "mesh/nEdgesOnCell");
    g->verticesOnCell_vec = idx(in, "mesh/verticesOnCell");
    g->cellsOnCell_vec = idx(in, "mesh/cellsOnCell");
    g->cellsOnVertex_vec = idx(in, "mesh/cellsOnVertex");
    g->cellRefBottomDepth_vec = f64(in, "mesh/refBottomDepth");
    if (has(in, "mesh/edgesOnCell")) {
        g->edgesOnCell_vec = idx(in, "mesh/edgesOnCell");
        g->cellsOnEdge_vec = idx(in, "mesh/cellsOnEdge");
        g->edgeCoord_vec = v3(in, "mesh/edgeCoord");
    }
    g->mCellsSize = static_cast<int>(g->cellCoord_vec.size());
    g->mVertexSize = static_cast<int>(g->vertexCoord_vec.size());
    g->mEdgesSize = static_cast<int>(g->edgeCoord_vec.size());
    g->mMaxEdgesSize = static_cast<int>(i64_at(in, "mesh/sizes", 0));
    g->mVertLevels = static_cast<int>(i64_at(in, "mesh/sizes", 1));
    g->mVertLevelsP1 = g->mVertLevels + 1;
    g->mCachedDataDir = scratch;
    g->mMeshName = "case";
    sycl::queue q;
    g->createKDTree((scratch + "/KDTree.bin").c_str(), q);  // as MOPSApp::addGrid
    return g;
}

std::shared_ptr<MPASOSolution> build_solution(const Bag& in, const std::string& p, int timestep, int levels)
{
    auto s = std::make_shared<MPASOSolution>();
    s->mTimesteps = timestep;
    s->mVertLevels = levels;
    s->mVertLevelsP1 = levels + 1;
    s->mTotalZTopLayer = 0;
    s->mTotalZTopLayerP1 = 0;
    s->cellLayerThickness_vec = f64(in, p + "layerThickness");
    s->cellBottomDepth_vec = f64(in, p + "bottomDepth");
    s->cellZonalVelocity_vec = f64(in, p + "zonalVelocity");
    s->cellMeridionalVelocity_vec = f64(in, p + "meridionalVelocity");
    s->cellVertVelocity_vec = f64(in, p + "vertVelocityTop");
    const std::string ap = p + "attr/";
    for (const auto& [name, a] : in) {
        if (name.compare(0, ap.size(), ap) == 0) s->mDoubleAttributes[name.substr(ap.size())] = f64(in, name);
    }
    return s;
}

// The calls of MOPSApp::addSol, in its order, each through the reference's own MPASOSolution member (which
// dispatches to the TBBBackend::Calc* functions); their cache files go to the scratch directory.
void init_solution(MPASOGrid* grid, MPASOSolution* sol, std::string& dir, const RuntimeContext& ctx)
{
    sol->mCellsSize = grid->mCellsSize;
    sol->mEdgesSize = grid->mEdgesSize;
    sol->mMaxEdgesSize = grid->mMaxEdgesSize;
    sol->mVertexSize = grid->mVertexSize;
    grid->mVertLevels = sol->mVertLevels;
    grid->mVertLevelsP1 = sol->mVertLevelsP1;
    sol->calcCellCenterZtop();
    sol->calcCellVertexZtop(grid, dir, ctx);
    sol->calcCellCenterVelocityByZM(grid, dir, ctx);
    sol->calcCellVertexVelocity(grid, dir, ctx);
    sol->calcCellVertexVertVelocity(grid, dir, ctx);
    for (const auto& [name, vec] : sol->mDoubleAttributes) sol->calcCellCenterToVertex(name, vec, grid, dir, ctx);
}

void put_solution(Bag& out, const std::string& p, const MPASOGrid& g, const MPASOSolution& s)
{
    const uint64_t C = g.mCellsSize, V = g.mVertexSize, L = s.mVertLevels;
    out[p + "cell_ztop"] = from_f64(s.cellZTop_vec, {C, L});
    out[p + "cell_vel"] = from_v3(s.cellCenterVelocity_vec);
    out[p + "vertex_ztop"] = from_f64(s.cellVertexZTop_vec, {V, L});
    out[p + "vertex_vel"] = from_v3(s.cellVertexVelocity_vec);
    out[p + "vertex_w"] = from_f64(s.cellVertexVertVelocity_vec, {V, L + 1});
    for (const auto& [name, vec] : s.mDoubleAttributes_CtoV) out[p + "vertex_attr/" + name] = from_f64(vec, {V, L});
}

void put_lines(Bag& out, const std::string& p, const std::vector<TrajectoryLine>& lines)
{
    std::vector<int64_t> counts, ids;
    std::vector<vec3> points, velocity, last;
    std::vector<double> temperature, salinity, depth, duration, timestamp;
    for (const auto& l : lines) {
        counts.insert(counts.end(), {static_cast<int64_t>(l.points.size()), static_cast<int64_t>(l.velocity.size()),
                                     static_cast<int64_t>(l.temperature.size()), static_cast<int64_t>(l.salinity.size())});
        ids.push_back(l.lineID);
        points.insert(points.end(), l.points.begin(), l.points.end());
        velocity.insert(velocity.end(), l.velocity.begin(), l.velocity.end());
        temperature.insert(temperature.end(), l.temperature.begin(), l.temperature.end());
        salinity.insert(salinity.end(), l.salinity.begin(), l.salinity.end());
        last.push_back(l.lastPoint);
        depth.push_back(l.depth);
        duration.push_back(l.duration);
        timestamp.push_back(l.timestamp);
    }
    out[p + "counts"] = make(I64, {lines.size(), 4}, counts.data());
    out[p + "lineID"] = make(I64, {lines.size()}, ids.data());
    out[p + "points"] = from_v3(points);
    out[p + "velocity"] = from_v3(velocity);
    out[p + "temperature"] = from_f64(temperature, {temperature.size()});
    out[p + "salinity"] = from_f64(salinity, {salinity.size()});
    out[p + "lastPoint"] = from_v3(last);
    out[p + "depth"] = from_f64(depth, {depth.size()});
    out[p + "duration"] = from_f64(duration, {duration.size()});
    out[p + "timestamp"] = from_f64(timestamp, {timestamp.size()});
}

void put_image(Bag& out, const std::string& name, const std::vector<ImageBuffer<double>>& imgs)
{
    const uint64_t h = imgs[0].getHeight(), w = imgs[0].getWidth();
    std::vector<double> px;
    for (const auto& im : imgs) px.insert(px.end(), im.mPixels.begin(), im.mPixels.end());
    out[name] = from_f64(px, {imgs.size(), h, w, 4});
}

void window(const Bag& in, const std::string& p, VisualizationSettings& cfg)
{
    cfg.imageSize = vec2(static_cast<double>(i64_at(in, p + "size", 0)), static_cast<double>(i64_at(in, p + "size", 1)));
    cfg.LatRange = vec2(f64_at(in, p + "window", 0), f64_at(in, p + "window", 1));
    cfg.LonRange = vec2(f64_at(in, p + "window", 2), f64_at(in, p + "window", 3));
}

void pixel_cells(Bag& out, const std::string& name, MPASOGrid* grid, const VisualizationSettings& cfg)
{
    const int w = static_cast<int>(cfg.imageSize.x()), h = static_cast<int>(cfg.imageSize.y());
    std::vector<int> cells(static_cast<size_t>(w) * h, -1);
    TBBKernel::SearchKDTree(cells.data(), grid, w, h, cfg.LatRange.x(), cfg.LatRange.y(), cfg.LonRange.x(), cfg.LonRange.y());
    out[name] = from_int(cells, {static_cast<uint64_t>(h), static_cast<uint64_t>(w)});
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 4) die("usage: mops_ref_driver <case> <result> <scratch dir>");
    const Bag in = read_bag(argv[1]);
    std::string scratch = argv[3];
    Bag out;

    CPUContext cpu;
    cpu.backend = CPUBackend::kTBB;
    const RuntimeContext ctx = RuntimeContext::FromCPU(cpu);

    const int64_t n_ops = i64_at(in, "n_ops", 0);
    std::shared_ptr<MPASOGrid> grid;
    std::shared_ptr<MPASOSolution> s0, s1;
    if (has(in, "mesh/cellCoord")) {
        grid = build_grid(in, scratch);
        const int levels = grid->mVertLevels;
        s0 = build_solution(in, "s0/", 0, levels);
        init_solution(grid.get(), s0.get(), scratch, ctx);
        if (has(in, "s1/layerThickness")) {
            s1 = build_solution(in, "s1/", 1, levels);
            init_solution(grid.get(), s1.get(), scratch, ctx);
        }
    }

    for (int64_t k = 0; k < n_ops; ++k) {
        const std::string p = "op" + std::to_string(k) + "/";
        const int64_t op = i64_at(in, p + "op", 0);
        MPASOField field;
        if (grid) field.initField(grid, s0, op == 3 ? s1 : nullptr);

        if (op == 0) {  // preprocess
            put_solution(out, p + "s0/", *grid, *s0);
            if (s1) put_solution(out, p + "s1/", *grid, *s1);
        } else if (op == 1) {  // locate
            std::vector<CartesianCoord> pts = v3(in, p + "points");
            std::vector<int> cells;
            field.calcInWhichCells(pts, cells);
            out[p + "cells"] = from_int(cells, {cells.size()});
        } else if (op == 2 || op == 3) {  // streamline / pathline, as MOPSApp::runStreamLine / runPathLine
            if (op == 3 && !s1) die("pathline needs two snapshots");
            std::vector<CartesianCoord> pts = v3(in, p + "seeds");
            TrajectorySettings cfg;
            cfg.deltaT = static_cast<size_t>(i64_at(in, p + "settings", 0));
            cfg.simulationDuration = static_cast<size_t>(i64_at(in, p + "settings", 1));
            cfg.recordT = static_cast<size_t>(i64_at(in, p + "settings", 2));
            cfg.directionType = i64_at(in, p + "settings", 3) ? CalcDirection::kBackward : CalcDirection::kForward;
            cfg.methodType = i64_at(in, p + "settings", 4) ? CalcMethodType::kEuler : CalcMethodType::kRK4;
            const Array& d = need(in, p + "depth", F32);
            cfg.depth = data<float>(d)[0];
            if (has(in, p + "particle_depths")) {
                const Array& pd = need(in, p + "particle_depths", F32);
                cfg.particle_depths.assign(data<float>(pd), data<float>(pd) + pd.count());
            }
            std::vector<int> cells;
            field.calcInWhichCells(pts, cells);
            out[p + "cells"] = from_int(cells, {cells.size()});
            auto lines = (op == 2) ? K::StreamLine(&field, pts, &cfg, cells) : K::PathLine(&field, pts, &cfg, cells);
            put_lines(out, p, lines);
        } else if (op == 4) {  // fixed depth, over MOPSApp::runRemapping's images
            VisualizationSettings cfg;
            window(in, p, cfg);
            cfg.FixedDepth = f64_at(in, p + "value", 0);
            const size_t n_attr = s0->mDoubleAttributes.size();
            std::vector<ImageBuffer<double>> imgs;
            imgs.emplace_back(cfg.imageSize.x(), cfg.imageSize.y());
            if (n_attr > 0) {
                for (size_t i = 0; i < (n_attr + 2) / 3; ++i) imgs.emplace_back(cfg.imageSize.x(), cfg.imageSize.y());
            }
            K::VisualizeFixedDepth(&field, &cfg, imgs);
            put_image(out, p + "images", imgs);
            pixel_cells(out, p + "cells", grid.get(), cfg);
        } else if (op == 5) {  // fixed latitude, as MOPSApp::runReGrid
            VisualizationSettings cfg;
            window(in, p, cfg);
            cfg.FixedLatitude = f64_at(in, p + "value", 0);
            std::vector<ImageBuffer<double>> imgs;
            imgs.emplace_back(cfg.imageSize.x(), cfg.imageSize.y());
            K::VisualizeFixedLatitude(&field, &cfg, &imgs[0]);
            put_image(out, p + "images", imgs);
        } else if (op == 6) {  // fixed layer
            VisualizationSettings cfg;
            window(in, p, cfg);
            cfg.FixedLayer = f64_at(in, p + "value", 0);
            cfg.VisType = VisualizeType::kFixedLayer;
            std::vector<ImageBuffer<double>> imgs;
            imgs.emplace_back(cfg.imageSize.x(), cfg.imageSize.y());
            K::VisualizeFixedLayer(&field, &cfg, &imgs[0]);
            put_image(out, p + "images", imgs);
            pixel_cells(out, p + "cells", grid.get(), cfg);
        } else if (op == 7) {  // RemoveNaNTrajectoriesAndReindex on given lines
            const Array& counts = need(in, p + "counts", I64);
            const size_t n = counts.count() / 4;
            std::vector<CartesianCoord> pts = v3(in, p + "points"), vel = v3(in, p + "velocity");
            std::vector<double> temp = f64(in, p + "temperature"), sal = f64(in, p + "salinity");
            std::vector<TrajectoryLine> lines(n);
            size_t o[4] = {0, 0, 0, 0};
            for (size_t i = 0; i < n; ++i) {
                const int64_t* c = data<int64_t>(counts) + 4 * i;
                lines[i].lineID = static_cast<int>(i64_at(in, p + "lineID", i));
                lines[i].points.assign(pts.begin() + o[0], pts.begin() + o[0] + c[0]);
                lines[i].velocity.assign(vel.begin() + o[1], vel.begin() + o[1] + c[1]);
                lines[i].temperature.assign(temp.begin() + o[2], temp.begin() + o[2] + c[2]);
                lines[i].salinity.assign(sal.begin() + o[3], sal.begin() + o[3] + c[3]);
                lines[i].lastPoint = vec3(0.0, 0.0, 0.0);
                lines[i].duration = lines[i].timestamp = lines[i].depth = 0.0;
                for (int q = 0; q < 4; ++q) o[q] += c[q];
            }
            put_lines(out, p, MOPS::Common::RemoveNaNTrajectoriesAndReindex(lines));
        } else {
            die("unknown op " + std::to_string(op));
        }
    }
    write_bag(argv[2], out);
    return 0;
}
