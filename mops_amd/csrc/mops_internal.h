// mops_internal.h -- what mops_engine.hip (the trajectory engine and what feeds it) and mops_analysis.hip (the
// analysis and imaging entries) both use, and nothing else.  Private to the two translation units: not installed
// under include/, not part of the ABI.  The trajectory tuning macros stay in mops_engine.hip.
#ifndef MOPS_INTERNAL_H
#define MOPS_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "mops_traj.h"

// records `msg` as the calling thread's mops_last_error and returns `st` (defined in mops_engine.hip)
__attribute__((visibility("hidden"))) mops_status fail(mops_status st, const std::string& msg);

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess)                                                           \
            return fail(MOPS_ERR_HIP, std::string(#expr " failed: ") + hipGetErrorString(_e)); \
    } while (0)

#define MOPS_TRY(expr)                 \
    do {                               \
        mops_status _s = (expr);       \
        if (_s != MOPS_OK) return _s;  \
    } while (0)

namespace {

constexpr int kMaxLevels = 100;  // reference MAX_VERTICAL_LEVEL_NUM
constexpr int kMaxVertex = 20;   // reference MAX_VERTEX_NUM
constexpr int kBlock = 256;
constexpr int kPairRec = 10;  // doubles per level-pair record (see mops_field::d_pr)
// Level-pair record layout (mops_field::d_pr) in 16-B pieces: record-major and level-major, [L-1][V][5] -- the
// five pieces of the record of layer k1 = k-1 and vertex v are contiguous -- plus one all-zero record after the
// last.  (The piece-major layout measured slower: DESIGN.md section 3.6.)
// (all in 16-B piece units; uint32 throughout: mops_mesh_create checks pr_pieces < 2^32)
__host__ __device__ __forceinline__ uint32_t pr_base(uint32_t k1, uint32_t v, uint32_t V) {  // piece 0
    return (k1 * V + v) * 5u;
}
__host__ __device__ __forceinline__ uint32_t pr_zero(uint32_t V, uint32_t L) {  // the all-zero record's piece 0
    return (L - 1u) * V * 5u;
}

}  // namespace

struct mops_mesh {
    int64_t C = 0, V = 0;
    int maxE = 0, L = 0;
    int maxv = 0;       // stencil capacity of the kernel instantiation (7, 12 or 20)
    int rec_ints = 0;   // ints per cell record
    int* d_cellrec = nullptr;    // [C][rec_ints]: nEdges | voc[maxv] | coc[maxv] (0-based, -1 none)
    double4* d_cxyz = nullptr;   // [C] (x,y,z,0)
    double4* d_vxyz = nullptr;   // [V]
    int* d_cov = nullptr;        // [V][3] cellsOnVertex 0-based, -1 = missing (boundary)
    double4* d_bary = nullptr;   // [V] barycentric weights in the cellsOnVertex centres (vertex_bary_kernel)
    // seed-location bucket index
    double bucket_h = 0.0, bucket_origin = 0.0;
    int origin_cell = -1;  // exact nearest centre to (0,0,0) (locate_kernel's tie rule)
    uint64_t* d_bkeys = nullptr;  // sorted bucket keys [C]
    int* d_bcells = nullptr;      // cell ids in key order [C]
    // bucket directory: open-addressing hash table (load <= 1/2) from a non-empty bucket's
    // key to its {first entry, entry count} in d_bkeys/d_bcells
    uint64_t* d_hkeys = nullptr;  // [H] key or ~0 (empty)
    int2* d_hval = nullptr;       // [H]
    uint32_t hmask = 0;           // H - 1
    uint32_t* d_cell_rank = nullptr;  // rank of each cell in the Morton order of the centres (particle locality order)
    int* d_rank_cell = nullptr;       // the inverse: the cell of each rank
    double2* d_cpolyr = nullptr;      // [2*7][C] d_cpoly's pieces by cell rank (maxv 7 meshes; MOPS_CPOLY_RANK)
    // [C][maxv] each cell's polygon in rotated slot order with its Wachspress weights' numerators:
    // slot j = {poly[j-1] (poly[-1] = poly[nv-1]), B_j = area(poly[j-1], poly[j], poly[j+1])}, zeros past nv
    double4* d_cpoly = nullptr;
    double* d_cnrm = nullptr;    // [C][kCellNrm] IsInMesh edge normals of the rotated polygon slots (maxv 7 meshes)
    uint4* d_nbr = nullptr;      // [C][kNbrQ] neighbour table (cell_nbr_kernel, dev::nbr_stay; maxv 7 meshes)
    double* d_rloc2 = nullptr;       // [C] squared hinted-locate radius (locate_radius_kernel)
    double* d_ring = nullptr;        // [C] hinted-locate ring distance (locate_radius_kernel)
    // grow-only scratch for mops_order_particles (not re-entrant, like the reference's global app)
    mutable void* d_scratch = nullptr;
    mutable size_t scratch_bytes = 0;
    int64_t bytes = 0;
    std::vector<int> h_nv;  // nEdgesOnCell (host copy, for mops_mesh_set_edges' validation)
    // edges (mops_mesh_set_edges): the RBF reconstruction's per-cell stencil, solved once
    int64_t E = 0;
    int* d_eoc = nullptr;        // [C][7] edgesOnCell 0-based, -1 = none
    int2* d_coe = nullptr;       // [E] cellsOnEdge 0-based, -1 = none (the reference's SIZE_MAX)
    double4* d_exyz = nullptr;   // [E] edgeCoord
    double* d_rbf_coef = nullptr;  // [C][7][3] RBF coefficients (rbf_coef_kernel)
    int* d_rbf_slot = nullptr;     // [C][7] edge read by each slot, -1 = velocity 0
    // MOPS_VPERM: internal vertex i is the caller's vertex h_vold[i] (Morton order); every vertex-indexed array
    // (coordinates, cellsOnVertex, the derived fields and records) is internal, and the vertex ids in the cell
    // records are internal ids.  The vertex-array entry points map at the boundary (mops_field_create_derived,
    // mops_field_export: host rows; mops_cell_to_vertex_attr: d_vold).  Empty / NULL = identity.
    std::vector<int> h_vold;
    int* d_vold = nullptr;
    // the pathline launches' instantiation flag (coop_select_kernel), one per HIP stream: launches on
    // one stream run in order, so the next launch's selection never overwrites a flag a running
    // trajectory kernel still reads; allocated once per stream (no per-launch allocation).  `launches` counts, on
    // the host, the stream's launches that ran the selection (mops_traj_selection's witness)
    struct CoopFlag {
        hipStream_t stream;
        int* d_flag;
        int64_t launches;
    };
    mutable std::mutex coop_mu;
    mutable std::vector<CoopFlag> coop_flags;
    // the pathline launches' time-fraction tables (alpha_table), one per distinct number of steps: a run's
    // n_steps comes from its settings, so a mesh sees one or a few; built on the first launch that needs it
    mutable std::vector<std::pair<int64_t, double*>> alpha_tabs;
};

struct mops_field {
    const mops_mesh* mesh = nullptr;
    int64_t V = 0;
    int L = 0;
    double* d_zt = nullptr;   // cellVertexZTop [V][L]
    double* d_vel = nullptr;  // cellVertexVelocity [V][L][3]
    double* d_w = nullptr;    // cellVertexVertVelocity [V][L+1]
    // [C] fast-path word (mono_kernel, read by dev::fast_ok): bit 31 = eligible, bits 20..26 = km,
    // the cell's decreasing prefix (every non-zero vertex column drops by >= 1e-6 m per level over
    // levels 0..km), bits 0..19 = which polygon slots are identically-zero columns (boundary
    // vertices, quirk Q10); bits 29-30 (a property of the mesh cell, kept here because the evaluation has
    // this word in a register): set unless the cell's Wachspress numerators all qualify for dev::wach_fast
    uint32_t* d_mono = nullptr;
    int32_t* d_vmono = nullptr;  // [V] first level that breaks the vertex column's decrease (L = none)
    uint8_t* d_vzero = nullptr;  // [V] 1 = every level of the vertex column is 0 (boundary vertex)
    // level-pair records [V][L-1][kPairRec] doubles, record k-1 of vertex v =
    // {z_{k-1}, z_k, w_{k-1}, w_k, vel_{k-1} (3), vel_k (3)}: one 80-B,
    // 16-B-aligned read (5 x dwordx4) gives a vertex's whole contribution when
    // the particle sits in layer k
    double* d_pr = nullptr;
    // derivation intermediates (cell zTop [C][L], cell-centre xyz velocity [C][L][3]), kept
    // only by fields built from device arrays so mops_field_rebuild_device never allocates
    double* d_ztc = nullptr;
    double* d_velc = nullptr;
    // d_vel / d_w hold every value (fields uploaded as vertex arrays); false after the fused
    // derivation (pair_record_fused_kernel), which writes only the records, d_zt and w at level L:
    // mops_field_export then rebuilds d_vel / d_w from the records (records_to_vertex_kernel)
    bool vtx_full = true;
    int64_t bytes = 0;
};

// A fused field's d_vel / d_w rebuilt from its records on `s` (records_to_vertex_kernel, so that the kernel
// stays in mops_engine.hip alone); nothing for a field whose vertex arrays hold every value (see vtx_full)
__attribute__((visibility("hidden"))) void records_to_vertex(const mops_field* f, hipStream_t s);

namespace {

template <typename T>
mops_status dmalloc(T** p, size_t count, int64_t* acc) {
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
    if (e != hipSuccess) return fail(MOPS_ERR_HIP, std::string("hipMalloc failed: ") + hipGetErrorString(e));
    if (acc) *acc += (int64_t)(count * sizeof(T));
    return MOPS_OK;
}

inline unsigned grid_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// mesh->maxv as a compile-time constant: f(std::integral_constant<int, MAXV>{}) for the mesh's stencil capacity,
// so a launch site names its kernel once (kernel<MAXV()><<<...>>>) and the instantiations for 7, 12 and 20 follow.
// mops_mesh_create's pick_maxv only ever yields 7, 12 or 20, so `case 7 / case 12 / default` here and the
// `<= 7 / <= 12 / else` that some launch sites used to spell out choose the same kernel for every mesh.
// -DMOPS_ONLY7 (experiment builds) leaves the MAXV 7 instantiations only; another mesh is an error.
template <class F>
mops_status with_maxv(int maxv, F&& f) {
    switch (maxv) {
        case 7: f(std::integral_constant<int, 7>{}); break;
#if !defined(MOPS_ONLY7)
        case 12: f(std::integral_constant<int, 12>{}); break;
        default: f(std::integral_constant<int, 20>{}); break;
#else
        default: return fail(MOPS_ERR_UNSUPPORTED, "experiment build: MAXV 7 only");
#endif
    }
    return MOPS_OK;
}

}  // namespace

namespace dev {

// Ablation hooks for perf experiments only (tools/build_variant.sh -DMOPS_ABL_*):
// they break parity and are never set in a product build.
#if defined(MOPS_ABL_SQRT)
__device__ __forceinline__ double xsqrt(double x) { return x * __builtin_amdgcn_rsq(x); }
#else
// Correctly rounded sqrt, bit-identical to the compiler's sqrt(): for x in
// [2^-767, inf) its gfx950 expansion is exactly this rsq + Newton/Markstein
// sequence -- the input/output ldexp scaling (for x < 2^-767) and the +-0/+inf
// select around it are then identities, so they are skipped here.  Other x
// (0, tiny, inf, NaN, negative) take sqrt() itself.  Checked bitwise against
// sqrt() on the device and the host (mops_selftest_math, tests/test_gpu_parity.py).
__device__ __forceinline__ double sqrt_core(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y;
    double h = y * 0.5;
    double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
#ifndef MOPS_FAST_SQRT
#define MOPS_FAST_SQRT 1
#endif
__device__ __forceinline__ double xsqrt(double x) {
#if MOPS_FAST_SQRT
    // the core result always, the library's only for the rare out-of-range x: a one-sided branch
    // (fewer exec-mask instructions than if/else; measured: streamline Euler segment 27.0 -> 26.0 ms,
    // RK4 86.5 -> 85.2 ms)
    double r = sqrt_core(x);
    if (__builtin_expect(!(x >= 0x1p-767 && x < __builtin_huge_val()), 0)) r = sqrt(x);
    return r;
#else
    return sqrt(x);
#endif
}
#endif

// Interpolator::triangle_area (Interpolation.hpp:95-110)
__device__ __forceinline__ double tri_area(double ax, double ay, double az, double bx, double by, double bz,
                                           double cx, double cy, double cz) {
    const double e1x = bx - ax, e1y = by - ay, e1z = bz - az;
    const double e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    const double px = e1y * e2z - e1z * e2y;
    const double py = e1z * e2x - e1x * e2z;
    const double pz = e1x * e2y - e1y * e2x;
    return xsqrt(px * px + py * py + pz * pz) / 2.0;
}

__device__ __forceinline__ double dmax(double a, double b) { return (a < b) ? b : a; }  // std::max

}  // namespace dev

#endif  // MOPS_INTERNAL_H
