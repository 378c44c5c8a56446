// mops_analysis.hip -- the analysis and imaging entries on a mesh and its fields: image remapping, vertical
// sections, the velocity gradient, the eddy census, the colormap, density maps and FTLE.  They share the mesh
// and field structs, the error and allocation helpers and a few device functions with the trajectory engine
// (mops_internal.h) and locate through the public mops_locate_cells; nothing here reads a trajectory tuning
// knob, and nothing in mops_engine.hip's hot path is compiled from this file.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "mops_internal.h"
#include "mops_traj.h"

// ===========================================================================
// image remapping: fixed depth (Kernel::VisualizeFixedDepth,
// MPASOVisualizerKernels.cpp:238-471) and fixed latitude (VisualizeFixedLatitude,
// :473-651).  One lane per pixel; the plain reference forms throughout (the
// trajectory path's cached / rescaled stencils are not used here), so every
// element sees the reference's operations in the reference's order.
// ===========================================================================
namespace {

constexpr double kRemapRadius = 6371010.0;  // GeoConverter.hpp:107 (6371010.0f is exact in float)

// GeoConverter::convertRadianLatLonToXYZ (GeoConverter.hpp:118-124) from the host's libm tables: the latitude
// depends on the row only, the longitude on the column only
__global__ void __launch_bounds__(256) remap_positions_kernel(int64_t n, int W, const double* __restrict__ row_cos,
                                                              const double* __restrict__ row_sin,
                                                              const double* __restrict__ col_cos,
                                                              const double* __restrict__ col_sin,
                                                              double* __restrict__ pts) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const int64_t i = g / W;
    const int j = (int)(g - i * W);
    const double r = kRemapRadius;
    const double costheta = row_cos[i], sintheta = row_sin[i], cosphi = col_cos[j], sinphi = col_sin[j];
    pts[3 * g + 0] = r * costheta * cosphi;
    pts[3 * g + 1] = r * costheta * sinphi;
    pts[3 * g + 2] = r * sintheta;
}

struct RemapArgs {
    int64_t n;                 // pixels
    int W;
    int64_t C, V;
    int L, rec_ints;
    const int* cellrec;
    const double4* vxyz;
    const double* zt;          // [V][L] internal vertex order
    const double* pr;          // level-pair records (L >= 2), else NULL
    const double* vel;         // [V][L][3] (read only when pr is NULL)
    const int* vold;           // internal vertex -> the caller's vertex (attribute arrays), NULL = identity
    const double* attr0;       // [V][L] in the caller's vertex order, or NULL
    const double* attr1;
    const double* pts;         // fixed depth: [n][3]; fixed latitude: [W][3]
    const int* cells;          // fixed depth: [n]; fixed latitude: [W]
    double depth;              // fixed depth: DEPTH = -FixedDepth
    double min_depth, i_step;  // fixed latitude rows
    int bracket;               // layer rule
    double* img0;
    double* img1;              // written only with two or more attributes
};

template <int MAXV>
struct RemapStencil {
    int nv;
    int vid[MAXV];
    double w[MAXV];
};

__device__ __forceinline__ void remap_set_pixel(double* img, int64_t g, double x, double y, double z) {
    // SetPixel (ImageBuffer.hpp:68-77): alpha 1.0 for every written pixel, NaN ones included
    img[4 * g + 0] = x;
    img[4 * g + 1] = y;
    img[4 * g + 2] = z;
    img[4 * g + 3] = 1.0;
}

// The cell's vertices, the inside test and the Wachspress weights.  OCEAN false: TBBKernel::IsInMesh
// (TBBKernel.h:21-54); true: MPASOField::isOnOcean (MPASOField.cpp:36-81), a sign-consistency test on (p - A).
// Then Interpolator::CalcPolygonWachspress (Interpolation.hpp:137-165).  false = the pixel is NaN.
// TAG: the section kernel's instantiations are its own (kSectionTag), so the curtain's code does not move.
template <int MAXV, bool OCEAN, int TAG = 0>
__device__ __forceinline__ bool remap_stencil(const RemapArgs& a, int cell, double px, double py, double pz,
                                              RemapStencil<MAXV>& s) {
    const int* r = a.cellrec + (int64_t)cell * a.rec_ints;
    const int nv = r[0];
    s.nv = nv;
    if (nv <= 0 || nv > MAXV) return false;
    if (!OCEAN && !(isfinite(px) && isfinite(py) && isfinite(pz))) return false;
    double x[MAXV], y[MAXV], z[MAXV];
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
        s.vid[k] = 0; s.w[k] = 0.0;
        x[k] = 0.0; y[k] = 0.0; z[k] = 0.0;
        if (k < nv) {
            const int v = r[1 + k];
            if (v < 0 || v >= a.V) return false;
            s.vid[k] = v;
            const double4 q = a.vxyz[v];
            x[k] = q.x; y[k] = q.y; z[k] = q.z;
        }
    }
    double lx = 0.0, ly = 0.0, lz = 0.0;  // poly[nv-1]
#pragma unroll
    for (int k = 0; k < MAXV; ++k)
        if (k == nv - 1) { lx = x[k]; ly = y[k]; lz = z[k]; }
    bool first_pos = false, ok = true;
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
        if (k < nv) {
            const bool wrap = (k + 1 >= nv);
            const double bx = wrap ? x[0] : x[(k + 1) % MAXV];
            const double by = wrap ? y[0] : y[(k + 1) % MAXV];
            const double bz = wrap ? z[0] : z[(k + 1) % MAXV];
            if (!OCEAN) {
                const double nx = y[k] * bz - z[k] * by;
                const double ny = z[k] * bx - x[k] * bz;
                const double nz = x[k] * by - y[k] * bx;
                const double direction = nx * px + ny * py + nz * pz;
                if (direction < 0.0) ok = false;
            } else {
                const double aox = 0.0 - x[k], aoy = 0.0 - y[k], aoz = 0.0 - z[k];
                const double box = 0.0 - bx, boy = 0.0 - by, boz = 0.0 - bz;
                const double apx = px - x[k], apy = py - y[k], apz = pz - z[k];
                const double nx = aoy * boz - aoz * boy;
                const double ny = aoz * box - aox * boz;
                const double nz = aox * boy - aoy * box;
                const double direction = nx * apx + ny * apy + nz * apz;
                const bool pos = direction > 0;
                if (k == 0) first_pos = pos;
                if (pos != first_pos) ok = false;  // is_land
            }
        }
    }
    if (!ok) return false;
    double sumweights = 0.0;
    double A_iplus1 = dev::tri_area(lx, ly, lz, x[0], y[0], z[0], px, py, pz);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        if (i < nv) {
            const bool wrap = (i + 1 >= nv);
            const double nx = wrap ? x[0] : x[(i + 1) % MAXV];
            const double ny = wrap ? y[0] : y[(i + 1) % MAXV];
            const double nz = wrap ? z[0] : z[(i + 1) % MAXV];
            const double qx = (i == 0) ? lx : x[(i + MAXV - 1) % MAXV];
            const double qy = (i == 0) ? ly : y[(i + MAXV - 1) % MAXV];
            const double qz = (i == 0) ? lz : z[(i + MAXV - 1) % MAXV];
            const double A_i = A_iplus1;
            A_iplus1 = dev::tri_area(x[i], y[i], z[i], nx, ny, nz, px, py, pz);
            const double B = dev::tri_area(qx, qy, qz, x[i], y[i], z[i], nx, ny, nz);
            s.w[i] = B / (A_i * A_iplus1);
            sumweights += s.w[i];
        }
    }
    const double recp = 1.0 / sumweights;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (i < nv) s.w[i] *= recp;
    return true;
}

// One pass over the clamped zTop column (MPASOVisualizerKernels.cpp:346-360 / :573-587) without storing it:
// z[0], the last clamped value, and the first level k whose (z[k-1], z[k]) satisfies the layer search
// predicate (:379-391 with tol 1e-8 / :597-607 with 1e-6), with that pair.  Returns that k or -1.
template <int MAXV>
__device__ __forceinline__ int remap_column(const RemapArgs& a, const RemapStencil<MAXV>& s, double D, double tol,
                                            double& z0, double& zlast, double& ztop, double& zbot) {
    int found = -1;
    double prev = 0.0;
    ztop = 0.0; zbot = 0.0;
    for (int k = 0; k < a.L; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int v = 0; v < MAXV; ++v)
            if (v < s.nv) acc += s.w[v] * a.zt[(int64_t)s.vid[v] * a.L + k];
        if (k == 0) {
            z0 = acc;
        } else {
            if (acc > prev) acc = prev - 1e-9;
            double topI = prev, botI = acc;
            if (topI < botI) { const double t = topI; topI = botI; botI = t; }
            if (found < 0 && D <= topI + tol && D >= botI - tol) { found = k; ztop = prev; zbot = acc; }
        }
        prev = acc;
    }
    zlast = prev;
    return found;
}

// TBBKernel::CalcVelocity (TBBKernel.h:128-147) at one level: the vertex velocities are read from the
// level-pair records (level j < L-1 from record j, level L-1 from the second half of record L-2; the same
// doubles as cellVertexVelocity_vec), or from the vertex array of a one-level field
template <int MAXV>
__device__ __forceinline__ void remap_velocity(const RemapArgs& a, const RemapStencil<MAXV>& s, int level,
                                               double& vx, double& vy, double& vz) {
    vx = 0.0; vy = 0.0; vz = 0.0;
    const bool hi = a.pr && level == a.L - 1;
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
        if (v < s.nv) {
            const double* p;
            if (a.pr)
                p = a.pr + (size_t)pr_base((uint32_t)(hi ? level - 1 : level), (uint32_t)s.vid[v], (uint32_t)a.V) * 2u +
                    (hi ? 7 : 4);
            else
                p = a.vel + ((int64_t)s.vid[v] * a.L + level) * 3;
            vx += s.w[v] * p[0];
            vy += s.w[v] * p[1];
            vz += s.w[v] * p[2];
        }
    }
}

// TBBKernel::CalcAttribute (TBBKernel.h:149-166); the attribute arrays are in the caller's vertex order
template <int MAXV>
__device__ __forceinline__ double remap_attribute(const RemapArgs& a, const RemapStencil<MAXV>& s, int level,
                                                  const double* __restrict__ attr) {
    double r = 0.0;
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
        if (v < s.nv) {
            const int64_t vid = a.vold ? a.vold[s.vid[v]] : s.vid[v];
            r += s.w[v] * attr[vid * a.L + level];
        }
    }
    return r;
}

// GeoConverter::convertXYZVelocityToENU (GeoConverter.hpp:200-223)
__device__ __forceinline__ void remap_enu(double px, double py, double pz, double vx, double vy, double vz,
                                          double& Uzon, double& Umer) {
    if (px == 0.0 && py == 0.0) { Uzon = 0.0; Umer = 0.0; return; }
    const double Rxy = sqrt(px * px + py * py);
    const double Rxyz = sqrt(px * px + py * py + pz * pz);
    const double slon = py / Rxy;
    const double clon = px / Rxy;
    const double slat = pz / Rxyz;
    const double clat = Rxy / Rxyz;
    Uzon = -slon * vx + clon * vy;
    Umer = -slat * (clon * vx + slon * vy) + clat * vz;
}

template <int MAXV>
__global__ void __launch_bounds__(256) remap_fixed_depth_kernel(RemapArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    const double nan = __builtin_nan("");
    const int cell = a.cells[g];
    const double px = a.pts[3 * g], py = a.pts[3 * g + 1], pz = a.pts[3 * g + 2];
    RemapStencil<MAXV> s;
    bool ok = cell >= 0 && cell < a.C;                               // :299
    if (ok) ok = remap_stencil<MAXV, false>(a, cell, px, py, pz, s);  // :312-335
    if (ok) ok = a.L > 0 && a.L <= kMaxLevels;                       // :338
    const double DEPTH = a.depth;
    int local_layer = -1;
    double z0 = 0.0, zlast = 0.0, ftop = 0.0, fbot = 0.0;
    if (ok) {
        local_layer = remap_column<MAXV>(a, s, DEPTH, 1e-8, z0, zlast, ftop, fbot);
        double z_surf = z0, z_bot = zlast;
        if (z_surf < z_bot) { const double t = z_surf; z_surf = z_bot; z_bot = t; }
        const double epsd = dev::dmax(1e-6, 1e-8 * fabs(z_surf - z_bot));
        if (!(DEPTH <= z_surf + epsd && DEPTH >= z_bot - epsd)) ok = false;  // :370
    }
    if (ok) {
        if (!a.bracket && DEPTH <= z0) local_layer = 0;  // :392-394, the layer override (reference rule only)
        if (local_layer < 0) ok = false;                 // :395
    }
    if (!ok) {
        remap_set_pixel(a.img0, g, nan, nan, nan);
        if (a.img1) remap_set_pixel(a.img1, g, nan, nan, nan);
        return;
    }
    double topI = local_layer == 0 ? z0 : ftop;  // z[max(0, local_layer - 1)]
    double botI = local_layer == 0 ? z0 : fbot;  // z[local_layer]
    if (topI < botI) { const double t = topI; topI = botI; botI = t; }
    const double denom = topI - botI;
    const double tparam = (denom > 1e-12) ? (DEPTH - botI) / denom : 0.5;
    const int vel_levels = a.L;
    int j = local_layer - 1;
    j = j < 0 ? 0 : (j > vel_levels - 1 ? vel_levels - 1 : j);
    const int j_bot = (j + 1 < vel_levels - 1) ? j + 1 : vel_levels - 1;
    const int j_top = j;
    double tx, ty, tz, bx, by, bz;
    remap_velocity<MAXV>(a, s, j_top, tx, ty, tz);
    remap_velocity<MAXV>(a, s, j_bot, bx, by, bz);
    const double mtop = sqrt(tx * tx + ty * ty + tz * tz), mbot = sqrt(bx * bx + by * by + bz * bz);
    double fx, fy, fz;
    if (mtop < 1e-12 && mbot < 1e-12) {
        fx = 0.0; fy = 0.0; fz = 0.0;
    } else if (mtop < 1e-12) {
        fx = bx; fy = by; fz = bz;
    } else if (mbot < 1e-12) {
        fx = tx; fy = ty; fz = tz;
    } else {
        const double c = 1.0 - tparam;
        fx = c * bx + tparam * tx;
        fy = c * by + tparam * ty;
        fz = c * bz + tparam * tz;
    }
    double u_east, v_north;
    remap_enu(px, py, pz, fx, fy, fz, u_east, v_north);
    const double spd = sqrt(u_east * u_east + v_north * v_north);
    remap_set_pixel(a.img0, g, u_east, v_north, spd);
    if (a.img1) {  // :443-469: x = the first attribute, y = the second, both at level clamp(local_layer - 1)
        const double a0 = remap_attribute<MAXV>(a, s, j, a.attr0);
        const double a1 = remap_attribute<MAXV>(a, s, j, a.attr1);
        remap_set_pixel(a.img1, g, a0, a1, 0.0);
    }
}

template <int MAXV>
__global__ void __launch_bounds__(256) remap_fixed_latitude_kernel(RemapArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    const double nan = __builtin_nan("");
    const int ih = (int)(g / a.W);
    const int jw = (int)(g - (int64_t)ih * a.W);
    const double depth_plot = a.min_depth + ih * a.i_step;  // :536
    const double DEPTH = -fabs(depth_plot);
    const int cell = a.cells[jw];
    const double px = a.pts[3 * jw], py = a.pts[3 * jw + 1], pz = a.pts[3 * jw + 2];
    RemapStencil<MAXV> s;
    bool ok = cell >= 0 && cell < a.C;                              // :545
    if (ok) ok = remap_stencil<MAXV, true>(a, cell, px, py, pz, s);  // :551-570
    int layer = -1;
    double z0 = 0.0, zlast = 0.0, up = 0.0, dn = 0.0;
    if (ok) {
        const double EPSILON = 1e-6;
        layer = remap_column<MAXV>(a, s, DEPTH, EPSILON, z0, zlast, up, dn);
        if (DEPTH > z0 + EPSILON || DEPTH < zlast - EPSILON) ok = false;  // :592
        if (layer == -1) ok = false;                                      // :609
    }
    double denom = 0.0;
    if (ok) {
        if (up < dn) { const double t = up; up = dn; dn = t; }
        denom = up - dn;
        if (fabs(denom) < 1e-30) ok = false;  // :621
    }
    if (!ok) {
        remap_set_pixel(a.img0, g, nan, nan, nan);
        return;
    }
    const double t = (DEPTH - dn) / denom;
    double ux, uy, uz, dx, dy, dz;
    remap_velocity<MAXV>(a, s, layer - 1, ux, uy, uz);
    remap_velocity<MAXV>(a, s, layer, dx, dy, dz);
    const double c = 1.0 - t;
    const double fx = c * dx + t * ux, fy = c * dy + t * uy, fz = c * dz + t * uz;
    double zonal, meridional;
    remap_enu(px, py, pz, fx, fy, fz, zonal, meridional);
    remap_set_pixel(a.img0, g, zonal, meridional, 0.0);
}

// Kernel::VisualizeFixedLayer (MPASOVisualizerKernels.cpp:141-236): the fixed-depth kernel without the column
// search -- the velocity at one layer (ClampLayer(FixedLayer, L), from the host) for every pixel inside its cell
template <int MAXV>
__global__ void __launch_bounds__(256) remap_fixed_layer_kernel(RemapArgs a, int layer) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    const double nan = __builtin_nan("");
    const int cell = a.cells[g];
    const double px = a.pts[3 * g], py = a.pts[3 * g + 1], pz = a.pts[3 * g + 2];
    RemapStencil<MAXV> s;
    bool ok = cell >= 0 && cell < a.C;                               // :191
    if (ok) ok = remap_stencil<MAXV, false>(a, cell, px, py, pz, s);  // :196-220
    if (!ok) {
        remap_set_pixel(a.img0, g, nan, nan, nan);
        return;
    }
    double vx, vy, vz;
    remap_velocity<MAXV>(a, s, layer, vx, vy, vz);  // :222-228
    double zonal, meridional;
    remap_enu(px, py, pz, vx, vy, vz, zonal, meridional);
    remap_set_pixel(a.img0, g, zonal, meridional, 0.0);
}

// GeoConverter::convertPixelToLatLonToRadians (GeoConverter.hpp:28-32) per row / per column, then the
// libm cos / sin of convertRadianLatLonToXYZ (:120-121)
void remap_depth_tables(const mops_remap_cfg* c, double* row_cos, double* row_sin, double* col_cos, double* col_sin) {
    const int width = c->width, height = c->height;
    for (int i = 0; i < height; ++i) {
        double lat = c->max_lat - (static_cast<double>(i) / static_cast<double>(height) * (c->max_lat - c->min_lat));
        lat = lat * (M_PI / 180.0);
        row_cos[i] = std::cos(lat); row_sin[i] = std::sin(lat);
    }
    for (int j = 0; j < width; ++j) {
        double lon = (static_cast<double>(j) / static_cast<double>(width) * (c->max_lon - c->min_lon)) + c->min_lon;
        lon = lon * (M_PI / 180.0);
        col_cos[j] = std::cos(lon); col_sin[j] = std::sin(lon);
    }
}

// VisualizeFixedLatitude's positions (MPASOVisualizerKernels.cpp:513-523): one row at FixedLatitude,
// lon = minLon + jw * j_step
void remap_latitude_tables(const mops_remap_cfg* c, double* row_cos, double* row_sin, double* col_cos,
                           double* col_sin) {
    const int width = c->width;
    const double j_step = (width > 1) ? (c->max_lon - c->min_lon) / (width - 1) : 0.0;
    const double lat = c->fixed_latitude * (M_PI / 180.0);
    row_cos[0] = std::cos(lat); row_sin[0] = std::sin(lat);
    for (int jw = 0; jw < width; ++jw) {
        const double lon = c->min_lon + jw * j_step;
        const double phi = lon * (M_PI / 180.0);
        col_cos[jw] = std::cos(phi); col_sin[jw] = std::sin(phi);
    }
}

mops_status remap_check(const char* what, const mops_mesh* mesh, const mops_field* field, const mops_remap_cfg* cfg,
                        const void* d_out) {
    if (!mesh || !field || !cfg || !d_out) return fail(MOPS_ERR_INVALID, std::string(what) + ": invalid inputs");
    if (cfg->width <= 0 || cfg->height <= 0 || (int64_t)cfg->width * cfg->height > 0x7fffffffLL)
        return fail(MOPS_ERR_INVALID, std::string(what) + ": invalid image size");
    if (cfg->layer_rule != MOPS_LAYER_REFERENCE && cfg->layer_rule != MOPS_LAYER_BRACKET)
        return fail(MOPS_ERR_INVALID, std::string(what) + ": invalid layer rule");
    if (field->mesh != mesh) return fail(MOPS_ERR_INVALID, std::string(what) + ": the field belongs to another mesh");
    return MOPS_OK;
}

RemapArgs remap_args(const mops_mesh* mesh, const mops_field* f, const mops_remap_cfg* cfg) {
    RemapArgs a{};
    a.W = cfg->width;
    a.C = mesh->C; a.V = mesh->V; a.L = mesh->L; a.rec_ints = mesh->rec_ints;
    a.cellrec = mesh->d_cellrec; a.vxyz = mesh->d_vxyz;
    a.zt = f->d_zt; a.pr = mesh->L >= 2 ? f->d_pr : nullptr; a.vel = f->d_vel;
    a.vold = mesh->d_vold;
    a.bracket = cfg->layer_rule == MOPS_LAYER_BRACKET;
    return a;
}

// positions -> locate -> `eval` on one scratch allocation: tables [2 rows + 2 W] | points [np][3] | cells [np]
template <typename Eval>
mops_status remap_run(const mops_mesh* mesh, int rows, int W, const std::vector<double>& tables, int32_t* d_cells,
                      float* h_stage_ms, hipStream_t s, Eval eval) {
    const int64_t np = (int64_t)rows * W;
    const size_t ntab = tables.size();
    double* scratch = nullptr;
    int32_t* own_cells = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    mops_status st = MOPS_OK;
    do {
        if ((st = dmalloc(&scratch, ntab + (size_t)np * 3, nullptr)) != MOPS_OK) break;
        if (!d_cells) {
            if ((st = dmalloc(&own_cells, (size_t)np, nullptr)) != MOPS_OK) break;
            d_cells = own_cells;
        }
        hipError_t e = hipMemcpyAsync(scratch, tables.data(), ntab * sizeof(double), hipMemcpyHostToDevice, s);
        for (int k = 0; k < 4 && e == hipSuccess && h_stage_ms; ++k) e = hipEventCreate(&ev[k]);
        if (e != hipSuccess) { st = fail(MOPS_ERR_HIP, std::string("remap: ") + hipGetErrorString(e)); break; }
        double* pts = scratch + ntab;
        if (h_stage_ms) (void)hipEventRecord(ev[0], s);
        remap_positions_kernel<<<grid_for(np), 256, 0, s>>>(np, W, scratch, scratch + rows, scratch + 2 * rows,
                                                           scratch + 2 * rows + W, pts);
        if (h_stage_ms) (void)hipEventRecord(ev[1], s);
        if ((st = mops_locate_cells(mesh, np, pts, d_cells, s)) != MOPS_OK) break;
        if (h_stage_ms) (void)hipEventRecord(ev[2], s);
        if ((st = eval(pts, d_cells)) != MOPS_OK) break;
        if (h_stage_ms) (void)hipEventRecord(ev[3], s);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { st = fail(MOPS_ERR_HIP, std::string("remap: ") + hipGetErrorString(e)); break; }
        for (int k = 0; k < 3 && h_stage_ms; ++k) (void)hipEventElapsedTime(&h_stage_ms[k], ev[k], ev[k + 1]);
    } while (0);
    for (int k = 0; k < 4; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    (void)hipFree(scratch);
    (void)hipFree(own_cells);
    return st;
}

}  // namespace

extern "C" {

int32_t mops_remap_num_images(int32_t n_attr) { return n_attr > 0 ? 1 + (n_attr + 2) / 3 : 1; }

mops_status mops_remap_tables(const mops_remap_cfg* cfg, int32_t fixed_latitude, double* h_row_cos, double* h_row_sin,
                              double* h_col_cos, double* h_col_sin) {
    if (!cfg || !h_row_cos || !h_row_sin || !h_col_cos || !h_col_sin || cfg->width <= 0 || cfg->height <= 0)
        return fail(MOPS_ERR_INVALID, "mops_remap_tables: invalid argument");
    if (fixed_latitude) remap_latitude_tables(cfg, h_row_cos, h_row_sin, h_col_cos, h_col_sin);
    else remap_depth_tables(cfg, h_row_cos, h_row_sin, h_col_cos, h_col_sin);
    return MOPS_OK;
}

mops_status mops_remap_fixed_depth(const mops_mesh* mesh, const mops_field* field, const mops_remap_cfg* cfg,
                                   int32_t n_attr, const double* d_attr0, const double* d_attr1, double* d_images,
                                   int32_t* d_cells, float* h_stage_ms, void* stream) {
    MOPS_TRY(remap_check("mops_remap_fixed_depth", mesh, field, cfg, d_images));
    if (n_attr < 0 || (n_attr >= 2 && (!d_attr0 || !d_attr1)))
        return fail(MOPS_ERR_INVALID, "mops_remap_fixed_depth: invalid attribute arrays");
    hipStream_t s = (hipStream_t)stream;
    const int W = cfg->width, H = cfg->height;
    const int64_t n = (int64_t)W * H;
    const int n_img = mops_remap_num_images(n_attr);
    const bool two = n_attr > 1;  // bDoubleAttributes (:261): image 1 is written only then
    // ImageBuffer's zero fill (ImageBuffer.hpp:15) for the images the kernel never writes
    if (n_img > (two ? 2 : 1))
        HIP_TRY(hipMemsetAsync(d_images + (size_t)(two ? 2 : 1) * n * 4, 0,
                               (size_t)(n_img - (two ? 2 : 1)) * n * 4 * sizeof(double), s));
    std::vector<double> tables(2 * (size_t)H + 2 * (size_t)W);
    remap_depth_tables(cfg, tables.data(), tables.data() + H, tables.data() + 2 * H, tables.data() + 2 * H + W);
    RemapArgs a = remap_args(mesh, field, cfg);
    a.n = n;
    a.depth = -cfg->fixed_depth;  // :251
    a.img0 = d_images;
    a.img1 = two ? d_images + n * 4 : nullptr;
    a.attr0 = two ? d_attr0 : nullptr;
    a.attr1 = two ? d_attr1 : nullptr;
    return remap_run(mesh, H, W, tables, d_cells, h_stage_ms, s, [&](const double* pts, const int32_t* cells) {
        a.pts = pts; a.cells = cells;
        return with_maxv(mesh->maxv,
                         [&](auto MAXV) { remap_fixed_depth_kernel<MAXV()><<<grid_for(a.n), 256, 0, s>>>(a); });
    });
}

mops_status mops_remap_fixed_latitude(const mops_mesh* mesh, const mops_field* field, const mops_remap_cfg* cfg,
                                      double* d_image, int32_t* d_cells, void* stream) {
    MOPS_TRY(remap_check("mops_remap_fixed_latitude", mesh, field, cfg, d_image));
    hipStream_t s = (hipStream_t)stream;
    const int W = cfg->width, H = cfg->height;
    std::vector<double> tables(2 + 2 * (size_t)W);
    remap_latitude_tables(cfg, tables.data(), tables.data() + 1, tables.data() + 2, tables.data() + 2 + W);
    RemapArgs a = remap_args(mesh, field, cfg);
    a.n = (int64_t)W * H;
    a.min_depth = cfg->min_depth;
    a.i_step = (H > 1) ? (cfg->max_depth - cfg->min_depth) / (H - 1) : 0.0;  // :513
    a.img0 = d_image;
    return remap_run(mesh, 1, W, tables, d_cells, nullptr, s, [&](const double* pts, const int32_t* cells) {
        a.pts = pts; a.cells = cells;
        return with_maxv(mesh->maxv,
                         [&](auto MAXV) { remap_fixed_latitude_kernel<MAXV()><<<grid_for(a.n), 256, 0, s>>>(a); });
    });
}

mops_status mops_remap_fixed_layer(const mops_mesh* mesh, const mops_field* field, const mops_remap_cfg* cfg,
                                   double* d_image, int32_t* d_cells, void* stream) {
    MOPS_TRY(remap_check("mops_remap_fixed_layer", mesh, field, cfg, d_image));
    if (mesh->L <= 0) return fail(MOPS_ERR_INVALID, "mops_remap_fixed_layer: invalid layer metadata");  // :158
    hipStream_t s = (hipStream_t)stream;
    const int W = cfg->width, H = cfg->height;
    std::vector<double> tables(2 * (size_t)H + 2 * (size_t)W);
    remap_depth_tables(cfg, tables.data(), tables.data() + H, tables.data() + 2 * H, tables.data() + 2 * H + W);
    RemapArgs a = remap_args(mesh, field, cfg);
    a.n = (int64_t)W * H;
    // ClampLayer((int)FixedLayer, L) (:14-26, :166): the double truncates toward zero; a NaN (undefined in the
    // reference) gives layer 0
    const double fl = cfg->fixed_layer;
    const int layer = !(fl >= 1.0) ? 0 : (fl >= (double)mesh->L ? mesh->L - 1 : (int)fl);
    a.img0 = d_image;
    return remap_run(mesh, H, W, tables, d_cells, nullptr, s, [&](const double* pts, const int32_t* cells) {
        a.pts = pts; a.cells = cells;
        return with_maxv(mesh->maxv, [&](auto MAXV) {
            remap_fixed_layer_kernel<MAXV()><<<grid_for(a.n), 256, 0, s>>>(a, layer);
        });
    });
}

}  // extern "C"

// ===========================================================================
// vertical sections along great-circle paths (mops_section_points, mops_remap_section,
// mops_section_transport; no reference counterpart beyond the pixel, which is VisualizeFixedLatitude's).
// A column's position, cell, inside test, Wachspress weights and weighted zTop column do not depend on the
// row, so one wave owns one column: every lane forms the column's stencil (wave-uniform operands), the lanes
// share out the L level sums into LDS, lane 0 applies the monotone clamp's recurrence in place, and then each
// lane takes rows ih = lane, lane + 64, ...: the layer search over the LDS column, two level sums for the
// velocity and two per attribute.  Every value comes out of the per-pixel form's FP64 expressions in that
// form's order (remap_stencil / remap_velocity / remap_attribute / remap_enu inline here as they do there; the
// search is remap_column's with the level sums read back from LDS), so the bytes do not depend on the split.
// ===========================================================================
namespace {

constexpr int kSectionBlock = 64;  // one wave per column
constexpr int kSectionTag = 1;     // remap_stencil's instantiations of the section kernel's own

struct SectionArgs {
    RemapArgs r;        // W, mesh and field arrays, pts [W][3], cells [W], min_depth, i_step, attr0 / attr1, img0 / img1
    const double* nrm;  // [W][3] unit normals, or NULL (across = 0.0)
    int H;
    int n_attr;         // 0..2; img1 is written iff >= 1
};

template <int MAXV>
__global__ void __launch_bounds__(kSectionBlock) remap_section_kernel(SectionArgs sa) {
    __shared__ double zs[kMaxLevels];  // the column's weighted zTop, clamped in place (L <= kMaxLevels: host check)
    const RemapArgs& a = sa.r;
    const int jw = (int)blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int L = a.L;
    const double nan = __builtin_nan("");
    const int cell = a.cells[jw];
    const double px = a.pts[3 * (int64_t)jw], py = a.pts[3 * (int64_t)jw + 1], pz = a.pts[3 * (int64_t)jw + 2];
    RemapStencil<MAXV> s;
    bool col_ok = cell >= 0 && cell < a.C;                                  // :545
    if (col_ok) col_ok = remap_stencil<MAXV, true, kSectionTag>(a, cell, px, py, pz, s);  // :551-570
    if (col_ok) {
        for (int k = lane; k < L; k += kSectionBlock) {  // :573-580, one level per lane
            double acc = 0.0;
#pragma unroll
            for (int v = 0; v < MAXV; ++v)
                if (v < s.nv) acc += s.w[v] * a.zt[(int64_t)s.vid[v] * L + k];
            zs[k] = acc;
        }
    }
    __syncthreads();
    if (col_ok && lane == 0) {  // :581-587, z[k] = z[k-1] - 1e-9 on the previous clamped value
        double prev = zs[0];
        for (int k = 1; k < L; ++k) {
            double acc = zs[k];
            if (acc > prev) { acc = prev - 1e-9; zs[k] = acc; }
            prev = acc;
        }
    }
    __syncthreads();
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (sa.nrm) { nx = sa.nrm[3 * (int64_t)jw]; ny = sa.nrm[3 * (int64_t)jw + 1]; nz = sa.nrm[3 * (int64_t)jw + 2]; }
    const double EPSILON = 1e-6;
    for (int ih = lane; ih < sa.H; ih += kSectionBlock) {
        const int64_t g = (int64_t)ih * a.W + jw;
        const double depth_plot = a.min_depth + ih * a.i_step;  // :536
        const double DEPTH = -fabs(depth_plot);
        bool ok = col_ok;
        if (ok && (DEPTH > zs[0] + EPSILON || DEPTH < zs[L - 1] - EPSILON)) ok = false;  // :592
        int layer = -1;
        double up = 0.0, dn = 0.0;
        if (ok) {
            for (int k = 1; k < L; ++k) {  // :597-607
                const double prev = zs[k - 1], acc = zs[k];
                double topI = prev, botI = acc;
                if (topI < botI) { const double t = topI; topI = botI; botI = t; }
                if (DEPTH <= topI + EPSILON && DEPTH >= botI - EPSILON) { layer = k; up = prev; dn = acc; break; }
            }
            if (layer == -1) ok = false;  // :609
        }
        double denom = 0.0;
        if (ok) {
            if (up < dn) { const double t = up; up = dn; dn = t; }
            denom = up - dn;
            if (fabs(denom) < 1e-30) ok = false;  // :621
        }
        if (!ok) {
            remap_set_pixel(a.img0, g, nan, nan, nan);
            if (sa.n_attr >= 1) remap_set_pixel(a.img1, g, nan, nan, nan);
            continue;
        }
        const double t = (DEPTH - dn) / denom;
        double ux, uy, uz, dx, dy, dz;
        remap_velocity<MAXV>(a, s, layer - 1, ux, uy, uz);
        remap_velocity<MAXV>(a, s, layer, dx, dy, dz);
        const double c = 1.0 - t;
        const double fx = c * dx + t * ux, fy = c * dy + t * uy, fz = c * dz + t * uz;
        double zonal, meridional;
        remap_enu(px, py, pz, fx, fy, fz, zonal, meridional);
        const double across = sa.nrm ? (fx * nx + fy * ny) + fz * nz : 0.0;
        remap_set_pixel(a.img0, g, zonal, meridional, across);
        if (sa.n_attr >= 1) {
            const double up0 = remap_attribute<MAXV>(a, s, layer - 1, a.attr0);
            const double dn0 = remap_attribute<MAXV>(a, s, layer, a.attr0);
            double v1 = 0.0;
            if (sa.n_attr >= 2) {
                const double up1 = remap_attribute<MAXV>(a, s, layer - 1, a.attr1);
                const double dn1 = remap_attribute<MAXV>(a, s, layer, a.attr1);
                v1 = c * dn1 + t * up1;
            }
            remap_set_pixel(a.img1, g, c * dn0 + t * up0, v1, 0.0);
        }
    }
}

mops_status launch_remap_section(int maxv, const SectionArgs& sa, hipStream_t s) {
    const unsigned grid = (unsigned)sa.r.W;
    return with_maxv(maxv, [&](auto MAXV) { remap_section_kernel<MAXV()><<<grid, kSectionBlock, 0, s>>>(sa); });
}

inline bool section_finite(double x) { return std::isfinite(x); }

}  // namespace

extern "C" {

mops_status mops_section_points(int32_t n_way, const double* h_waypoints, int32_t width, double* h_points,
                                double* h_normals, double* h_dist) {
    if (!h_waypoints || !h_points || !h_normals || !h_dist)
        return fail(MOPS_ERR_INVALID, "mops_section_points: null argument");
    if (n_way < 2 || width < 2) return fail(MOPS_ERR_INVALID, "mops_section_points: need two waypoints and two columns");
    const int n_leg = n_way - 1;
    std::vector<double> u(3 * (size_t)n_way), tg(3 * (size_t)n_leg), ang(n_leg), cum((size_t)n_leg + 1);
    for (int i = 0; i < n_way; ++i) {
        const double lat = h_waypoints[2 * i], lon = h_waypoints[2 * i + 1];
        if (!section_finite(lat) || !section_finite(lon) || std::fabs(lat) > 90.0)
            return fail(MOPS_ERR_INVALID, "mops_section_points: invalid waypoint");
        const double theta = lat * (M_PI / 180.0), phi = lon * (M_PI / 180.0);
        const double ct = std::cos(theta), st = std::sin(theta), cp = std::cos(phi), sp = std::sin(phi);
        u[3 * i] = ct * cp; u[3 * i + 1] = ct * sp; u[3 * i + 2] = st;
    }
    cum[0] = 0.0;
    for (int i = 0; i < n_leg; ++i) {
        const double* a = &u[3 * i];
        const double* b = a + 3;
        const double d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
        const double qx = b[0] - d * a[0], qy = b[1] - d * a[1], qz = b[2] - d * a[2];
        const double lq = std::sqrt((qx * qx + qy * qy) + qz * qz);
        ang[i] = std::atan2(lq, d);
        if (!(ang[i] >= 1e-12)) return fail(MOPS_ERR_INVALID, "mops_section_points: a leg of zero length");
        if (ang[i] > M_PI - 1e-9)
            return fail(MOPS_ERR_INVALID, "mops_section_points: a leg between antipodal waypoints");
        tg[3 * i] = qx / lq; tg[3 * i + 1] = qy / lq; tg[3 * i + 2] = qz / lq;
        cum[i + 1] = cum[i] + ang[i];
    }
    const double total = cum[n_leg];
    for (int j = 0; j < width; ++j) {
        int leg;
        double s, phi;
        if (j == 0) {
            leg = 0; s = 0.0; phi = 0.0;
        } else if (j == width - 1) {
            leg = n_leg - 1; s = total; phi = ang[leg];
        } else {
            s = (static_cast<double>(j) * total) / static_cast<double>(width - 1);
            leg = 0;
            while (leg < n_leg - 1 && s > cum[leg + 1]) ++leg;
            phi = s - cum[leg];
            if (phi > ang[leg]) phi = ang[leg];
        }
        const double* a = &u[3 * leg];
        const double* t = &tg[3 * leg];
        const double c = std::cos(phi), sn = std::sin(phi);
        const double px = c * a[0] + sn * t[0], py = c * a[1] + sn * t[1], pz = c * a[2] + sn * t[2];
        const double tx = c * t[0] - sn * a[0], ty = c * t[1] - sn * a[1], tz = c * t[2] - sn * a[2];
        h_points[3 * j] = kRemapRadius * px; h_points[3 * j + 1] = kRemapRadius * py; h_points[3 * j + 2] = kRemapRadius * pz;
        h_normals[3 * j] = py * tz - pz * ty;
        h_normals[3 * j + 1] = pz * tx - px * tz;
        h_normals[3 * j + 2] = px * ty - py * tx;
        h_dist[j] = kRemapRadius * s;
    }
    return MOPS_OK;
}

mops_status mops_remap_section(const mops_mesh* mesh, const mops_field* field, int32_t width, int32_t height,
                               double min_depth, double max_depth, const double* h_points, const double* h_normals,
                               int32_t n_attr, const double* d_attr0, const double* d_attr1, double* d_image0,
                               double* d_image1, int32_t* d_cells, void* stream) {
    if (!mesh || !field || !h_points || !d_image0) return fail(MOPS_ERR_INVALID, "mops_remap_section: null argument");
    if (width < 1 || height < 1 || (int64_t)width * height > 0x7fffffffLL)
        return fail(MOPS_ERR_INVALID, "mops_remap_section: invalid image size");
    if (n_attr < 0 || n_attr > 2) return fail(MOPS_ERR_INVALID, "mops_remap_section: n_attr must be 0..2");
    if ((n_attr >= 1 && (!d_attr0 || !d_image1)) || (n_attr >= 2 && !d_attr1))
        return fail(MOPS_ERR_INVALID, "mops_remap_section: null attribute array or image");
    if (!section_finite(min_depth) || !section_finite(max_depth))
        return fail(MOPS_ERR_INVALID, "mops_remap_section: non-finite depth range");
    if (field->mesh != mesh) return fail(MOPS_ERR_INVALID, "mops_remap_section: the field belongs to another mesh");
    if (mesh->L < 1 || mesh->L > kMaxLevels) return fail(MOPS_ERR_INVALID, "mops_remap_section: invalid level count");
    hipStream_t s = (hipStream_t)stream;
    const int W = width, H = height;
    const size_t np3 = 3 * (size_t)W;
    mops_remap_cfg cfg{};
    cfg.width = W; cfg.height = H;
    cfg.layer_rule = MOPS_LAYER_REFERENCE;
    SectionArgs sa{};
    sa.r = remap_args(mesh, field, &cfg);
    sa.r.n = (int64_t)W * H;
    sa.r.min_depth = min_depth;
    sa.r.i_step = (H > 1) ? (max_depth - min_depth) / (H - 1) : 0.0;  // :513
    sa.r.img0 = d_image0;
    sa.r.img1 = n_attr >= 1 ? d_image1 : nullptr;
    sa.r.attr0 = n_attr >= 1 ? d_attr0 : nullptr;
    sa.r.attr1 = n_attr >= 2 ? d_attr1 : nullptr;
    sa.H = H;
    sa.n_attr = n_attr;
    double* scratch = nullptr;  // points [W][3] | normals [W][3]
    int32_t* own_cells = nullptr;
    mops_status st = MOPS_OK;
    do {
        if ((st = dmalloc(&scratch, (h_normals ? 2 : 1) * np3, nullptr)) != MOPS_OK) break;
        if (!d_cells) {
            if ((st = dmalloc(&own_cells, (size_t)W, nullptr)) != MOPS_OK) break;
            d_cells = own_cells;
        }
        hipError_t e = hipMemcpyAsync(scratch, h_points, np3 * sizeof(double), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && h_normals)
            e = hipMemcpyAsync(scratch + np3, h_normals, np3 * sizeof(double), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { st = fail(MOPS_ERR_HIP, std::string("mops_remap_section: ") + hipGetErrorString(e)); break; }
        if ((st = mops_locate_cells(mesh, W, scratch, d_cells, s)) != MOPS_OK) break;
        sa.r.pts = scratch; sa.r.cells = d_cells;
        sa.nrm = h_normals ? scratch + np3 : nullptr;
        if ((st = launch_remap_section(mesh->maxv, sa, s)) != MOPS_OK) break;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { st = fail(MOPS_ERR_HIP, std::string("mops_remap_section: ") + hipGetErrorString(e)); break; }
    } while (0);
    if (st != MOPS_OK) (void)hipStreamSynchronize(s);  // the host arrays and the scratch are in flight until then
    (void)hipFree(scratch);
    (void)hipFree(own_cells);
    return st;
}

mops_status mops_section_transport(int32_t width, int32_t height, const double* h_image0, const double* h_dist,
                                   double min_depth, double max_depth, double* h_sverdrup, double* h_valid_area) {
    if (!h_image0 || !h_dist || !h_sverdrup || !h_valid_area)
        return fail(MOPS_ERR_INVALID, "mops_section_transport: null argument");
    if (width < 2 || height < 2 || (int64_t)width * height > 0x7fffffffLL)
        return fail(MOPS_ERR_INVALID, "mops_section_transport: needs at least 2 x 2 pixels");
    if (!section_finite(min_depth) || !section_finite(max_depth))
        return fail(MOPS_ERR_INVALID, "mops_section_transport: non-finite depth range");
    const int W = width, H = height;
    std::vector<double> ds(W);
    for (int j = 0; j < W; ++j) {
        const double lo = h_dist[j > 0 ? j - 1 : 0], hi = h_dist[j < W - 1 ? j + 1 : W - 1];
        ds[j] = 0.5 * (hi - lo);
    }
    const double dz = (max_depth - min_depth) / (H - 1);
    double sum = 0.0, area = 0.0;
    for (int i = 0; i < H; ++i) {
        const double dzi = (i == 0 || i == H - 1) ? 0.5 * dz : dz;
        for (int j = 0; j < W; ++j) {
            const double across = h_image0[4 * ((size_t)i * W + j) + 2];
            if (across != across) continue;
            sum += (across * ds[j]) * dzi;
            area += ds[j] * dzi;
        }
    }
    *h_sverdrup = sum / 1.0e6;
    *h_valid_area = area;
    return MOPS_OK;
}

}  // extern "C"

// ===========================================================================
// velocity gradient per cell and level (mops_velocity_gradient; no reference counterpart; the operator is
// stated in include/mops_traj.h): relative vorticity, horizontal divergence, strain rate and the Okubo-Weiss
// parameter from the Green-Gauss contour sum over a cell's vertex velocities in the cell centre's east / north
// frame.  The frame, the plane coordinates xi / eta, the contour coefficients gx / gy and the signed area A2
// depend on the cell alone, the velocities on the level, and a vertex's consecutive levels are contiguous.  So
// a group of `lpc` lanes of one wave (the smallest power of two >= L, 8 at the least, the whole wave from 33
// levels on) owns one cell: its lanes share out the cell's vertices to form xi / eta and then gx / gy into LDS,
// every lane runs the A2 sum over them, and then each lane takes levels l = ll, ll + lpc, ... and runs the
// sequential k loop of its level with the coefficients read back from LDS (every lane of a group reads the
// same word: a broadcast).  The k sums keep their stated order -- the lanes split the levels, never k -- so the
// bytes do not depend on the split.  The vertex velocities are read from the vertex array [V][L][3], a lane's
// level next to its neighbour's; after the fused derivation, which leaves that array stale, the entry first
// rebuilds it from the level-pair records (records_to_vertex_kernel, as mops_field_export does: the same
// doubles).  Reading the level-major records in place measured twice as slow as rebuilding and then reading
// (DESIGN.md section 3.22).
// ===========================================================================
namespace {

constexpr int kEddyBlock = 64;    // one wave per block
constexpr int kEddyMinLanes = 8;  // lanes per cell at the least: at most 8 cells per wave

struct EddyArgs {
    int64_t C;
    int L, rec_ints;
    int lpc;                   // lanes per cell: a power of two, kEddyMinLanes..kEddyBlock
    const int* cellrec;
    const double4* cxyz;
    const double4* vxyz;
    const double* vel;         // [V][L][3]
    double* vort;              // [C][L] each, or NULL
    double* div;
    double* strain;
    double* ow;
};

template <int MAXV>
__global__ void __launch_bounds__(kEddyBlock) velocity_gradient_kernel(EddyArgs a) {
    constexpr int kCells = kEddyBlock / kEddyMinLanes;
    __shared__ double s_xi[kCells][MAXV], s_eta[kCells][MAXV], s_gx[kCells][MAXV], s_gy[kCells][MAXV];
    __shared__ int s_vid[kCells][MAXV];
    const int lane = (int)threadIdx.x;
    const int lpc = a.lpc;
    const int sub = lane / lpc;        // the cell of this lane within the wave
    const int ll = lane - sub * lpc;   // the lane within its cell's group
    const int64_t c = (int64_t)blockIdx.x * (kEddyBlock / lpc) + sub;
    const bool live = c < a.C;
    const int L = a.L;
    int n = 0;
    double ex = 1.0, ey = 0.0, ez = 0.0, nx = 0.0, ny = 1.0, nz = 0.0;
    if (live) {
        const int* r = a.cellrec + c * a.rec_ints;
        n = r[0];
        if (n > MAXV) n = 0;  // (mops_mesh_create admits no such cell)
        const double4 q = a.cxyz[c];
        const double cx = q.x, cy = q.y, cz = q.z;
        const double Rxy = sqrt(cx * cx + cy * cy);
        if (Rxy == 0.0) {
            ny = cz > 0.0 ? 1.0 : -1.0;
        } else {
            const double Rxyz = sqrt((cx * cx + cy * cy) + cz * cz);
            const double clon = cx / Rxy, slon = cy / Rxy, slat = cz / Rxyz, clat = Rxy / Rxyz;
            ex = -slon; ey = clon; ez = 0.0;
            nx = -slat * clon; ny = -slat * slon; nz = clat;
        }
        for (int k = ll; k < n; k += lpc) {
            const int v = r[1 + k];  // 0 <= v < V for k < n (mops_mesh_create)
            const double4 p = a.vxyz[v];
            const double dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
            s_vid[sub][k] = v;
            s_xi[sub][k] = (dx * ex + dy * ey) + dz * ez;
            s_eta[sub][k] = (dx * nx + dy * ny) + dz * nz;
        }
    }
    __syncthreads();
    double A2 = 0.0;
    if (live) {
        for (int k = ll; k < n; k += lpc) {
            const int kp = k + 1 == n ? 0 : k + 1, km = k == 0 ? n - 1 : k - 1;
            s_gx[sub][k] = s_eta[sub][kp] - s_eta[sub][km];
            s_gy[sub][k] = s_xi[sub][km] - s_xi[sub][kp];
        }
        for (int k = 0; k < n; ++k) {
            const int kp = k + 1 == n ? 0 : k + 1;
            A2 += s_xi[sub][k] * s_eta[sub][kp] - s_xi[sub][kp] * s_eta[sub][k];
        }
    }
    __syncthreads();
    if (!live) return;
    const bool valid = n >= 3 && A2 != 0.0 && isfinite(A2);
    const double nan = __builtin_nan("");
    for (int l = ll; l < L; l += lpc) {
        const int64_t o = c * L + l;
        double vort = nan, dvg = nan, strain = nan, ow = nan;
        if (valid) {
            double sux = 0.0, suy = 0.0, svx = 0.0, svy = 0.0;
#pragma unroll 4
            for (int k = 0; k < n; ++k) {
                const int v = s_vid[sub][k];
                const double* p = a.vel + ((int64_t)v * L + l) * 3;
                const double Ux = p[0], Uy = p[1], Uz = p[2];
                const double u = (Ux * ex + Uy * ey) + Uz * ez;
                const double w = (Ux * nx + Uy * ny) + Uz * nz;
                const double gx = s_gx[sub][k], gy = s_gy[sub][k];
                sux += u * gx;
                suy += u * gy;
                svx += w * gx;
                svy += w * gy;
            }
            const double ux = sux / A2, uy = suy / A2, vx = svx / A2, vy = svy / A2;
            vort = vx - uy;
            dvg = ux + vy;
            const double sn = ux - vy, ss = vx + uy;
            const double s2 = sn * sn + ss * ss;
            strain = sqrt(s2);
            ow = s2 - vort * vort;
        }
        if (a.vort) a.vort[o] = vort;
        if (a.div) a.div[o] = dvg;
        if (a.strain) a.strain[o] = strain;
        if (a.ow) a.ow[o] = ow;
    }
}

mops_status launch_velocity_gradient(int maxv, const EddyArgs& a, hipStream_t s) {
    const int cells_per_block = kEddyBlock / a.lpc;
    const unsigned grid = (unsigned)((a.C + cells_per_block - 1) / cells_per_block);
    return with_maxv(maxv, [&](auto MAXV) { velocity_gradient_kernel<MAXV()><<<grid, kEddyBlock, 0, s>>>(a); });
}

}  // namespace

extern "C" {

mops_status mops_velocity_gradient(const mops_mesh* mesh, const mops_field* field, double* d_vorticity,
                                   double* d_divergence, double* d_strain, double* d_okubo_weiss, void* stream) {
    if (!mesh || !field) return fail(MOPS_ERR_INVALID, "mops_velocity_gradient: null argument");
    if (!d_vorticity && !d_divergence && !d_strain && !d_okubo_weiss)
        return fail(MOPS_ERR_INVALID, "mops_velocity_gradient: no output requested");
    if (field->mesh != mesh) return fail(MOPS_ERR_INVALID, "mops_velocity_gradient: the field belongs to another mesh");
    hipStream_t s = (hipStream_t)stream;
    EddyArgs a{};
    a.C = mesh->C; a.L = mesh->L; a.rec_ints = mesh->rec_ints;
    a.lpc = kEddyMinLanes;
    while (a.lpc < kEddyBlock && a.lpc < mesh->L) a.lpc *= 2;
    a.cellrec = mesh->d_cellrec; a.cxyz = mesh->d_cxyz; a.vxyz = mesh->d_vxyz;
    records_to_vertex(field, s);  // fused field: rebuild the vertex arrays from the records first
    a.vel = field->d_vel;
    a.vort = d_vorticity; a.div = d_divergence; a.strain = d_strain; a.ow = d_okubo_weiss;
    MOPS_TRY(launch_velocity_gradient(mesh->maxv, a, s));
    HIP_TRY(hipGetLastError());
    return MOPS_OK;
}

}  // extern "C"

// ===========================================================================
// eddy census (mops_cell_area, mops_eddy_classify, mops_label_components, mops_eddy_count, mops_eddy_table; no
// reference counterpart; stated in include/mops_traj.h): the cells whose Okubo-Weiss parameter lies below a
// threshold, split by the sign of their vorticity, grouped into the connected components of the cellsOnCell
// graph, and one table row per component.
//
// Labelling is union-find over a parent array with 32-bit atomicMin, one lane per cell.
// label[] itself is the parent array.  Invariants:
//   (a) parent[x] <= x at every instant: a cell starts as its own parent and the only concurrent write is
//       atomicMin(&parent[hi], lo) with lo < hi.  A pointer chase therefore descends strictly and ends after at
//       most x hops whatever the other lanes do; cc_find also stops at a value that breaks (a), so a corrupted
//       array ends the chase instead of extending it.
//   (b) every link joins two cells of one component of the graph: a lane only ever unites the ends of an edge of
//       equal non-zero class, or two cells already linked to them.
//   (c) no link is lost: when atomicMin finds parent[hi] == old != hi, hi stays linked to min(old, lo) and the
//       lane goes on to unite old with lo, so whatever was connected stays connected.  The pair's maximum
//       falls strictly with every turn of that loop: it ends without waiting for any other lane.
// No kernel waits on another workgroup or spins on a flag.  After the hook kernel the flatten kernel points
// every cell at its root, and the check kernel (a launch of its own, so it sees every write) raises a flag if an
// edge of equal class still has two roots or a parent is not a root; the host reads the flag and, if it is up,
// runs another round, kLabelMaxRounds at the most.  With one tree per component (b, c) and (a), the root is the
// component's smallest cell: the result is unique, so its bytes do not depend on the schedule.
// ===========================================================================
namespace {

constexpr int kLabelMaxRounds = 16;

// twice the signed area of cell c in its centre's east / north plane: velocity_gradient_kernel's frame, xi / eta
// and A2 sum restated for one lane (sharing a device function with that kernel would re-inline it there)
__global__ void __launch_bounds__(kBlock) cell_area_kernel(int64_t C, int rec_ints, int maxv, const int* cellrec,
                                                           const double4* cxyz, const double4* vxyz, double* area) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= C) return;
    const int* r = cellrec + c * rec_ints;
    int n = r[0];
    if (n > maxv) n = 0;  // (mops_mesh_create admits no such cell)
    const double4 q = cxyz[c];
    const double cx = q.x, cy = q.y, cz = q.z;
    double ex = 1.0, ey = 0.0, ez = 0.0, nx = 0.0, ny = 1.0, nz = 0.0;
    const double Rxy = sqrt(cx * cx + cy * cy);
    if (Rxy == 0.0) {
        ny = cz > 0.0 ? 1.0 : -1.0;
    } else {
        const double Rxyz = sqrt((cx * cx + cy * cy) + cz * cz);
        const double clon = cx / Rxy, slon = cy / Rxy, slat = cz / Rxyz, clat = Rxy / Rxyz;
        ex = -slon; ey = clon; ez = 0.0;
        nx = -slat * clon; ny = -slat * slon; nz = clat;
    }
    double A2 = 0.0, xi0 = 0.0, eta0 = 0.0, xik = 0.0, etak = 0.0;
    for (int k = 0; k <= n && n > 0; ++k) {  // step k forms vertex k (vertex 0 again at k == n) and adds term k-1
        double xi = xi0, eta = eta0;
        if (k < n) {
            const double4 p = vxyz[r[1 + k]];  // 0 <= r[1 + k] < V for k < n (mops_mesh_create)
            const double dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
            xi = (dx * ex + dy * ey) + dz * ez;
            eta = (dx * nx + dy * ny) + dz * nz;
        }
        if (k == 0) { xi0 = xi; eta0 = eta; }
        else A2 += xik * eta - xi * etak;
        xik = xi; etak = eta;
    }
    const bool valid = n >= 3 && A2 != 0.0 && isfinite(A2);
    area[c] = valid ? 0.5 * fabs(A2) : __builtin_nan("");
}

__global__ void __launch_bounds__(kBlock) eddy_classify_kernel(int64_t C, int L, int l, const double* ow,
                                                               const double* vort, double threshold, int* cls) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= C) return;
    const double w = ow[c * L + l], z = vort[c * L + l];
    cls[c] = w < threshold ? (z > 0.0 ? 1 : (z < 0.0 ? -1 : 0)) : 0;  // NaN compares false: class 0
}

struct LabelArgs {
    int C, rec_ints, maxv;
    const int* cellrec;
    const int* cls;
    int* parent;
    int* flag;
};

__global__ void __launch_bounds__(kBlock) label_init_kernel(int C, int* parent) {
    const int c = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (c < C) parent[c] = c;
}

// the root of x's tree: parent[] read at device scope, so a link made by another workgroup is seen; ends at the
// first value that is not a smaller valid index (invariant (a): at most x hops)
__device__ __forceinline__ int cc_find(const int* parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)p >= (unsigned)x) return x;
        x = p;
    }
}

__global__ void __launch_bounds__(kBlock) label_hook_kernel(LabelArgs a) {
    const int c = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (c >= a.C) return;
    const int k = a.cls[c];
    if (k == 0) return;
    const int* r = a.cellrec + (int64_t)c * a.rec_ints;
    int n = r[0];
    if (n > a.maxv) n = a.maxv;
    for (int j = 0; j < n; ++j) {
        const int d = r[1 + a.maxv + j];
        if ((unsigned)d >= (unsigned)a.C || d == c || a.cls[d] != k) continue;
        int x = cc_find(a.parent, c), y = cc_find(a.parent, d);
        while (x != y) {  // max(x, y) falls strictly with every turn
            const int hi = x > y ? x : y, lo = x > y ? y : x;
            const int old = atomicMin(a.parent + hi, lo);
            if (old == hi || old == lo) break;  // hi was a root and hangs under lo now, or did already
            x = cc_find(a.parent, old);         // hi hangs under min(old, lo): unite the other one with it
            y = lo;
        }
    }
}

__global__ void __launch_bounds__(kBlock) label_flatten_kernel(LabelArgs a) {
    const int c = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (c >= a.C) return;
    // a root keeps itself; any other cell is overwritten by a smaller value of its own tree (another lane that
    // reads it meanwhile sees the old or the new one: both are its ancestors; the store is atomic like the chase's
    // loads, so the two do not race).  Class 0 is never part of a chain.
    __hip_atomic_store(a.parent + c, a.cls[c] == 0 ? -1 : cc_find(a.parent, c), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kBlock) label_check_kernel(LabelArgs a) {
    const int c = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (c >= a.C) return;
    const int k = a.cls[c];
    if (k == 0) return;
    const int p = a.parent[c];
    bool bad = (unsigned)p > (unsigned)c || a.parent[p < 0 ? c : p] != p;
    const int* r = a.cellrec + (int64_t)c * a.rec_ints;
    int n = r[0];
    if (n > a.maxv) n = a.maxv;
    for (int j = 0; j < n; ++j) {
        const int d = r[1 + a.maxv + j];
        if ((unsigned)d >= (unsigned)a.C || a.cls[d] != k) continue;
        bad = bad || a.parent[d] != p;
    }
    if (bad) *a.flag = 1;
}

// before another round: class-0 cells back to their own parent (the hook kernel never reads them, the chase
// never reaches them; this keeps invariant (a) literally true)
__global__ void __launch_bounds__(kBlock) label_reopen_kernel(LabelArgs a) {
    const int c = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (c < a.C && a.cls[c] == 0) a.parent[c] = c;
}

struct EddyTableArgs {
    int E, L, l;
    const int* offs;     // [E + 1]
    const int* members;  // ascending within an eddy
    const int* cls;
    const double* area;
    const double* vort;
    const double* ow;
    const double4* cxyz;
    int* root; int* n_cells; int* polarity; int* core_cell;
    double* sum_area; double* circulation; double* ow_min; double* centre;  // centre [E][3]
};

// one lane per eddy walks its members in ascending cell order: the order fixes the bits
__global__ void __launch_bounds__(kBlock) eddy_table_kernel(EddyTableArgs a) {
    const int e = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (e >= a.E) return;
    const int b = a.offs[e], end = a.offs[e + 1];
    double A = 0.0, G = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0, wmin = INFINITY;
    int core = -1;
    for (int i = b; i < end; ++i) {
        const int c = a.members[i];
        const double ar = a.area[c];
        const int64_t o = (int64_t)c * a.L + a.l;
        const double w = a.ow[o];
        const double4 q = a.cxyz[c];
        A += ar;
        G += a.vort[o] * ar;
        Sx += ar * q.x;
        Sy += ar * q.y;
        Sz += ar * q.z;
        if (w < wmin) { wmin = w; core = c; }
    }
    const double nrm = sqrt((Sx * Sx + Sy * Sy) + Sz * Sz);
    const int first = end > b ? a.members[b] : -1;
    a.root[e] = first;
    a.n_cells[e] = end - b;
    a.polarity[e] = first >= 0 ? a.cls[first] : 0;
    a.core_cell[e] = core;
    a.sum_area[e] = A;
    a.circulation[e] = G;
    a.ow_min[e] = wmin;
    a.centre[3 * e] = Sx / nrm;
    a.centre[3 * e + 1] = Sy / nrm;
    a.centre[3 * e + 2] = Sz / nrm;
}

struct DevBuf {  // a temporary device allocation of one call
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace

extern "C" {

mops_status mops_cell_area(const mops_mesh* mesh, double* d_area, void* stream) {
    if (!mesh || !d_area) return fail(MOPS_ERR_INVALID, "mops_cell_area: null argument");
    hipStream_t s = (hipStream_t)stream;
    cell_area_kernel<<<grid_for(mesh->C), kBlock, 0, s>>>(mesh->C, mesh->rec_ints, mesh->maxv, mesh->d_cellrec,
                                                          mesh->d_cxyz, mesh->d_vxyz, d_area);
    HIP_TRY(hipGetLastError());
    return MOPS_OK;
}

mops_status mops_eddy_classify(const mops_mesh* mesh, const double* d_okubo_weiss, const double* d_vorticity,
                               int32_t level, double threshold, int32_t* d_class, void* stream) {
    if (!mesh || !d_okubo_weiss || !d_vorticity || !d_class)
        return fail(MOPS_ERR_INVALID, "mops_eddy_classify: null argument");
    if (level < 0 || level >= mesh->L) return fail(MOPS_ERR_INVALID, "mops_eddy_classify: level outside the levels");
    hipStream_t s = (hipStream_t)stream;
    eddy_classify_kernel<<<grid_for(mesh->C), kBlock, 0, s>>>(mesh->C, mesh->L, level, d_okubo_weiss, d_vorticity,
                                                              threshold, d_class);
    HIP_TRY(hipGetLastError());
    return MOPS_OK;
}

mops_status mops_label_components(const mops_mesh* mesh, const int32_t* d_class, int32_t* d_label, int32_t* h_rounds,
                                  void* stream) {
    if (!mesh || !d_class || !d_label) return fail(MOPS_ERR_INVALID, "mops_label_components: null argument");
    if (h_rounds) *h_rounds = 0;
    hipStream_t s = (hipStream_t)stream;
    DevBuf flag;
    HIP_TRY(flag.alloc(sizeof(int)));
    LabelArgs a{};
    a.C = (int)mesh->C; a.rec_ints = mesh->rec_ints; a.maxv = mesh->maxv;  // C <= 2^30 (mops_mesh_create)
    a.cellrec = mesh->d_cellrec; a.cls = d_class; a.parent = d_label; a.flag = flag.as<int>();
    const unsigned grid = grid_for(mesh->C);
    if (grid == 0) return MOPS_OK;
    label_init_kernel<<<grid, kBlock, 0, s>>>(a.C, a.parent);
    HIP_TRY(hipGetLastError());
    // By invariant (c) the hook kernel leaves one tree per component, so round 1's check finds nothing and the
    // entry returns there: rounds 2 .. kLabelMaxRounds and label_reopen_kernel are a safety net that no correct
    // run, and therefore no test, reaches.  They turn a defect in the hook kernel into more work or an error.
    for (int round = 1; round <= kLabelMaxRounds; ++round) {
        HIP_TRY(hipMemsetAsync(a.flag, 0, sizeof(int), s));
        label_hook_kernel<<<grid, kBlock, 0, s>>>(a);
        label_flatten_kernel<<<grid, kBlock, 0, s>>>(a);
        label_check_kernel<<<grid, kBlock, 0, s>>>(a);
        HIP_TRY(hipGetLastError());
        int h_flag = 0;
        HIP_TRY(hipMemcpyAsync(&h_flag, a.flag, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h_rounds) *h_rounds = round;
        if (!h_flag) return MOPS_OK;
        label_reopen_kernel<<<grid, kBlock, 0, s>>>(a);
    }
    HIP_TRY(hipStreamSynchronize(s));
    return fail(MOPS_ERR_UNSUPPORTED, "mops_label_components: not converged after " +
                                          std::to_string(kLabelMaxRounds) + " rounds");
}

mops_status mops_eddy_count(const mops_mesh* mesh, const int32_t* d_label, int32_t min_cells, int32_t* d_eddy_of_cell,
                            int64_t* h_n_eddies, void* stream) {
    if (!mesh || !d_label || !d_eddy_of_cell || !h_n_eddies)
        return fail(MOPS_ERR_INVALID, "mops_eddy_count: null argument");
    if (min_cells < 1) return fail(MOPS_ERR_INVALID, "mops_eddy_count: min_cells < 1");
    hipStream_t s = (hipStream_t)stream;
    const int64_t C = mesh->C;
    std::vector<int32_t> lab((size_t)C), cnt((size_t)C, 0);
    HIP_TRY(hipMemcpyAsync(lab.data(), d_label, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t c = 0; c < C; ++c) {
        const int32_t r = lab[c];
        if (r < -1 || r > c || (r >= 0 && lab[r] != r))
            return fail(MOPS_ERR_INVALID, "mops_eddy_count: not a label array (a label is -1 or a root cell <= its cell)");
        if (r >= 0) ++cnt[r];
    }
    int64_t E = 0;
    for (int64_t c = 0; c < C; ++c)  // cnt becomes the eddy index of a root, ascending by root
        cnt[c] = (lab[c] == c && cnt[c] >= min_cells) ? (int32_t)E++ : -1;
    for (int64_t c = 0; c < C; ++c) lab[c] = lab[c] >= 0 ? cnt[lab[c]] : -1;
    HIP_TRY(hipMemcpyAsync(d_eddy_of_cell, lab.data(), (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // lab leaves scope
    *h_n_eddies = E;
    return MOPS_OK;
}

mops_status mops_eddy_table(const mops_mesh* mesh, const int32_t* d_eddy_of_cell, int64_t n_eddies,
                            const int32_t* d_class, const double* d_area, const double* d_vorticity,
                            const double* d_okubo_weiss, int32_t level, int32_t* h_root, int32_t* h_n_cells,
                            int32_t* h_polarity, int32_t* h_core_cell, double* h_area, double* h_circulation,
                            double* h_ow_min, double* h_centre, void* stream) {
    if (!mesh || !d_eddy_of_cell || !d_class || !d_area || !d_vorticity || !d_okubo_weiss)
        return fail(MOPS_ERR_INVALID, "mops_eddy_table: null argument");
    if (level < 0 || level >= mesh->L) return fail(MOPS_ERR_INVALID, "mops_eddy_table: level outside the levels");
    if (n_eddies < 0 || n_eddies > mesh->C) return fail(MOPS_ERR_INVALID, "mops_eddy_table: n_eddies out of range");
    if (n_eddies == 0) return MOPS_OK;
    if (!h_root || !h_n_cells || !h_polarity || !h_core_cell || !h_area || !h_circulation || !h_ow_min || !h_centre)
        return fail(MOPS_ERR_INVALID, "mops_eddy_table: null output");
    hipStream_t s = (hipStream_t)stream;
    const int64_t C = mesh->C;
    const int E = (int)n_eddies;
    std::vector<int32_t> eoc((size_t)C), offs((size_t)E + 1, 0);
    HIP_TRY(hipMemcpyAsync(eoc.data(), d_eddy_of_cell, (size_t)C * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t c = 0; c < C; ++c) {
        if (eoc[c] < -1 || eoc[c] >= E) return fail(MOPS_ERR_INVALID, "mops_eddy_table: eddy index out of range");
        if (eoc[c] >= 0) ++offs[eoc[c] + 1];
    }
    for (int e = 0; e < E; ++e) offs[e + 1] += offs[e];
    std::vector<int32_t> members((size_t)offs[E]), fill(offs.begin(), offs.end() - 1);
    for (int64_t c = 0; c < C; ++c)  // ascending c: every eddy's members come out in ascending cell order
        if (eoc[c] >= 0) members[fill[eoc[c]]++] = (int32_t)c;
    DevBuf d_offs, d_mem, d_int, d_dbl;
    HIP_TRY(d_offs.alloc(offs.size() * sizeof(int32_t)));
    HIP_TRY(d_mem.alloc(members.size() * sizeof(int32_t)));
    HIP_TRY(d_int.alloc((size_t)E * 4 * sizeof(int32_t)));
    HIP_TRY(d_dbl.alloc((size_t)E * 6 * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(d_offs.p, offs.data(), offs.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_mem.p, members.data(), members.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    EddyTableArgs a{};
    a.E = E; a.L = mesh->L; a.l = level;
    a.offs = d_offs.as<int>(); a.members = d_mem.as<int>();
    a.cls = d_class; a.area = d_area; a.vort = d_vorticity; a.ow = d_okubo_weiss; a.cxyz = mesh->d_cxyz;
    a.root = d_int.as<int>(); a.n_cells = a.root + E; a.polarity = a.root + 2 * (size_t)E;
    a.core_cell = a.root + 3 * (size_t)E;
    a.sum_area = d_dbl.as<double>(); a.circulation = a.sum_area + E; a.ow_min = a.sum_area + 2 * (size_t)E;
    a.centre = a.sum_area + 3 * (size_t)E;
    eddy_table_kernel<<<grid_for(E), kBlock, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    const size_t ib = (size_t)E * sizeof(int32_t), db = (size_t)E * sizeof(double);
    HIP_TRY(hipMemcpyAsync(h_root, a.root, ib, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_n_cells, a.n_cells, ib, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_polarity, a.polarity, ib, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_core_cell, a.core_cell, ib, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_area, a.sum_area, db, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_circulation, a.circulation, db, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_ow_min, a.ow_min, db, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_centre, a.centre, 3 * db, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MOPS_OK;
}

}  // extern "C"

// ===========================================================================
// colour mapping: MOPS::SaveToPNG's pixel work (src/Common/ImageBuffer.hpp:91-136) for an [H][W][4]
// float64 device image, channels together.  Two passes over the image: the float range of every channel
// (per-block partials, then one block reduces them -- min / max do not depend on the order, so no atomics and
// no hand-off between workgroups are needed), then tinycolormap's Viridis lerp (tinycolormap.hpp:162-171) per
// pixel and selected channel, one uchar4 store per plane.  The table (include/mops_viridis.h, generated from
// matplotlib's published Viridis samples) is staged in LDS: the per-lane index is data dependent.
//
// Infinities: an infinite pixel makes max - min infinite or NaN, and the reference then indexes its table
// with static_cast<size_t>(NaN), which is undefined.  Here a NaN `norm` takes table entry 0.
// ===========================================================================
#include "mops_viridis.h"

namespace {

constexpr int kCmapMaxBlocks = 1024;  // range-pass grid cap: 4 blocks of 256 lanes per CU on 256 CUs

__device__ __forceinline__ void cmap_acc(float& mn, float& mx, double v) {
    const float f = static_cast<float>(v);  // :105
    if (!(f != f)) {                        // :106
        mn = f < mn ? f : mn;               // std::min / std::max (:107-108)
        mx = mx < f ? f : mx;
    }
}

// per block and channel {min, max} of the non-NaN float values -> partial [gridDim.x][4][2].  The values are
// order independent; only the sign of a zero minimum or maximum may differ from the reference's, and it
// reaches no colour: x - (+0) and x - (-0) differ for no x but -0, whose norm is a zero of either sign.
__global__ void __launch_bounds__(256) colormap_range_kernel(int64_t n, const double2* __restrict__ img,
                                                             float* __restrict__ partial) {
    __shared__ float red[4][8];  // [wave][channel * 2 + {min, max}]
    float mn[4], mx[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { mn[c] = FLT_MAX; mx[c] = -FLT_MAX; }  // :101-102
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
        const double2 xy = img[2 * g], za = img[2 * g + 1];  // the 32-B pixel as two 16-B loads
        cmap_acc(mn[0], mx[0], xy.x);
        cmap_acc(mn[1], mx[1], xy.y);
        cmap_acc(mn[2], mx[2], za.x);
        cmap_acc(mn[3], mx[3], za.y);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], off, 64));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], off, 64));
        }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) { red[wave][2 * c] = mn[c]; red[wave][2 * c + 1] = mx[c]; }
    __syncthreads();
    if (threadIdx.x < 8) {
        const bool is_max = threadIdx.x & 1;
        float r = red[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) r = is_max ? fmaxf(r, red[w][threadIdx.x]) : fminf(r, red[w][threadIdx.x]);
        partial[(int64_t)blockIdx.x * 8 + threadIdx.x] = r;
    }
}

// one block: partial [n_blocks][4][2] -> minmax [4][2], with `if (min >= max) max = min + 1e-5f` (:111)
__global__ void __launch_bounds__(256) colormap_reduce_kernel(int n_blocks, const float* __restrict__ partial,
                                                              float* __restrict__ minmax) {
    __shared__ float red[256];
    const int k = threadIdx.x & 7;  // channel * 2 + {min, max}
    const bool is_max = k & 1;
    float r = is_max ? -FLT_MAX : FLT_MAX;
    for (int b = threadIdx.x >> 3; b < n_blocks; b += 32) {
        const float v = partial[(int64_t)b * 8 + k];
        r = is_max ? fmaxf(r, v) : fminf(r, v);
    }
    red[threadIdx.x] = r;
    __syncthreads();
    if (threadIdx.x < 8) {
        for (int j = 1; j < 32; ++j) {
            const float v = red[j * 8 + k];
            r = is_max ? fmaxf(r, v) : fminf(r, v);
        }
        red[threadIdx.x] = r;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const float minVal = red[2 * threadIdx.x];
        float maxVal = red[2 * threadIdx.x + 1];
        if (minVal >= maxVal) maxVal = minVal + 1e-5f;
        minmax[2 * threadIdx.x] = minVal;
        minmax[2 * threadIdx.x + 1] = maxVal;
    }
}

// :115-132 for one value: norm in float, tinycolormap::GetViridisColor in double, truncation to bytes
__device__ __forceinline__ uchar4 cmap_pixel(double v, float minVal, float maxVal, const double (*T)[3]) {
    const float raw_val = static_cast<float>(v);
    if (raw_val != raw_val) return make_uchar4(0, 0, 0, 0);
    const float norm_val = (raw_val - minVal) / (maxVal - minVal);
    const double x = norm_val;
    double cl = (x < 0.0) ? 0.0 : (x > 1.0) ? 1.0 : x;  // Clamp01
    if (cl != cl) cl = 0.0;                              // NaN norm: entry 0 (see the section comment)
    const double a = cl * (MOPS_VIRIDIS_N - 1);
    const double i = floor(a);
    const double t = a - i;
    const int i0 = (int)i, i1 = (int)ceil(a);
    const double u = 1.0 - t;
    const double r = u * T[i0][0] + t * T[i1][0];
    const double g = u * T[i0][1] + t * T[i1][1];
    const double b = u * T[i0][2] + t * T[i1][2];
    return make_uchar4((unsigned char)(r * 255.0), (unsigned char)(g * 255.0), (unsigned char)(b * 255.0), 255);
}

__global__ void __launch_bounds__(256) colormap_map_kernel(int64_t n, const double2* __restrict__ img,
                                                           const double* __restrict__ table,
                                                           const float* __restrict__ minmax, int mask,
                                                           uchar4* __restrict__ out) {
    __shared__ double T[MOPS_VIRIDIS_N][3];
    for (int k = threadIdx.x; k < MOPS_VIRIDIS_N * 3; k += blockDim.x) (&T[0][0])[k] = table[k];
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const double2 xy = img[2 * g], za = img[2 * g + 1];
    const double v[4] = {xy.x, xy.y, za.x, za.y};
    int plane = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (mask & (1 << c)) {
            out[(int64_t)plane * n + g] = cmap_pixel(v[c], minmax[2 * c], minmax[2 * c + 1], T);
            ++plane;
        }
}

std::mutex g_cmap_mutex;
double* g_cmap_table[64] = {};  // the table in HBM, per device, uploaded on first use (6 KB, kept)

mops_status cmap_table(const double** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(MOPS_ERR_UNSUPPORTED, "mops_colormap_rgba8: device index above 63");
    std::lock_guard<std::mutex> lock(g_cmap_mutex);
    if (!g_cmap_table[dev]) {
        double* p = nullptr;
        HIP_TRY(hipMalloc(&p, sizeof(MOPS_VIRIDIS_TABLE)));
        hipError_t e = hipMemcpy(p, MOPS_VIRIDIS_TABLE, sizeof(MOPS_VIRIDIS_TABLE), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return fail(MOPS_ERR_HIP, std::string("mops_colormap_rgba8: ") + hipGetErrorString(e));
        }
        g_cmap_table[dev] = p;
    }
    *out = g_cmap_table[dev];
    return MOPS_OK;
}

}  // namespace

extern "C" {

mops_status mops_colormap_rgba8(const double* d_image, int32_t width, int32_t height, int32_t channel_mask,
                                uint8_t* d_rgba, float* h_minmax, void* stream) {
    if (!d_image || !d_rgba || width <= 0 || height <= 0 || (int64_t)width * height > 0x7fffffffLL ||
        channel_mask <= 0 || channel_mask > 15)
        return fail(MOPS_ERR_INVALID, "mops_colormap_rgba8: invalid argument");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)width * height;
    // at least four grid-stride rounds per lane where the image allows it, so few partials are left to reduce
    const int n_blocks = (int)std::min<int64_t>((n + 4 * 256 - 1) / (4 * 256), kCmapMaxBlocks);
    const double* table = nullptr;
    MOPS_TRY(cmap_table(&table));
    float* scratch = nullptr;  // partial [n_blocks][4][2] | minmax [4][2]
    MOPS_TRY(dmalloc(&scratch, (size_t)n_blocks * 8 + 8, nullptr));
    float* minmax = scratch + (size_t)n_blocks * 8;
    colormap_range_kernel<<<n_blocks, 256, 0, s>>>(n, (const double2*)d_image, scratch);
    colormap_reduce_kernel<<<1, 256, 0, s>>>(n_blocks, scratch, minmax);
    colormap_map_kernel<<<grid_for(n), 256, 0, s>>>(n, (const double2*)d_image, table, minmax, channel_mask,
                                                    (uchar4*)d_rgba);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && h_minmax) e = hipMemcpyAsync(h_minmax, minmax, 8 * sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    if (e != hipSuccess) return fail(MOPS_ERR_HIP, std::string("mops_colormap_rgba8: ") + hipGetErrorString(e));
    return MOPS_OK;
}

mops_status mops_colormap_image(const double* h_image, int32_t width, int32_t height, int32_t channel_mask,
                                uint8_t* h_rgba, float* h_minmax, void* stream) {
    if (!h_image || !h_rgba || width <= 0 || height <= 0 || (int64_t)width * height > 0x7fffffffLL ||
        channel_mask <= 0 || channel_mask > 15)
        return fail(MOPS_ERR_INVALID, "mops_colormap_image: invalid argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)width * height;
    const size_t planes = (size_t)__builtin_popcount((unsigned)channel_mask);
    double* d_image = nullptr;
    uint8_t* d_rgba = nullptr;
    mops_status st = MOPS_OK;
    do {
        if ((st = dmalloc(&d_image, n * 4, nullptr)) != MOPS_OK) break;
        if ((st = dmalloc(&d_rgba, planes * n * 4, nullptr)) != MOPS_OK) break;
        hipError_t e = hipMemcpyAsync(d_image, h_image, n * 4 * sizeof(double), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { st = fail(MOPS_ERR_HIP, std::string("mops_colormap_image: ") + hipGetErrorString(e)); break; }
        if ((st = mops_colormap_rgba8(d_image, width, height, channel_mask, d_rgba, h_minmax, stream)) != MOPS_OK) break;
        e = hipMemcpyAsync(h_rgba, d_rgba, planes * n * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) st = fail(MOPS_ERR_HIP, std::string("mops_colormap_image: ") + hipGetErrorString(e));
    } while (0);
    (void)hipFree(d_image);
    (void)hipFree(d_rgba);
    return st;
}

}  // extern "C"

// ===========================================================================
// particle density maps: record points -> {count, fixed-point value sum} per lat / lon pixel (mops_traj.h;
// DESIGN.md section 3.16).  One lane per particle walks its records in k.  A particle moves a fraction of a
// pixel per record, so consecutive records of a lane mostly share a pixel: the lane keeps {pixel, count, qsum}
// in registers and touches the accumulator only when the pixel changes (and once at the end).  The sums are
// integers, so neither this run-length merge nor the order of the atomics changes a byte of the result.
// Self-contained on purpose: no dev:: helper is instantiated here, so the trajectory kernels' code stays as
// it is.
// ===========================================================================
namespace {

struct DensityArgs {
    int64_t n, k_begin, k_end;
    const double* pts;
    int64_t sk, si, sc;
    const double* seeds;  // [n][3] or null
    int kind;
    const double* vals;
    int64_t vk, vi;
    unsigned long long* acc;  // [H][W][2]
    int W, H;
    double min_lat, max_lat, min_lon, max_lon;
};

// the pixel of a point, or -1 where the point is skipped or outside the window
__device__ __forceinline__ int density_pixel(const DensityArgs& a, double x, double y, double z) {
    const double r = sqrt(x * x + y * y + z * z);
    if (!(isfinite(x) && isfinite(y) && isfinite(z)) || r == 0.0) return -1;
    double s = z / r;
    s = s < -1.0 ? -1.0 : (s > 1.0 ? 1.0 : s);
    const double lat = asin(s) * (180.0 / M_PI);
    double lon = atan2(y, x) * (180.0 / M_PI);
    lon -= 360.0 * floor((lon - a.min_lon) / 360.0);
    const double fr = (a.max_lat - lat) / (a.max_lat - a.min_lat) * (double)a.H;
    const double fc = (lon - a.min_lon) / (a.max_lon - a.min_lon) * (double)a.W;
    if (!(fr >= 0.0 && fr < (double)a.H && fc >= 0.0 && fc < (double)a.W)) return -1;
    return (int)floor(fr) * a.W + (int)floor(fc);
}

// q = llrint(v * 2^24) of a usable value; false where the value skips its point
__device__ __forceinline__ bool density_quantise(double v, long long& q) {
    if (!isfinite(v) || !(fabs(v) < 274877906944.0)) return false;  // 2^38
    q = (long long)rint(v * 16777216.0);                             // ties to even (the default rounding mode)
    return true;
}

// The second lever the data offers -- merging equal pixels across a wave's lanes before the atomic (a leader
// loop: ballot, the first lane's pixel, a wave reduction of its group) -- was built and measured: 4.77 ms against
// 2.90 ms for a COUNT map of one config-3 pair, because at 3601 x 1801 neighbouring lanes rarely share a pixel and
// every flush pays for the loop.  It is not kept.

// SLAB: the record slab's si == 1 known at compile time, so a wave's loads of one component are one run of
// consecutive doubles whatever the compiler makes of the generic stride
template <bool SLAB>
__global__ void __launch_bounds__(256) density_accumulate_kernel(DensityArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int64_t si = SLAB ? 1 : a.si;
    const double* p = a.pts + i * si;
    const double* val = a.kind == MOPS_DENSITY_VALUES ? a.vals + i * a.vi : nullptr;
    int pix = -1;
    unsigned long long cnt = 0, qs = 0;
    auto flush = [&]() {
        if (cnt == 0) return;
        atomicAdd(&a.acc[2 * (int64_t)pix], cnt);
        if (a.kind != MOPS_DENSITY_COUNT) atomicAdd(&a.acc[2 * (int64_t)pix + 1], qs);  // (wraps as the signed sum)
    };
    auto add = [&](int px, long long q) {
        if (px != pix) {
            flush();
            pix = px; cnt = 0; qs = 0;
        }
        cnt += 1;
        qs += (unsigned long long)q;
    };
    if (a.seeds && a.kind == MOPS_DENSITY_COUNT) {
        const int px = density_pixel(a, a.seeds[3 * i], a.seeds[3 * i + 1], a.seeds[3 * i + 2]);
        if (px >= 0) add(px, 0);
    }
    for (int64_t k = a.k_begin; k < a.k_end; ++k) {
        const double* pk = p + k * a.sk;
        const int px = density_pixel(a, pk[0], pk[a.sc], pk[2 * a.sc]);
        if (px < 0) continue;
        long long q = 0;
        if (a.kind == MOPS_DENSITY_SPEED) {
            const double vx = pk[3 * a.sc], vy = pk[4 * a.sc], vz = pk[5 * a.sc];
            if (!density_quantise(sqrt(vx * vx + vy * vy + vz * vz), q)) continue;
        } else if (a.kind == MOPS_DENSITY_VALUES) {
            if (!density_quantise(val[k * a.vk], q)) continue;
        }
        add(px, q);
    }
    flush();
}

__global__ void __launch_bounds__(256) density_image_kernel(int64_t n, const long long* __restrict__ acc,
                                                            int nan_empty, double2* __restrict__ img) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const long long cnt = acc[2 * g], qs = acc[2 * g + 1];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double2 xy, za;
    za.y = 1.0;
    if (cnt == 0) {
        xy.x = nan_empty ? nan : 0.0;
        xy.y = nan;
        za.x = nan_empty ? nan : 0.0;
    } else {
        const double sum = (double)qs / 16777216.0;
        xy.x = (double)cnt;
        xy.y = sum / (double)cnt;
        za.x = sum;
    }
    img[2 * g] = xy;
    img[2 * g + 1] = za;
}

mops_status density_check(const char* what, const mops_remap_cfg* cfg, const void* a, const void* b) {
    if (!cfg || !a || !b) return fail(MOPS_ERR_INVALID, std::string(what) + ": null argument");
    if (cfg->width < 1 || cfg->height < 1 || (int64_t)cfg->width * cfg->height >= (1LL << 31))
        return fail(MOPS_ERR_INVALID, std::string(what) + ": invalid image size");
    if (!std::isfinite(cfg->min_lat) || !std::isfinite(cfg->max_lat) || !std::isfinite(cfg->min_lon) ||
        !std::isfinite(cfg->max_lon) || !(cfg->max_lat > cfg->min_lat) || !(cfg->max_lon > cfg->min_lon) ||
        !std::isfinite(cfg->max_lat - cfg->min_lat) || cfg->max_lon - cfg->min_lon > 360.0)
        return fail(MOPS_ERR_INVALID, std::string(what) + ": invalid latitude / longitude range");
    return MOPS_OK;
}

}  // namespace

extern "C" {

int64_t mops_density_bytes(int32_t width, int32_t height) {
    if (width < 1 || height < 1 || (int64_t)width * height >= (1LL << 31)) return -1;
    return (int64_t)width * height * 16;
}

mops_status mops_density_accumulate(const mops_remap_cfg* cfg, int64_t n, int64_t k_begin, int64_t k_end,
                                    const double* d_points, int64_t sk, int64_t si, int64_t sc,
                                    const double* d_seeds, int32_t value_kind, const double* d_values, int64_t vk,
                                    int64_t vi, void* d_accum, void* stream) {
    MOPS_TRY(density_check("mops_density_accumulate", cfg, d_points, d_accum));
    if (n < 0 || k_begin < 0) return fail(MOPS_ERR_INVALID, "mops_density_accumulate: negative count or range");
    if (value_kind != MOPS_DENSITY_COUNT && value_kind != MOPS_DENSITY_SPEED && value_kind != MOPS_DENSITY_VALUES)
        return fail(MOPS_ERR_INVALID, "mops_density_accumulate: invalid value kind");
    if (value_kind == MOPS_DENSITY_VALUES && !d_values)
        return fail(MOPS_ERR_INVALID, "mops_density_accumulate: MOPS_DENSITY_VALUES without d_values");
    if (n == 0 || k_end <= k_begin) return MOPS_OK;
    if (n > (int64_t)0x7fffffff * 256) return fail(MOPS_ERR_INVALID, "mops_density_accumulate: too many particles");
    DensityArgs a;
    a.n = n; a.k_begin = k_begin; a.k_end = k_end;
    a.pts = d_points; a.sk = sk; a.si = si; a.sc = sc;
    a.seeds = d_seeds;
    a.kind = value_kind;
    a.vals = d_values; a.vk = vk; a.vi = vi;
    a.acc = (unsigned long long*)d_accum;
    a.W = cfg->width; a.H = cfg->height;
    a.min_lat = cfg->min_lat; a.max_lat = cfg->max_lat; a.min_lon = cfg->min_lon; a.max_lon = cfg->max_lon;
    hipStream_t s = (hipStream_t)stream;
    if (si == 1) density_accumulate_kernel<true><<<grid_for(n), 256, 0, s>>>(a);
    else density_accumulate_kernel<false><<<grid_for(n), 256, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return MOPS_OK;
}

mops_status mops_density_image(const mops_remap_cfg* cfg, const void* d_accum, int32_t nan_empty, double* d_image,
                               void* stream) {
    MOPS_TRY(density_check("mops_density_image", cfg, d_accum, d_image));
    const int64_t n = (int64_t)cfg->width * cfg->height;
    density_image_kernel<<<grid_for(n), 256, 0, (hipStream_t)stream>>>(n, (const long long*)d_accum, nan_empty,
                                                                       (double2*)d_image);
    HIP_TRY(hipGetLastError());
    return MOPS_OK;
}

}  // extern "C"

// ===========================================================================
// flow-map lattices and FTLE (mops_traj.h).  The lattice is the fixed-depth remapping's
// pixel positions (remap_positions_kernel on the remap_depth_tables tables), so seed (i, j) has the bits of the
// remapped image's pixel (i, j).  ftle_kernel: one lane per pixel, a five-point stencil over the unit seeds and
// unit last points (normalised once per block into an LDS tile) with one-sided differences where a neighbour is
// missing, the Cauchy-Green tensor's two eigenvalues in closed form.  FP64 + - * / sqrt up to lambda, so the restatement in tests/ftle_reference.py
// reproduces channels 1 and 2 byte for byte; the one libm call is the log of channel 0.
// Self-contained on purpose, as the density kernels: no dev:: helper is instantiated here.
// ===========================================================================
namespace {

struct FtleArgs {
    int64_t n;
    int W, H;
    const double* seeds;   // [n][3]
    const double* last;    // [n][3]
    const int32_t* death;  // [n] or null
    double two_h;          // 2 * horizon
    int wrap;
    double2* img;          // [n][4]
};

// p / |p|, or false for a non-finite or zero-length p
__device__ __forceinline__ bool ftle_unit(const double* __restrict__ p, double& ox, double& oy, double& oz) {
    const double x = p[0], y = p[1], z = p[2];
    const double r = sqrt((x * x + y * y) + z * z);
    if (!(isfinite(x) && isfinite(y) && isfinite(z)) || r == 0.0) return false;
    ox = x / r; oy = y / r; oz = z / r;
    return true;
}

struct FtlePoint {
    double sx, sy, sz, ux, uy, uz;
};

// the unit seed and unit last point of particle g, or false where it is not valid
__device__ __forceinline__ bool ftle_point(const FtleArgs& a, int64_t g, FtlePoint& p) {
    if (a.death && a.death[g] >= 0) return false;
    return ftle_unit(a.seeds + 3 * g, p.sx, p.sy, p.sz) && ftle_unit(a.last + 3 * g, p.ux, p.uy, p.uz);
}

// the pair (minus side, plus side) of one direction: d = (u_p - u_m) / |s_p - s_m|; false for a zero spacing
__device__ __forceinline__ bool ftle_diff(const FtlePoint& m, const FtlePoint& p, double& dx, double& dy,
                                          double& dz) {
    const double hx = p.sx - m.sx, hy = p.sy - m.sy, hz = p.sz - m.sz;
    const double h = sqrt((hx * hx + hy * hy) + hz * hz);
    if (h == 0.0) return false;
    dx = (p.ux - m.ux) / h; dy = (p.uy - m.uy) / h; dz = (p.uz - m.uz) / h;
    return true;
}

// A block is a tile of 32 x 8 pixels.  Its 34 x 10 points (the tile and a halo of one) are normalised once into
// LDS -- {s, u} as six planes and a validity byte, 16.7 KB -- then every lane reads its stencil from there: 1.33
// normalisations (an FP64 sqrt and three correctly rounded divisions each, twice) per pixel instead of the five of
// a lane that does its own neighbours.  That form was built first and measured: 0.295 ms against this one's
// 0.152 ms at 3601 x 1801, the same bytes.  The source keeps this comment, not the code.
constexpr int kFtleTx = 32, kFtleTy = 8, kFtleHx = kFtleTx + 2, kFtleHy = kFtleTy + 2, kFtleHn = kFtleHx * kFtleHy;

__global__ void __launch_bounds__(256) ftle_kernel(FtleArgs a, int tiles_x) {
    __shared__ double lds[6][kFtleHn];
    __shared__ unsigned char okp[kFtleHn];
    const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x % (unsigned)tiles_x);
    const int i0 = tile_y * kFtleTy - 1, j0 = tile_x * kFtleTx - 1;
    for (int k = threadIdx.x; k < kFtleHn; k += 256) {
        const int hy = k / kFtleHx, hx = k - hy * kFtleHx;
        const int i = i0 + hy;
        int j = j0 + hx;
        if (a.wrap) j = j == -1 ? a.W - 1 : (j == a.W ? 0 : j);
        bool ok = i >= 0 && i < a.H && j >= 0 && j < a.W;
        FtlePoint p;
        if (ok) ok = ftle_point(a, (int64_t)i * a.W + j, p);
        okp[k] = ok;
        if (ok) {
            lds[0][k] = p.sx; lds[1][k] = p.sy; lds[2][k] = p.sz;
            lds[3][k] = p.ux; lds[4][k] = p.uy; lds[5][k] = p.uz;
        }
    }
    __syncthreads();
    const int ly = threadIdx.x / kFtleTx, lx = threadIdx.x % kFtleTx;
    const int i = i0 + 1 + ly, j = j0 + 1 + lx;
    if (i >= a.H || j >= a.W) return;
    const int64_t g = (int64_t)i * a.W + j;
    const int kc = (ly + 1) * kFtleHx + lx + 1;
    auto get = [&](int k) {
        FtlePoint p;
        p.sx = lds[0][k]; p.sy = lds[1][k]; p.sz = lds[2][k];
        p.ux = lds[3][k]; p.uy = lds[4][k]; p.uz = lds[5][k];
        return p;
    };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double2 xy, za;
    xy.x = nan; xy.y = nan; za.x = nan; za.y = 1.0;
    const bool okl = okp[kc - 1], okr = okp[kc + 1], oku = okp[kc - kFtleHx], okd = okp[kc + kFtleHx];
    // jm == jp: both sides missing, or (with wrap) both the same column
    bool ok = okp[kc] && (okl || okr) && (oku || okd) && !(a.wrap && a.W <= 2);
    if (ok) {
        const FtlePoint em = get(okl ? kc - 1 : kc), ep = get(okr ? kc + 1 : kc);
        const FtlePoint nm = get(oku ? kc - kFtleHx : kc), np = get(okd ? kc + kFtleHx : kc);
        double ax, ay, az, bx, by, bz;
        ok = ftle_diff(em, ep, ax, ay, az) && ftle_diff(np, nm, bx, by, bz);
        if (ok) {
            const double c11 = (ax * ax + ay * ay) + az * az;
            const double c12 = (ax * bx + ay * by) + az * bz;
            const double c22 = (bx * bx + by * by) + bz * bz;
            const double m = 0.5 * (c11 + c22), d = 0.5 * (c11 - c22);
            const double q = sqrt(d * d + c12 * c12);
            const double lmax = m + q, lmin = m - q;
            xy.x = log(lmax) / a.two_h;
            xy.y = lmax;
            za.x = lmin;
        }
    }
    a.img[2 * g] = xy;
    a.img[2 * g + 1] = za;
}

mops_status lattice_check(const char* what, const mops_remap_cfg* cfg) {
    if (!cfg) return fail(MOPS_ERR_INVALID, std::string(what) + ": null argument");
    if (cfg->width < 1 || cfg->height < 1 || (int64_t)cfg->width * cfg->height >= (1LL << 31))
        return fail(MOPS_ERR_INVALID, std::string(what) + ": invalid image size");
    return MOPS_OK;
}

}  // namespace

extern "C" {

mops_status mops_flowmap_lattice(const mops_remap_cfg* cfg, double* d_points, void* stream) {
    MOPS_TRY(lattice_check("mops_flowmap_lattice", cfg));
    if (!d_points) return fail(MOPS_ERR_INVALID, "mops_flowmap_lattice: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int W = cfg->width, H = cfg->height;
    const int64_t n = (int64_t)W * H;
    std::vector<double> tables(2 * (size_t)H + 2 * (size_t)W);
    remap_depth_tables(cfg, tables.data(), tables.data() + H, tables.data() + 2 * H, tables.data() + 2 * H + W);
    double* d_tab = nullptr;
    MOPS_TRY(dmalloc(&d_tab, tables.size(), nullptr));
    hipError_t e = hipMemcpyAsync(d_tab, tables.data(), tables.size() * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        remap_positions_kernel<<<grid_for(n), 256, 0, s>>>(n, W, d_tab, d_tab + H, d_tab + 2 * H, d_tab + 2 * H + W,
                                                          d_points);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the tables are freed below
    (void)hipFree(d_tab);
    if (e != hipSuccess) return fail(MOPS_ERR_HIP, std::string("mops_flowmap_lattice: ") + hipGetErrorString(e));
    return MOPS_OK;
}

mops_status mops_ftle_image(const mops_remap_cfg* cfg, const double* d_seeds, const double* d_last,
                            const int32_t* d_death, double horizon, int32_t wrap_lon, double* d_image, void* stream) {
    MOPS_TRY(lattice_check("mops_ftle_image", cfg));
    if (!d_seeds || !d_last || !d_image) return fail(MOPS_ERR_INVALID, "mops_ftle_image: null argument");
    if (!std::isfinite(horizon) || !(horizon > 0.0))
        return fail(MOPS_ERR_INVALID, "mops_ftle_image: the horizon must be finite and positive");
    FtleArgs a;
    a.W = cfg->width; a.H = cfg->height;
    a.n = (int64_t)a.W * a.H;
    a.seeds = d_seeds; a.last = d_last; a.death = d_death;
    a.two_h = 2.0 * horizon;
    a.wrap = wrap_lon != 0;
    a.img = (double2*)d_image;
    // (tiles_x * tiles_y <= (W/32 + 1) * (H/8 + 1) < 2^31 for every W * H < 2^31)
    const int tiles_x = (a.W + kFtleTx - 1) / kFtleTx, tiles_y = (a.H + kFtleTy - 1) / kFtleTy;
    ftle_kernel<<<(unsigned)((int64_t)tiles_x * tiles_y), 256, 0, (hipStream_t)stream>>>(a, tiles_x);
    HIP_TRY(hipGetLastError());
    return MOPS_OK;
}

}  // extern "C"

// ===========================================================================
// path integrals and LAVD (mops_traj.h): the weighted mean of a cell field per level,
// the sum of |sample| * weight along a particle's record slots, and the sum as an image.
//
// mops_level_mean.  The order of the sum is part of the ABI: groups of MOPS_MEAN_GROUP consecutive cells, each
// summed in ascending cell order, then the groups in ascending order.  Lanes run over the levels, as in
// velocity_gradient_kernel: a row of [C][L] is one run of consecutive doubles, and the weight of the row's cell is
// one wave-uniform word.  Stage 1: one wave per group (and per chunk of 64 levels where L > 64) leaves the group's
// {num, den} per level in the partials [L][G]; stage 2: one block per level adds that level's partials in
// ascending g.  No atomics and no hand-off between workgroups: two launches.
// Self-contained on purpose, as the density and FTLE kernels: no dev:: helper is instantiated here.
// ===========================================================================
namespace {

constexpr int kMeanBlock = 64;  // one wave: 64 consecutive levels of one group

static_assert(MOPS_MEAN_GROUP >= 1, "a group holds at least one cell");

__global__ void __launch_bounds__(kMeanBlock) level_mean_group_kernel(int64_t C, int L,
                                                                      const double* __restrict__ field,
                                                                      const double* __restrict__ weight,
                                                                      double* __restrict__ pnum,
                                                                      double* __restrict__ pden) {
    const int l = (int)blockIdx.y * kMeanBlock + (int)threadIdx.x;
    if (l >= L) return;
    const int64_t g = blockIdx.x;
    const int64_t c0 = g * MOPS_MEAN_GROUP;
    const int64_t c1 = c0 + MOPS_MEAN_GROUP < C ? c0 + MOPS_MEAN_GROUP : C;
    double num = 0.0, den = 0.0;
#pragma unroll 8
    for (int64_t c = c0; c < c1; ++c) {
        const double w = weight[c];
        const double x = field[c * L + l];
        if (isfinite(x) && isfinite(w) && w > 0.0) {
            num = num + (w * x);
            den = den + w;
        }
    }
    pnum[(int64_t)l * gridDim.x + g] = num;  // [L][G]: a level's partials are one run for the second stage
    pden[(int64_t)l * gridDim.x + g] = den;
}

// One block per level: its G partials (a contiguous run of [L][G]) go through LDS a tile at a time, loaded by the
// whole block so that a tile's loads are in flight together, and thread 0 adds a tile in ascending g -- the order
// is the ABI's, only the loads are spread.  (One lane per level reading [G][L] rows in a loop was measured first:
// a chain of dependent-latency loads, most of the entry's 0.68 ms at 235 567 x 60)
constexpr int kMeanTotalBlock = 256;
constexpr int kMeanTile = 2048;  // partials of one level per tile: 2 x 16 KB of LDS

__global__ void __launch_bounds__(kMeanTotalBlock) level_mean_total_kernel(int64_t G, const double* __restrict__ pnum,
                                                                           const double* __restrict__ pden,
                                                                           double* __restrict__ mean,
                                                                           double* __restrict__ wsum) {
    __shared__ double sn[kMeanTile], sd[kMeanTile];
    const int l = (int)blockIdx.x;
    const double* rn = pnum + (int64_t)l * G;
    const double* rd = pden + (int64_t)l * G;
    double num = 0.0, den = 0.0;
    for (int64_t g0 = 0; g0 < G; g0 += kMeanTile) {
        const int cnt = (int)(G - g0 < kMeanTile ? G - g0 : kMeanTile);
        for (int k = (int)threadIdx.x; k < cnt; k += kMeanTotalBlock) {
            sn[k] = rn[g0 + k];
            sd[k] = rd[g0 + k];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll 8
            for (int k = 0; k < cnt; ++k) {
                num = num + sn[k];
                den = den + sd[k];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mean[l] = den == 0.0 ? std::numeric_limits<double>::quiet_NaN() : num / den;
        wsum[l] = den;
    }
}

// one lane per slot; ids are a permutation, so every accumulator element has one writer
__global__ void __launch_bounds__(256) path_integral_abs_kernel(int64_t n, int64_t k_begin, int64_t k_end,
                                                                const double* __restrict__ values, int64_t vk,
                                                                int64_t vi, const int32_t* __restrict__ ids,
                                                                double weight, double* __restrict__ accum) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids ? (int64_t)ids[i] : i;
    const double* v = values + i * vi;
    double s = accum[id];
    for (int64_t k = k_begin; k < k_end; ++k) s = s + (fabs(v[k * vk]) * weight);
    accum[id] = s;
}

__global__ void __launch_bounds__(256) path_integral_image_kernel(int64_t n, const double* __restrict__ accum,
                                                                  const int32_t* __restrict__ death, double horizon,
                                                                  double2* __restrict__ img) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const double s = accum[g];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double2 xy, za;
    za.y = 1.0;
    if ((death && death[g] >= 0) || !isfinite(s)) {
        xy.x = nan; xy.y = nan; za.x = nan;
    } else {
        xy.x = s; xy.y = s / horizon; za.x = 0.0;
    }
    img[2 * g] = xy;
    img[2 * g + 1] = za;
}

}  // namespace

extern "C" {

mops_status mops_level_mean(int64_t n_cells, int32_t n_levels, const double* d_field, const double* d_weight,
                            double* d_mean, double* d_wsum, void* stream) {
    if (!d_field || !d_weight || !d_mean || !d_wsum) return fail(MOPS_ERR_INVALID, "mops_level_mean: null argument");
    if (n_cells < 1 || n_levels < 1) return fail(MOPS_ERR_INVALID, "mops_level_mean: n_cells or n_levels below 1");
    const int64_t G = (n_cells + MOPS_MEAN_GROUP - 1) / MOPS_MEAN_GROUP;
    const int64_t chunks = ((int64_t)n_levels + kMeanBlock - 1) / kMeanBlock;
    if (G > 0x7fffffffLL || chunks > 65535)
        return fail(MOPS_ERR_INVALID, "mops_level_mean: too many cells or levels for one launch");
    hipStream_t s = (hipStream_t)stream;
    DevBuf part;  // pnum [L][G] | pden [L][G]
    HIP_TRY(part.alloc((size_t)G * (size_t)n_levels * 2 * sizeof(double)));
    double* pnum = part.as<double>();
    double* pden = pnum + (size_t)G * (size_t)n_levels;
    level_mean_group_kernel<<<dim3((unsigned)G, (unsigned)chunks), kMeanBlock, 0, s>>>(n_cells, n_levels, d_field,
                                                                                       d_weight, pnum, pden);
    level_mean_total_kernel<<<(unsigned)n_levels, kMeanTotalBlock, 0, s>>>(G, pnum, pden, d_mean, d_wsum);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the partials are freed on return
    if (e != hipSuccess) return fail(MOPS_ERR_HIP, std::string("mops_level_mean: ") + hipGetErrorString(e));
    return MOPS_OK;
}

mops_status mops_path_integral_abs(int64_t n, int64_t k_begin, int64_t k_end, const double* d_values, int64_t vk,
                                   int64_t vi, const int32_t* d_ids, double weight, double* d_accum, void* stream) {
    if (!d_values || !d_accum) return fail(MOPS_ERR_INVALID, "mops_path_integral_abs: null argument");
    if (n < 1 || n > (int64_t)0x7fffffff * 256) return fail(MOPS_ERR_INVALID, "mops_path_integral_abs: invalid n");
    if (k_begin < 0 || k_end < k_begin) return fail(MOPS_ERR_INVALID, "mops_path_integral_abs: invalid slot range");
    if (!std::isfinite(weight) || weight < 0.0)
        return fail(MOPS_ERR_INVALID, "mops_path_integral_abs: the weight must be finite and not negative");
    if (k_begin == k_end) return MOPS_OK;
    path_integral_abs_kernel<<<grid_for(n), 256, 0, (hipStream_t)stream>>>(n, k_begin, k_end, d_values, vk, vi, d_ids,
                                                                           weight, d_accum);
    HIP_TRY(hipGetLastError());
    return MOPS_OK;
}

mops_status mops_path_integral_image(int64_t n, const double* d_accum, const int32_t* d_death, double horizon,
                                     double* d_image, void* stream) {
    if (!d_accum || !d_image) return fail(MOPS_ERR_INVALID, "mops_path_integral_image: null argument");
    if (n < 1 || n > (int64_t)0x7fffffff * 256) return fail(MOPS_ERR_INVALID, "mops_path_integral_image: invalid n");
    if (!std::isfinite(horizon) || !(horizon > 0.0))
        return fail(MOPS_ERR_INVALID, "mops_path_integral_image: the horizon must be finite and positive");
    path_integral_image_kernel<<<grid_for(n), 256, 0, (hipStream_t)stream>>>(n, d_accum, d_death, horizon,
                                                                             (double2*)d_image);
    HIP_TRY(hipGetLastError());
    return MOPS_OK;
}

}  // extern "C"
