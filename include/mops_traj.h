/*
 * mops_traj.h -- C ABI of the MI355X (gfx950) particle-trajectory engine.
 *
 * Drop-in boundary for the reference's trajectory path (YosefQiu/MOPS):
 * every entry point below replaces one reference interface, cited per
 * function.  Plain pointers and sizes only; no C++ or torch types.  Device
 * pointers are named d_*, host pointers h_*; `stream` is a hipStream_t
 * passed as void* (NULL = the default stream).
 *
 * Conventions taken from the reference so a caller can pass its own arrays
 * unchanged:
 *   - connectivity is size_t (uint64_t), 1-based, 0 = missing
 *     (MPASOGrid::verticesOnCell_vec / cellsOnCell_vec / cellsOnVertex_vec,
 *     src/Core/MPASOGrid.h);
 *   - coordinates are AoS xyz doubles (std::vector<vec3>::data());
 *   - fields are row-major [entity][level] (MPASOSolution vectors).
 * Internally the engine keeps its own int32 0-based, per-cell-record layout
 * in HBM.
 *
 * Error convention: every function returns mops_status.  MOPS_ERR_INVALID
 * is what the reference answers with Error() + an empty result
 * (MPASOVisualizerKernels.cpp:659-669); mops_last_error() gives the text.
 * Per-particle failures are not errors: the particle stops ("dies") exactly
 * where the reference's lambda returns, and its death step is reported.
 */
#ifndef MOPS_TRAJ_H
#define MOPS_TRAJ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MOPS_OK = 0,
    MOPS_ERR_INVALID = -1,     /* bad arguments / settings (reference: Error() + {}) */
    MOPS_ERR_HIP = -2,         /* HIP runtime failure */
    MOPS_ERR_UNSUPPORTED = -3  /* e.g. maxEdges > 20 (reference MAX_VERTEX_NUM) */
} mops_status;

/* CalcDirection / CalcMethodType (src/Core/MPASOVisualizer.h:14-15) */
enum { MOPS_FORWARD = 0, MOPS_BACKWARD = 1 };
/* MOPS_RK4_RELOCATE: this engine's extension, the opt-out of quirk Q1 (pathlines only).  The pathline RK4 with each of
   stages 2-4 located by the step's own one-hop walk from the step's cell -- over its neighbours in cellsOnCell order,
   then the cell itself; strict <, first minimum -- and evaluated in the cell found, instead of in the step's start
   cell, where a stage point across a cell edge fails IsInMesh and kills the particle.  The particle's own cell does
   not move with a stage; a stage that fails in its own cell still kills the particle at that step.  A particle whose
   stages never leave its cell gets the same bytes as under MOPS_RK4.  A streamline run (back == NULL) and every
   attribute sampling entry return MOPS_ERR_UNSUPPORTED with it.  Any other value than these three runs as MOPS_RK4. */
enum { MOPS_RK4 = 0, MOPS_EULER = 1, MOPS_RK4_RELOCATE = 2 };

typedef struct mops_mesh mops_mesh;    /* device-resident mesh (opaque) */
typedef struct mops_field mops_field;  /* device-resident derived snapshot (opaque) */

/* Host description of an MPAS-O mesh, in MPASOGrid's storage form. */
typedef struct {
    int64_t n_cells;                     /* mCellsSize */
    int64_t n_vertices;                  /* mVertexSize */
    int32_t max_edges;                   /* mMaxEdgesSize */
    int32_t n_vert_levels;               /* mVertLevels (the w grid has +1) */
    const uint64_t* h_n_edges_on_cell;   /* numberVertexOnCell_vec [C] */
    const uint64_t* h_vertices_on_cell;  /* verticesOnCell_vec [C*maxE] */
    const uint64_t* h_cells_on_cell;     /* cellsOnCell_vec [C*maxE] */
    const uint64_t* h_cells_on_vertex;   /* cellsOnVertex_vec [V*3] */
    const double* h_cell_coord;          /* cellCoord_vec [C*3] */
    const double* h_vertex_coord;        /* vertexCoord_vec [V*3] */
} mops_mesh_desc;

/* Raw per-cell fields of one history snapshot (MPASOSolution members). */
typedef struct {
    int32_t timestep;                    /* mTimesteps (informational) */
    const double* h_layer_thickness;     /* cellLayerThickness_vec [C*L] (required) */
    const double* h_bottom_depth;        /* cellBottomDepth_vec [C] or NULL */
    const double* h_surface_height;      /* cellSurfaceHeight_vec [C] or NULL */
    const double* h_zonal_velocity;      /* cellZonalVelocity_vec [C*L] */
    const double* h_meridional_velocity; /* cellMeridionalVelocity_vec [C*L] */
    const double* h_vert_velocity_top;   /* cellVertVelocity_vec [C*(L+1)] or NULL (= 0) */
    const double* h_normal_velocity;     /* cellNormalVelocity_vec [E*L] or NULL: used only when the
                                            zonal/meridional pair is absent, on a mesh with edges
                                            (mops_mesh_set_edges) -- the RBF reconstruction */
} mops_snapshot_desc;

/* TrajectorySettings (src/Core/MPASOVisualizer.h:90-103); seconds. */
typedef struct {
    int64_t delta_t;                     /* deltaT */
    int64_t simulation_duration;         /* simulationDuration */
    int64_t record_t;                    /* recordT */
    int32_t direction;                   /* MOPS_FORWARD / MOPS_BACKWARD */
    int32_t method;                      /* MOPS_RK4 / MOPS_EULER (reference default Euler) */
} mops_traj_cfg;

/* Device-resident particle state, SoA, caller-owned (n entries each). */
typedef struct {
    int64_t n;
    double* d_x;                         /* stable_points x,y,z (updated in place) */
    double* d_y;
    double* d_z;
    float* d_depth;                      /* effective_depths (float, as the reference) */
    int32_t* d_cell;                     /* in: seed cell (default_cell_id), then current cell */
    int32_t* d_death_step;               /* out: -1 alive, else the step it died at */
    const int32_t* d_order;              /* optional processing order (slot -> particle index),
                                            from mops_order_particles; NULL = identity.  Never
                                            changes results, but it decides the kernel family as
                                            well as the speed: a pathline launch with d_order runs
                                            the plain per-lane kernels and never the cooperative
                                            tile kernels, which need the state itself in slot
                                            order (see mops_traj_selection). */
    const int32_t* d_n_live;             /* optional device count: only slots [0, *d_n_live) hold
                                            live particles (after mops_order_particles_live); the
                                            launch spreads just those over the XCDs.  NULL = all n. */
} mops_particles;

const char* mops_last_error(void);
int32_t mops_abi_version(void);

/* Self-test of the trajectory kernel's exact math helpers on the device (not
 * a reference entry point): for n doubles at d_x, op 0 writes {fast sqrt,
 * sqrt()} pairs, op 1 writes {fast sin, sin(), fast cos, cos()} (|x| < 0.78
 * only; other x copy the library values) into d_out (2n or 4n doubles); op 2
 * reads n 3-vectors (3n doubles) and writes {fast a_j / |a| (j = 0..2), a_j / |a|}
 * (6n doubles; zeros where |a| <= 1e-12).  Op 3 reads d_x[0] = a number of
 * steps N and writes the pathline time fractions (double)i / (double)N, i < n,
 * divided on the device (n doubles).  Op 4 reads n pairs (a, b) and writes {a / b
 * by the no-scale division where both lie in its window (else `/`), a / b, 1.0
 * where the no-scale division ran} (3n doubles).  Op 5 reads n hexagons as {6
 * Wachspress numerators 4 B_i, 6 doubled triangle areas R_i} (12n doubles) and
 * writes {6 weights by the evaluation's guarded quotient block, 6 by the plain
 * block, 1.0 where the guard passed} (13n doubles). */
mops_status mops_selftest_math(int64_t n, const double* d_x, double* d_out, int32_t op, void* stream);

/* The pathline kernels' per-run table of time fractions, as built on the host:
 * h_out[s] = (double)s / (double)n_steps for s < n_steps (nothing is written for
 * n_steps <= 0, past the cap or h_out NULL).  Returns the cap: the largest
 * n_steps a run gets a table for; a longer run divides per step.  No device. */
int64_t mops_traj_alpha_table(int64_t n_steps, double* h_out);

/* Self-test of the trajectory kernel's exact neighbour-table shortcut (not a
 * reference entry point; maxEdges <= 7 meshes): for n points d_pts [n][3] in
 * cells d_cells [n], d_out [n] gets bit 0 = the float bisector test kept the
 * cell, bit 1 = the one-hop walk (MPASOVisualizerKernels.cpp:902-922) kept it,
 * bits 8.. = the stay radius the test set (metres); -1 for an invalid cell.
 * Bit 0 without bit 1 would be a wrong shortcut. */
mops_status mops_selftest_walk(const mops_mesh* mesh, int64_t n, const double* d_pts, const int32_t* d_cells,
                               int32_t* d_out, void* stream);

/* ---- mesh / snapshots -------------------------------------------------- */

/* Upload + re-layout a mesh.  Replaces MOPSApp::addGrid / MPASOGrid
 * (src/Core/MOPSApp.cpp:65-75): the KD-tree build becomes the engine's
 * bucket index for mops_locate_cells. */
mops_status mops_mesh_create(const mops_mesh_desc* desc, void* stream, mops_mesh** out);
void mops_mesh_destroy(mops_mesh* mesh);
/* Bytes the mesh occupies in HBM. */
int64_t mops_mesh_bytes(const mops_mesh* mesh);

/* Upload the mesh's edges (MPASOGrid edgesOnCell_vec [C*maxE], cellsOnEdge_vec
 * [E*2], edgeCoord_vec [E*3], reference storage form) for the RBF
 * reconstruction of the cell-centre velocity from edge-normal velocities
 * (TBBBackend::CalcCellCenterVelocity, src/CPU/TBB/MPASOSolutionTBB.cpp:131-245,
 * reached through MPASOSolution::calcCellCenterVelocity,
 * src/Core/MPASOSolution.cpp:85-110).  The per-cell RBF systems depend on the
 * geometry only and are solved here once.  MOPS_ERR_UNSUPPORTED if a cell has
 * more than 7 edges (the reference's stencil arrays hold MAX_VERTEX_NUM = 7). */
mops_status mops_mesh_set_edges(mops_mesh* mesh, int64_t n_edges, const uint64_t* h_edges_on_cell,
                                const uint64_t* h_cells_on_edge, const double* h_edge_coord, void* stream);
/* The RBF cell-centre velocity [C*L*3] from the edge-normal velocity [E*L]
 * (device pointers) -- TBBBackend::CalcCellCenterVelocity's output, bit for
 * bit, quirks included: the stencil always has 7 points (absent edges enter
 * as zero points with zero unit vectors, which makes the 7x7 system singular,
 * i.e. NaN, for every cell with fewer than 7 edges), alpha is 1 and the
 * right-hand side evaluates the RBF at 1 (Interpolation.hpp:223-302). */
mops_status mops_cell_center_velocity_rbf(const mops_mesh* mesh, const double* d_normal_velocity, double* d_out,
                                          void* stream);

/* Upload raw fields and derive, on the GPU, the vertex arrays the trajectory
 * kernels read.  Replaces MOPSApp::addSol's preprocessing chain
 * (src/Core/MOPSApp.cpp:100-129): MPASOSolution::calcCellCenterZtop
 * (MPASOSolution.cpp:535-618), TBBBackend::CalcCellVertexZtop
 * (MPASOSolutionTBB.cpp:9-55), CalcCellCenterVelocityByZM (:108-129) -- or,
 * for a snapshot with edge normals only, CalcCellCenterVelocity (:131-245),
 * CalcCellVertexVelocity (:270-318), CalcCellVertexVertVelocity (:320-366). */
mops_status mops_field_create(const mops_mesh* mesh, const mops_snapshot_desc* desc, void* stream,
                              mops_field** out);
/* As mops_field_create, but every array pointer in d_desc is a DEVICE pointer
 * (raw fields already in HBM, e.g. decoded or generated on the GPU); they are
 * read in place and stay owned by the caller.  Same preprocessing chain
 * (MOPSApp::addSol, src/Core/MOPSApp.cpp:100-129); lets a snapshot-chaining
 * driver (tutorial/pathLine.cpp:244-309) stream snapshots without a host
 * round trip. */
mops_status mops_field_create_device(const mops_mesh* mesh, const mops_snapshot_desc* d_desc, void* stream,
                                     mops_field** out);
/* Re-derive a field made by mops_field_create_device from another snapshot's
 * raw DEVICE arrays, in place: no allocation, asynchronous on `stream`.  The
 * reference rebuilds MPASOSolution per snapshot (MOPSApp::addSol); here a
 * pair-chaining driver recycles the buffers of the snapshot it just finished
 * (stream order: every earlier trajectory launch reading `field` on `stream`
 * completes first).  The raw arrays must stay valid until the work runs. */
mops_status mops_field_rebuild_device(mops_field* field, const mops_snapshot_desc* d_desc, void* stream);
/* Upload already-derived vertex arrays (cellVertexZTop_vec [V*L],
 * cellVertexVelocity_vec [V*L*3], cellVertexVertVelocity_vec [V*(L+1)]);
 * the path MOPSApp::addSol takes when they are pre-set (MOPSApp.cpp:100,107,117). */
mops_status mops_field_create_derived(const mops_mesh* mesh, const double* h_vertex_ztop,
                                      const double* h_vertex_vel, const double* h_vertex_w,
                                      void* stream, mops_field** out);
/* Copy the derived vertex arrays back to the host (any pointer may be NULL). */
mops_status mops_field_export(const mops_field* field, double* h_vertex_ztop, double* h_vertex_vel,
                              double* h_vertex_w, void* stream);
/* CalcCellCenterToVertex (MPASOSolutionTBB.cpp:57-106) for one double
 * attribute [C*L] -> [V*L] (negative results clamped to 0), device pointers. */
mops_status mops_cell_to_vertex_attr(const mops_mesh* mesh, const double* d_cell_attr, double* d_vertex_attr,
                                     void* stream);
void mops_field_destroy(mops_field* field);
int64_t mops_field_bytes(const mops_field* field);

/* ---- seed location ----------------------------------------------------- */

/* Exact nearest cell centre (Euclidean) for n points [n*3] (device
 * pointers).  Replaces MPASOField::calcInWhichCells -> MPASOGrid::searchKDT
 * (src/Core/MPASOField.cpp:23-34, src/Core/MPASOGrid.cpp:287-313, nanoflann
 * 1-NN).  Ties resolve to the smallest cell index. */
mops_status mops_locate_cells(const mops_mesh* mesh, int64_t n, const double* d_points, int32_t* d_cells,
                              void* stream);

/* Same answer as mops_locate_cells, faster when a candidate cell per point is
 * known (d_hint [n], device, may be NULL; entries outside [0, C) are
 * ignored): a point within half the distance from its hint's centre to the
 * nearest OTHER centre (less 1 m) provably has the hint as its unique nearest
 * centre, and skips the search.  Used between chained pathline pairs, where
 * each continuation point's hint is the cell its particle ended in
 * (pyMOPSAPI.py:1446-1459 re-locates every pair's seeds). */
mops_status mops_locate_cells_hinted(const mops_mesh* mesh, int64_t n, const double* d_points,
                                     const int32_t* d_hint, int32_t* d_cells, void* stream);

/* Locality order for n particles: sorts particle indices by a Morton key
 * of their current cell centre, so a wavefront's lanes share cell stencils
 * (no reference counterpart: the reference processes particles in index
 * order).  d_cell [n] -> d_order [n] (device). */
mops_status mops_order_particles(const mops_mesh* mesh, int64_t n, const int32_t* d_cell, int32_t* d_order,
                                 void* stream);

/* Out-of-place gather of particle arrays by a slot order, all in one launch
 * (no reference counterpart: the locality order is the engine's own):
 * dst[row][i] = src[row][d_order[i]] for i < n (d_order NULL = copy), for up
 * to 16 arrays of 4-, 8- or 24-byte elements, each with `rows` rows
 * `row_stride` elements apart (e.g. the [K][6][stride] record slab). */
typedef struct {
    const void* d_src;
    void* d_dst;                         /* must differ from d_src */
    int64_t elem_bytes;                  /* 4, 8 or 24 */
    int64_t rows;                        /* >= 1 */
    int64_t row_stride;                  /* elements between rows (>= n when rows > 1) */
} mops_perm_array;
mops_status mops_permute_arrays(int64_t n, const int32_t* d_order, int32_t count, const mops_perm_array* arrays,
                                void* stream);

/* Dead-particle compaction (no reference counterpart: the reference's
 * parallel_for keeps visiting particles whose lambda has returned,
 * MPASOVisualizerKernels.cpp:944-957, quirk Q1).  As mops_order_particles,
 * but particles with d_death[i] >= 0 (d_death may be NULL) sort after every
 * live one, so live particles fill whole waves; d_n_live (device, may be
 * NULL) receives their count, for mops_particles::d_n_live.  Re-entrant: the caller passes device scratch of
 * at least mops_order_scratch_bytes(n) bytes, so several particle parts can
 * be re-sorted concurrently on their own streams. */
int64_t mops_order_scratch_bytes(int64_t n);
mops_status mops_order_particles_live(const mops_mesh* mesh, int64_t n, const int32_t* d_cell,
                                      const int32_t* d_death, int32_t* d_order, int32_t* d_n_live,
                                      void* d_scratch, int64_t scratch_bytes, void* stream);
/* Zero record slots [k_begin, K) of slots [*d_n_live, n) (d_records [K][6][record_stride]):
 * after a compaction that moved only the sampled slots [0, k_begin), the dead particles now
 * at the end carry the zeros of their unsampled slots again (see mops_traj_advance).  No
 * reference counterpart (the reference never re-sorts). */
mops_status mops_records_clear_dead(int64_t n, const int32_t* d_n_live, int64_t k_begin, int64_t K,
                                    double* d_records, int64_t record_stride, void* stream);

/* ---- trajectory hot path (device-resident) ----------------------------- */

/* Number of record slots K = simulation_duration / record_t (reference
 * each_points_size, MPASOVisualizerKernels.cpp:703). */
int64_t mops_traj_num_records(const mops_traj_cfg* cfg);
/* Number of integration steps = simulation_duration / delta_t. */
int64_t mops_traj_num_steps(const mops_traj_cfg* cfg);

/* Advance particles over global steps [step_begin, step_end) of one
 * StreamLine (back == NULL; Kernel::StreamLine, MPASOVisualizerKernels.cpp:
 * 874-1003) or PathLine (Kernel::PathLine, :1329-1483) call.  Records go to
 * d_records laid out [K][6][record_stride] doubles (px,py,pz,vx,vy,vz);
 * slot 0 also receives the seed / first-step velocity pre-writes
 * (:901, :990).  d_records needs no initialisation when the calls start at
 * step 0: every slot a particle does not sample (after its death, past the
 * run's last record step, or all of them for a particle already dead at step
 * 0) is written with the zeros of the reference's vector::resize zero-init --
 * at its death or by the call that reaches n_steps.  A caller whose
 * first call starts after step 0 passes records zero-filled.  Calling it over
 * consecutive step ranges is identical to one call over [0, n_steps); a
 * caller that moves particles between slots in between (a re-sort) moves
 * every record slot, or clears the moved dead particles' unsampled slots
 * (mops_records_clear_dead).
 * Streams: pathline launches keep one small device flag per HIP stream in
 * the mesh (the cooperative-tile selection), freed with the mesh.  Use
 * long-lived streams (torch's pool, or streams created once): a stream
 * destroyed while its launches still run, whose handle a new stream then
 * reuses, would share that flag with the old launches.
 * Ranges: the number of steps, the number of records and the record period
 * in steps must each be below 2^31 (MOPS_ERR_INVALID otherwise, decided from
 * cfg alone): the kernel counts them in 32 bits. */
mops_status mops_traj_advance(const mops_mesh* mesh, const mops_field* front, const mops_field* back,
                              const mops_traj_cfg* cfg, const mops_particles* particles,
                              int64_t step_begin, int64_t step_end, double* d_records,
                              int64_t record_stride, void* stream);

/* Which kernel family the pathline launches of `stream` on this mesh ran: a
 * blocking test / diagnostic entry, not part of any hot path (no reference
 * counterpart).  A pathline launch of mops_traj_advance (and of the sampled and
 * captured entries over it) on a maxEdges <= 7 mesh with d_order == NULL and a
 * method other than MOPS_RK4_RELOCATE first runs the selection kernel, which
 * counts the runs of equal cells per 64-slot wave and sets the stream's device
 * flag: 1 = the cooperative tile kernels run (Euler: the tile step; RK4: the
 * hand-off kernel and the resumed one), 0 = the plain kernel.  Every other
 * launch -- streamlines, d_order set, MOPS_RK4_RELOCATE, the layer and the
 * diffusive entries, a wider mesh -- makes no selection and runs per-lane
 * kernels.
 * *count: the number of launches so far on this (mesh, stream) that made a
 * selection, a host counter (0 if none).  *flag: the device flag after
 * hipStreamSynchronize(stream), i.e. how the stream's last selection fell;
 * -1 when *count == 0.  A caller reads *count before and after a launch: the
 * difference says a selection was made, *flag how it fell.
 * MOPS_ERR_INVALID for a null argument. */
mops_status mops_traj_selection(const mops_mesh* mesh, void* stream, int32_t* flag, int64_t* count);

/* ---- fixed-layer streamlines and pathlines -------------------------------- */

/* Advection within ONE model layer k (0 <= k < nVertLevels): the StreamLine / PathLine loop of
 * mops_traj_advance -- the one-hop walk, the Euler rotation, the RK4 stage positions, stage alphas, mean and
 * chord step, the two recording rules, the step-0 pre-writes, the death bookkeeping, the zero-filled
 * unsampled slots -- with calc_velocity_at replaced by the layer evaluation:
 *   1. the reference's cell guards, TBBKernel::IsInMesh and the Wachspress weights of the cell;
 *   2. h_f = sum_v w_v * cellVertexVelocity_front[v*L + k], in the reference's vertex order
 *      (TBBKernel::CalcVelocity, TBBKernel.h:128-147); a streamline takes h = h_f, a pathline forms h_b the
 *      same way from the back snapshot and h = h_b*alpha + h_f*(1 - alpha), in that order;
 *   3. the evaluation fails, and the particle dies at that step, where |h| < 1e-12 with
 *      |h| = sqrt((x*x + y*y) + z*z).  For streamlines that is the reference's own rule
 *      (MPASOVisualizerKernels.cpp:838-852); for pathlines it is THIS ENGINE'S CHOICE (the reference's pathline
 *      has no such test), so that particles over land die instead of sitting still for the rest of the run;
 *   4. the vertical velocity is 0.0: zTop and cellVertexVertVelocity are never read.
 * The vertical-update lines are kept with w = 0, so the depth stays what the caller gave (a negative depth
 * becomes 0, as the reference's max(0, .) makes it) and the position is renormalised to its radius each step.
 * With fields whose vertex zTop column is exactly 0, -100, -200, ... and whose w is zero, a depth-0 run of
 * mops_traj_advance is a layer-0 run (its bracket blends level 0 with weight 1.0 exactly).
 *
 * cfg->method: MOPS_RK4 evaluates the stages in the step's start cell (quirk Q1); MOPS_RK4_RELOCATE locates
 * each of stages 2-4 as mops_traj_advance does for pathlines -- here for streamlines as well (the refusals of
 * the depth entries are unchanged).
 *
 * A layer slice is one snapshot's velocity at layer k as a compact per-vertex array in the engine's own vertex
 * order: opaque to the caller, mops_layer_velocity_bytes(mesh) bytes of device memory, 16-byte aligned.
 * mops_field_layer_velocity writes it (asynchronous on `stream`; rebuild it whenever the field is rebuilt);
 * MOPS_ERR_INVALID before any launch for a null pointer, a field of another mesh or a layer outside
 * [0, nVertLevels). */
int64_t mops_layer_velocity_bytes(const mops_mesh* mesh);
mops_status mops_field_layer_velocity(const mops_mesh* mesh, const mops_field* field, int32_t layer, void* d_out,
                                      void* stream);

/* mops_traj_advance in layer mode: d_front_layer / d_back_layer are layer slices of the same layer
 * (d_back_layer NULL = a streamline).  Particles, step ranges, records, d_order / d_n_live, re-sorts between
 * calls and the 32-bit ranges are those of mops_traj_advance; the kernel reads the mesh and the two slices
 * only.  One lane per particle, no cooperative tile, no capture, no attribute channel.  MOPS_ERR_INVALID
 * before any launch for a null d_front_layer. */
mops_status mops_traj_advance_layer(const mops_mesh* mesh, const void* d_front_layer, const void* d_back_layer,
                                    const mops_traj_cfg* cfg, const mops_particles* particles, int64_t step_begin,
                                    int64_t step_end, double* d_records, int64_t record_stride, void* stream);

/* ---- random-walk horizontal diffusion (no reference counterpart) ----------- */

/* A horizontal random walk with a constant eddy diffusivity kh (m^2/s; Visser's walk with uniform deviates): one
 * kick per live particle per step, after the step's position update (the vertical update and its renormalisation
 * included) and before the record test, so records hold the kicked position; the recorded velocity stays the
 * advective one.  A particle that dies at a step gets no kick at that step.  All of it in FP64 without
 * contraction, len(v) = sqrt((x*x + y*y) + z*z), every `/` and sqrt correctly rounded.
 *
 * Generator: Philox4x32-10 as in Random123 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 /
 * 0xBB67AE85, 10 rounds) with key = (seed & 0xffffffff, seed >> 32) and counter = (gid & 0xffffffff, gid >> 32,
 * step, epoch): gid = id_base + d_id[particle] (d_id NULL: the particle's index in the arrays) is the 64-bit
 * global particle id, step the call's global step index, epoch a word the caller owns (a chain of calls sets it
 * to the call's index).  So a run's bytes do not depend on how it is split into launches, re-sorted, compacted or
 * spread over devices, as long as every particle keeps its id.
 * Deviates: R1 from output word 0, R2 from word 1, R = ((double)(int32_t)w + 0.5) * 2^-31 -- exact, symmetric,
 * in (-1, 1), never 0, variance 1/3.
 * Kick of p = (x, y, z):
 *   s   = sqrt(6.0 * kh * (double)|delta_t|)                       (once, on the host: mops_diffusion_scale)
 *   r   = len(p), rho = sqrt(x*x + y*y)
 *   e   = (-y/rho, x/rho, 0) if rho > 1e-6, else (1, 0, 0)         (east)
 *   n   = ((0.0 - z*e_y)/r, (z*e_x)/r, (x*e_y - y*e_x)/r)          (north)
 *   a   = R1*s, b = R2*s, d = (a*e_x + b*n_x, a*e_y + b*n_y, b*n_z)
 *   p'  = CalcPositionAfterRotation(p, axis = p x d, theta = len(d) / max(1e-12, r))
 * with the cross-product order of the Euler step.  No renormalisation follows: the kick is horizontal, depth and
 * radius are untouched.  A kick onto land or out of the mesh kills the particle at the next step by the existing
 * rules.  Backward runs use |delta_t|.
 *
 * kh == 0 runs no kick code: every entry below forwards to the entry it mirrors (the same bytes).  kh < 0 or a
 * non-finite kh is MOPS_ERR_INVALID before any launch. */
typedef struct {
    double kh;                           /* eddy diffusivity, m^2/s */
    uint64_t seed;                       /* the Philox key */
    uint32_t epoch;                      /* counter word 3 */
    int64_t id_base;                     /* added to every id */
    const int32_t* d_id;                 /* device ids [n], indexed like the particle arrays; NULL = the index */
} mops_diffusion;

/* sqrt(6.0 * kh * (double)|delta_t|) as the entries form it. */
double mops_diffusion_scale(double kh, int64_t delta_t);

/* mops_traj_advance with the kick, for pathlines: every method (MOPS_EULER, MOPS_RK4, MOPS_RK4_RELOCATE), a
 * per-lane kernel (no cooperative tile, no capture).  MOPS_ERR_UNSUPPORTED for back == NULL with kh > 0. */
mops_status mops_traj_advance_diffuse(const mops_mesh* mesh, const mops_field* front, const mops_field* back,
                                      const mops_traj_cfg* cfg, const mops_particles* particles,
                                      const mops_diffusion* diffusion, int64_t step_begin, int64_t step_end,
                                      double* d_records, int64_t record_stride, void* stream);

/* mops_traj_advance_layer with the kick: streamlines (d_back_layer NULL) and pathlines, every method. */
mops_status mops_traj_advance_layer_diffuse(const mops_mesh* mesh, const void* d_front_layer,
                                            const void* d_back_layer, const mops_traj_cfg* cfg,
                                            const mops_particles* particles, const mops_diffusion* diffusion,
                                            int64_t step_begin, int64_t step_end, double* d_records,
                                            int64_t record_stride, void* stream);

/* Self-test of the generator on the device: d_in holds n rows of {4 counter words, 2 key words}; d_words gets the
 * 4 output words per row, d_r the deviates {R1, R2} of words 0 and 1. */
mops_status mops_selftest_philox(int64_t n, const uint32_t* d_in, uint32_t* d_words, double* d_r, void* stream);

/* FinalizeTrajectoryLines[WithAttrs] + RemoveNaNTrajectoriesAndReindex
 * (src/Common/TrajectoryCommon.h:57-190) on the device: seeds [n*3] and
 * records -> points/velocity [n*(K+1)*3], temperature/salinity [n*(K+1)]
 * (pathline: velocity x/y, reference quirk Q9; streamline: zeros),
 * last point [n*3].  d_line [n] (or NULL = identity) maps particle slot i of
 * seeds/records to output line d_line[i] -- for particles kept physically in
 * locality order (the record stores of mops_traj_advance then coalesce).
 * Any output pointer except points may be NULL. */
mops_status mops_traj_finalize(int64_t n, int64_t K, const double* d_seeds, const double* d_records,
                               int64_t record_stride, int32_t pathline, const int32_t* d_line, double* d_points,
                               double* d_velocity, double* d_temperature, double* d_salinity, double* d_last_point,
                               void* stream);

/* mops_traj_finalize's d_last_point alone: each line's cleaned last point
 * (RemoveNaNTrajectoriesAndReindex, src/Common/TrajectoryCommon.h:92-121:
 * the last finite point before the first non-finite one) from the seeds and
 * the records' positions, written at d_line[i] (NULL = identity).  What the
 * next pair of a chain needs as its seeds (MOPSPathline.run's _last_pt,
 * tutorial/pyMOPSAPI.py:1488), so the full line assembly can run
 * beside the next pair.  Same values as mops_traj_finalize's bit for bit. */
mops_status mops_traj_last_points(int64_t n, int64_t K, const double* d_seeds, const double* d_records,
                                  int64_t record_stride, const int32_t* d_line, double* d_last_point, void* stream);

/* ---- attribute sampling along pathlines (opt-in) -------------------------- */

/* Attributes one call samples at most (the reference's vec3 channel holds two,
 * MPASOVisualizerKernels.cpp:1288-1324). */
#define MOPS_MAX_SAMPLE_ATTRS 4

/* The attribute channel of Kernel::PathLine (MPASOVisualizerKernels.cpp:
 * 1091-1104, :1288-1324, :1431, :1453-1456, :1476-1478), which the reference
 * computes at every evaluation and FinalizeTrajectoryLinesWithAttrs then drops
 * (src/Common/TrajectoryCommon.h:176-185, quirk Q9).  Attribute arrays are
 * DEVICE vertex arrays [V*L] in the caller's vertex order, as
 * mops_cell_to_vertex_attr makes them (mDoubleAttributes_CtoV), one per field
 * and attribute.  The slab d_attr_records is [K][n_attr][attr_stride] doubles,
 * zero-filled by the caller before step 0 (the reference's update_attrs after
 * vector::resize); a particle that never reaches a slot leaves its zero there.
 *
 * Sample steps of a run, with ri = record_t / delta_t (:1470): step 0 writes
 * slot 0 (the first_attr pre-write, :1453-1456, which a later record into
 * slot 0 overwrites); every step j < n_steps with ri > 0 and (j + 1) % ri == 0
 * writes slot (j + 1) / ri - 1 when that slot is below K (:1470-1481).
 *
 * mops_traj_sample_attrs: one sample step for particles that stand exactly at
 * `step` (after mops_traj_advance over [.., step), or fresh seeds for step 0).
 * It evaluates that step as the pathline loop does before the move -- the
 * one-hop walk (:1361-1381, step > 0), calc_velocity_at with its attributes at
 * the position, cell, float depth and alpha the step starts from; for RK4 the
 * four stages and their weighted mean (:1404-1432) -- and writes current_attrs
 * into the step's slot for every live particle the step does not kill.  It
 * reads the particle state only: positions, depths, cells and death steps
 * stay untouched.  d_order and d_n_live are honoured as by mops_traj_advance.
 * MOPS_ERR_INVALID for a null handle or pointer, n_attr outside
 * 1..MOPS_MAX_SAMPLE_ATTRS, attr_stride < n or a step that is not a sample
 * step; MOPS_ERR_UNSUPPORTED for back == NULL (the reference's StreamLine has
 * no attribute channel).  Every argument is checked before any device work. */
mops_status mops_traj_sample_attrs(const mops_mesh* mesh, const mops_field* front, const mops_field* back,
                                   const mops_traj_cfg* cfg, const mops_particles* particles, int64_t step,
                                   int32_t n_attr, const double* const* d_front_attrs,
                                   const double* const* d_back_attrs, double* d_attr_records, int64_t attr_stride,
                                   void* stream);

/* mops_traj_advance over [step_begin, step_end) with the attribute channel
 * (Kernel::PathLine, MPASOVisualizerKernels.cpp:1329-1483): one host call that
 * advances to each sample step of the range, samples it
 * (mops_traj_sample_attrs) and goes on.  Positions, records, depths and death
 * steps are those of mops_traj_advance over the same range, bit for bit
 * (mops_traj_advance is exact over consecutive step ranges).  Argument checks
 * as mops_traj_sample_attrs, before any device work. */
mops_status mops_traj_advance_sampled(const mops_mesh* mesh, const mops_field* front, const mops_field* back,
                                      const mops_traj_cfg* cfg, const mops_particles* particles, int64_t step_begin,
                                      int64_t step_end, double* d_records, int64_t record_stride, int32_t n_attr,
                                      const double* const* d_front_attrs, const double* const* d_back_attrs,
                                      double* d_attr_records, int64_t attr_stride, void* stream);

/* ---- the same in one launch per window: capture, then one batched sampler ---- */

/* Bytes of a capture slab of `slots` window slots for `stride` particles: per
 * particle and slot the state a sample step starts from -- x, y, z (double),
 * the float depth, the cell its walk starts from -- 32 B, one plane per
 * component ([5 planes][slots][stride]).  0 for an empty slab, -1 for a
 * negative argument or an overflow.  Host only. */
int64_t mops_traj_capture_bytes(int64_t stride, int64_t slots);

/* The launches mops_traj_advance_captured makes for steps [step_begin,
 * step_end) (clamped to the run) with a window of W = capture_slots slots
 * (at most 65535 are used per launch).  Host only, no device work.  Returns
 * the number of launches and stores the end step of launch i in out_bounds[i]
 * for i < cap (out_bounds may be NULL with cap == 0): launch i runs
 * [out_bounds[i - 1], out_bounds[i]), the first from step_begin, the last to
 * step_end; the ends increase strictly.  Every sample step of the range is
 * either a launch's first step -- sampled from the particle state by
 * mops_traj_sample_attrs' kernel, as step 0 and a range that starts on a
 * sample step are -- or interior to exactly one launch, which holds at most W
 * interior sample steps: each launch ends at the (W + 1)-th sample step after
 * its first step, or at step_end.  W = 0 is mops_traj_advance_sampled's split:
 * a launch boundary at every sample step.  -1 (and mops_last_error) for a null
 * or invalid cfg, capture_slots < 0, cap < 0 or a NULL out_bounds with
 * cap > 0. */
int64_t mops_traj_capture_plan(const mops_traj_cfg* cfg, int64_t step_begin, int64_t step_end, int64_t capture_slots,
                               int64_t* out_bounds, int64_t cap);

/* mops_traj_advance_sampled without a launch boundary at every sample step.
 * Per launch of mops_traj_capture_plan, all on `stream`: the window's cell
 * plane is marked "not captured" (all-ones bytes, cell = -1); a sample step
 * that is the launch's first step is sampled from the particle state; the
 * trajectory launch -- the capture instantiation of the same kernel -- stores
 * the step-start state of every interior sample step for every particle still
 * alive there (a dead particle never stores); one batched kernel then
 * evaluates every captured (slot, particle) exactly as mops_traj_sample_attrs
 * does from the particle state and writes the attribute slots.  A particle the
 * sample step kills writes nothing, so the slot keeps its zero.  Slot 0 is
 * written twice as in the reference: the step-0 pre-write first, then the
 * sample of step ri - 1, which overwrites only on success (with ri == 1 step
 * 0 is both).  The attribute slab, the records, positions, depths, cells and
 * death steps are those of mops_traj_advance_sampled byte for byte, for every
 * capture_slots and step range.
 *
 * d_capture: mops_traj_capture_bytes(n, capture_slots) bytes of device
 * memory for this call's n = particles->n (scratch: nothing is kept in it
 * between calls; concurrent calls on disjoint particle ranges need disjoint
 * slabs).  d_n_live and d_order are honoured as by mops_traj_advance.
 * capture_slots == 0, or a mesh past maxEdges 7 (no capture instantiations),
 * takes mops_traj_advance_sampled's path inside this entry; d_capture may then
 * be NULL.  Argument checks as mops_traj_advance_sampled plus
 * MOPS_ERR_INVALID for capture_slots < 0 or a NULL d_capture with
 * capture_slots > 0, all before any device work. */
mops_status mops_traj_advance_captured(const mops_mesh* mesh, const mops_field* front, const mops_field* back,
                                       const mops_traj_cfg* cfg, const mops_particles* particles, int64_t step_begin,
                                       int64_t step_end, double* d_records, int64_t record_stride, int32_t n_attr,
                                       const double* const* d_front_attrs, const double* const* d_back_attrs,
                                       double* d_attr_records, int64_t attr_stride, void* d_capture,
                                       int64_t capture_slots, void* stream);

/* The attribute lines from the slab, with the cleanup
 * RemoveNaNTrajectoriesAndReindex applies to temperature / salinity
 * (src/Common/TrajectoryCommon.h:88-121): entry j < K of a line is slot j,
 * entry K the appended 0 (:88-90); with k the first non-finite point of the
 * line (the seed at index 0, record j at index j + 1), k == 0 sets every entry
 * to entry 0 and 0 < k < K + 1 sets the entries j >= k to entry k - 1.
 * d_line as in mops_traj_finalize; d_attr_lines is [n_attr][n*(K+1)]. */
mops_status mops_traj_finalize_attrs(int64_t n, int64_t K, const double* d_seeds, const double* d_records,
                                     int64_t record_stride, int32_t n_attr, const double* d_attr_records,
                                     int64_t attr_stride, const int32_t* d_line, double* d_attr_lines, void* stream);

/* RemoveNaNTrajectoriesAndReindex alone on n lines of P points each, in
 * place (device pointers; [n*P*3], [n*P*3], [n*P], [n*P], out [n*3]). */
mops_status mops_remove_nan_lines(int64_t n, int64_t P, double* d_points, double* d_velocity,
                                  double* d_temperature, double* d_salinity, double* d_last_point, void* stream);
/* The same for ragged lines -- the reference's vector<TrajectoryLine>, whose
 * lines may differ in length (RemoveNaNTrajectoriesAndReindex,
 * src/Common/TrajectoryCommon.h:57-129; test/test_trajector.cpp:26-194):
 * line i is points [d_offsets[i], d_offsets[i+1]) of the packed arrays
 * (d_offsets [n+1], device), velocity/temperature/salinity already resized to
 * the points' length (:88-90).  One launch for all lines; an empty line is
 * left untouched (the reference drops it and re-indexes the rest, which is
 * host bookkeeping).  d_last_point [n*3] gets each non-empty line's last point. */
mops_status mops_remove_nan_ragged(int64_t n, const int64_t* d_offsets, double* d_points, double* d_velocity,
                                   double* d_temperature, double* d_salinity, double* d_last_point, void* stream);

/* ---- image remapping ---------------------------------------------------- */

/* Layer rule of mops_remap_fixed_depth.  MOPS_LAYER_REFERENCE is the
 * reference: MPASOVisualizerKernels.cpp:392-394 set local_layer = 0 whenever
 * the depth lies at or below the column's top, so every wet pixel is the mean
 * of the two top levels.  MOPS_LAYER_BRACKET (no
 * reference counterpart) leaves those three lines out: the layer is the one
 * the search found. */
enum { MOPS_LAYER_REFERENCE = 0, MOPS_LAYER_BRACKET = 1 };

/* VisualizationSettings (src/Core/MPASOVisualizer.h:20-42) as the two
 * remapping kernels read it; degrees and metres. */
typedef struct {
    int32_t width, height;               /* imageSize.x, imageSize.y */
    double min_lat, max_lat;             /* LatRange (fixed depth only) */
    double min_lon, max_lon;             /* LonRange */
    double fixed_depth;                  /* FixedDepth, positive down (negated, :251) */
    double fixed_latitude;               /* FixedLatitude (fixed latitude only) */
    double min_depth, max_depth;         /* fixed latitude rows: cellRefBottomDepth_vec.front() / .back() (:496-497) */
    int32_t layer_rule;                  /* MOPS_LAYER_REFERENCE / MOPS_LAYER_BRACKET (fixed depth only) */
    double fixed_layer;                  /* FixedLayer (fixed layer only; read by mops_remap_fixed_layer alone, so a
                                            caller of the other entries may pass the struct without it) */
} mops_remap_cfg;

/* Images MOPSApp::runRemapping returns for a solution with n_attr double
 * attributes (MOPSApp.cpp:176-185): 1 + ceil(n_attr / 3), or 1 without any. */
int32_t mops_remap_num_images(int32_t n_attr);

/* The host cos / sin tables the pixel positions are formed from (host only,
 * no device work): fixed_latitude == 0 -- GeoConverter::
 * convertPixelToLatLonToRadians (GeoConverter.hpp:28-32) per row [height] and
 * per column [width]; != 0 -- VisualizeFixedLatitude's one row [1] at
 * FixedLatitude and columns lon = minLon + j * j_step
 * (MPASOVisualizerKernels.cpp:513-523).  libm cos / sin, as the reference's
 * convertRadianLatLonToXYZ (GeoConverter.hpp:118-124). */
mops_status mops_remap_tables(const mops_remap_cfg* cfg, int32_t fixed_latitude, double* h_row_cos,
                              double* h_row_sin, double* h_col_cos, double* h_col_sin);

/* MOPSApp::runRemapping -> Kernel::VisualizeFixedDepth (MOPSApp.cpp:171-196,
 * MPASOVisualizerKernels.cpp:238-471), bit for bit: TBBKernel::SearchKDTree
 * becomes mops_locate_cells on positions formed on the device from
 * mops_remap_tables.  d_images receives mops_remap_num_images(n_attr) images
 * [height][width][4] doubles: image 0 = {u_east, v_north, speed, 1}; image 1
 * is written only when n_attr > 1, {d_attr0, d_attr1, 0, 1} (vertex arrays
 * [V*L] in the caller's vertex order from mops_cell_to_vertex_attr, in
 * std::map name order: mDoubleAttributes_CtoV), and stays zero otherwise, as
 * every later image.  d_cells [height*width] (optional) receives the cell of
 * each pixel.  h_stage_ms (optional, host, 3 floats) receives the HIP-event
 * times of the positions, locate and evaluation stages.  Synchronises
 * `stream`.  MOPS_ERR_INVALID (nothing written) where the reference answers
 * Error() and returns, and for a bad image size, rule or attribute count. */
mops_status mops_remap_fixed_depth(const mops_mesh* mesh, const mops_field* field, const mops_remap_cfg* cfg,
                                   int32_t n_attr, const double* d_attr0, const double* d_attr1, double* d_images,
                                   int32_t* d_cells, float* h_stage_ms, void* stream);

/* MOPSApp::runReGrid -> Kernel::VisualizeFixedLatitude (MOPSApp.cpp:198-210,
 * MPASOVisualizerKernels.cpp:473-651), bit for bit: rows are depths from
 * min_depth to max_depth, columns longitudes at fixed_latitude; the inside
 * test is MPASOField::isOnOcean (MPASOField.cpp:36-81).  d_image
 * [height][width][4] = {zonal, meridional, 0, 1}.  A column's position and
 * cell do not depend on the row, so only `width` points are located; d_cells
 * [width] (optional) receives them.  Synchronises `stream`. */
mops_status mops_remap_fixed_latitude(const mops_mesh* mesh, const mops_field* field, const mops_remap_cfg* cfg,
                                      double* d_image, int32_t* d_cells, void* stream);

/* Kernel::VisualizeFixedLayer (MPASOVisualizerKernels.cpp:141-236), bit for
 * bit: pixel positions and cells as mops_remap_fixed_depth (LatRange,
 * LonRange); a pixel is {NaN, NaN, NaN, 1} where its cell is out of range, the
 * cell's vertex count is outside 1..20 or TBBKernel::IsInMesh fails, else
 * {zonal, meridional, 0, 1} of the Wachspress-weighted vertex velocity
 * (TBBKernel::CalcVelocity) at layer ClampLayer((int)cfg->fixed_layer, L)
 * (:14-26, :166): the double truncates toward zero, a negative value gives 0,
 * L or more gives L - 1 (a NaN, undefined there, gives 0).  d_image
 * [height][width][4]; d_cells [height*width] (optional) receives the cell of
 * each pixel.  Synchronises `stream`. */
mops_status mops_remap_fixed_layer(const mops_mesh* mesh, const mops_field* field, const mops_remap_cfg* cfg,
                                   double* d_image, int32_t* d_cells, void* stream);

/* ---- vertical sections along great-circle paths -------------------------- */

/* The columns of a section through n_way >= 2 waypoints h_waypoints
 * [n_way][2] = (lat, lon) in degrees, joined by great-circle legs: width >= 2
 * columns equally spaced in arc length over the whole polyline.  Host only, no
 * device work; FP64, libm cos / sin / atan2 / sqrt, no contraction, every
 * expression as written here, left to right (R = 6371010, the remapping's
 * radius; dot(a, b) = (ax*bx + ay*by) + az*bz; len(q) = sqrt((qx*qx + qy*qy) +
 * qz*qz)):
 *   waypoint i:  theta = lat * (M_PI / 180.0), phi = lon * (M_PI / 180.0),
 *                u_i = (cos(theta)*cos(phi), cos(theta)*sin(phi), sin(theta))
 *   leg i (a = u_i, b = u_i+1):  d = dot(a, b), q = b - d*a (per component),
 *                ang_i = atan2(len(q), d), t_i = q / len(q) (per component),
 *                cum_0 = 0.0, cum_i+1 = cum_i + ang_i, total = cum_(n_way-1)
 *   column j:    j == 0: leg 0, s = 0.0, phi = 0.0;  j == width-1: the last
 *                leg, s = total, phi = its ang;  else s = ((double)j * total) /
 *                (double)(width - 1), the leg is the first whose cum_i+1 is
 *                not below s (the last leg otherwise), phi = s - cum_leg,
 *                lowered to ang_leg where it exceeds it
 *                c = cos(phi), sn = sin(phi), with the leg's a and t:
 *                p^ = c*a + sn*t          (unit position)
 *                tau = c*t - sn*a         (direction of travel)
 *                h_points[j]  = (R * p^x, R * p^y, R * p^z)
 *                h_normals[j] = p^ x tau = (p^y*tauz - p^z*tauy,
 *                               p^z*taux - p^x*tauz, p^x*tauy - p^y*taux)
 *                h_dist[j]    = R * s     (metres from the first waypoint)
 * The normal is the horizontal unit vector to the LEFT of the direction of
 * travel: north for a west-to-east section.  h_points, h_normals [width][3],
 * h_dist [width].  MOPS_ERR_INVALID, nothing written: a null pointer, n_way <
 * 2, width < 2, a non-finite waypoint, |lat| > 90, a leg of zero length (ang <
 * 1e-12 rad, where q is rounding noise) or within 1e-9 rad of antipodal (ang >
 * M_PI - 1e-9: its great circle is not defined). */
mops_status mops_section_points(int32_t n_way, const double* h_waypoints, int32_t width, double* h_points,
                                double* h_normals, double* h_dist);

/* A depth-by-distance image along `width` columns.  h_points [width][3] (host;
 * mops_section_points' or any others) are the column positions, located with
 * mops_locate_cells; rows are depths, depth_plot = min_depth + ih * i_step,
 * i_step = height > 1 ? (max_depth - min_depth) / (height - 1) : 0, DEPTH =
 * -fabs(depth_plot), as in mops_remap_fixed_latitude.
 *   d_image0 [height][width][4] = {zonal, meridional, across, 1}: channels 0
 *   and 1 are Kernel::VisualizeFixedLatitude's pixel
 *   (MPASOVisualizerKernels.cpp:545-651) for the column's position and the
 *   row's depth, bit for bit: MPASOField::isOnOcean, the Wachspress weights,
 *   the weighted zTop column with its clamp, the range test and the layer
 *   search with EPSILON = 1e-6, `up` / `dn` ordered, denom = up - dn (|denom| <
 *   1e-30 fails), t = (DEPTH - dn) / denom, c = 1.0 - t, the level sums vel_up
 *   (layer - 1) and vel_dn (layer), f = c*vel_dn + t*vel_up per component,
 *   convertXYZVelocityToENU(position, f).  across = (fx*nx + fy*ny) + fz*nz
 *   with the column's h_normals [width][3] row n; 0.0 when h_normals is NULL.
 *   A failed pixel is {NaN, NaN, NaN, 1}.
 *   d_image1 (written iff n_attr >= 1) = {attr0, attr1 or 0, 0, 1}: d_attr0 /
 *   d_attr1 are vertex arrays [V*L] in the caller's vertex order
 *   (mops_cell_to_vertex_attr); up_a = sum_v w_v * attr[v*L + layer-1], dn_a =
 *   sum_v w_v * attr[v*L + layer], both in the cell's vertex order from 0.0,
 *   attr = c*dn_a + t*up_a.  NaN where image 0 is NaN.
 * d_cells [width] (optional) receives the columns' cells.  n_attr is 0..2.
 * The per-column work is done once per column, not per pixel; the values do
 * not depend on that.  Synchronises `stream`.  MOPS_ERR_INVALID before any
 * device work, nothing written: a null handle or pointer (h_points, d_image0;
 * d_attr0 and d_image1 with n_attr >= 1; d_attr1 with n_attr == 2), a field of
 * another mesh, width or height < 1, width * height > 2^31 - 1, n_attr outside
 * 0..2, a non-finite depth, a mesh of more than 100 levels. */
mops_status mops_remap_section(const mops_mesh* mesh, const mops_field* field, int32_t width, int32_t height,
                               double min_depth, double max_depth, const double* h_points, const double* h_normals,
                               int32_t n_attr, const double* d_attr0, const double* d_attr1, double* d_image0,
                               double* d_image1, int32_t* d_cells, void* stream);

/* Volume transport through a section image (host only): h_image0
 * [height][width][4] from mops_remap_section, h_dist [width] from
 * mops_section_points, the rows' depth range.  ds_j = 0.5 * (dist[min(j+1,
 * width-1)] - dist[max(j-1, 0)]) (half the distance to each neighbour,
 * one-sided at the ends); dz = (max_depth - min_depth) / (height - 1), dz_i =
 * 0.5 * dz in the first and last row, dz elsewhere.  Over the pixels whose
 * across channel is not NaN, row major, one sequential FP64 sum each from 0.0:
 * sum += (across * ds_j) * dz_i; area += ds_j * dz_i.  *h_sverdrup = sum /
 * 1.0e6 (1e6 m^3/s), *h_valid_area = area (m^2).  MOPS_ERR_INVALID, nothing
 * written: a null pointer, width or height < 2, a non-finite depth. */
mops_status mops_section_transport(int32_t width, int32_t height, const double* h_image0, const double* h_dist,
                                   double min_depth, double max_depth, double* h_sverdrup, double* h_valid_area);

/* ---- velocity gradient: vorticity, divergence, strain, Okubo-Weiss --------- */

/* Relative vorticity, horizontal divergence, strain rate and the Okubo-Weiss
 * parameter of every cell and level, from the field's vertex velocities (no
 * reference counterpart).  Wachspress interpolation is linear along polygon
 * edges, so in the planar approximation the Green-Gauss contour sum over a
 * cell's vertex velocities is the cell mean of the gradient of the field the
 * engine interpolates everywhere else.
 *
 * FP64, no contraction; every expression as written here, left to right; every
 * sum starts from 0.0 and runs over k = 0 .. n-1 in order; only + - * / and
 * sqrt.  Cell c: centre (cx, cy, cz) = cellCoord, n = nEdgesOnCell[c],
 * vertices p_k in verticesOnCell order, U_k the vertex velocity at level l
 * (cellVertexVelocity, the doubles mops_field_export returns).
 *   frame (convertXYZVelocityToENU's expressions):
 *     Rxy = sqrt(cx*cx + cy*cy), Rxyz = sqrt((cx*cx + cy*cy) + cz*cz),
 *     clon = cx/Rxy, slon = cy/Rxy, slat = cz/Rxyz, clat = Rxy/Rxyz,
 *     e = (-slon, clon, 0), nn = (-slat*clon, -slat*slon, clat);
 *     Rxy == 0 (a centre on the axis): e = (1, 0, 0), nn = (0, 1, 0) for
 *     cz > 0 and (0, -1, 0) otherwise
 *   plane:  d_k = p_k - c per component, xi_k = (d.x*e.x + d.y*e.y) + d.z*e.z,
 *     eta_k the same with nn
 *   geometry (indices modulo n):
 *     A2 = sum_k (xi_k*eta_k+1 - xi_k+1*eta_k)     (twice the signed area)
 *     gx_k = eta_k+1 - eta_k-1,  gy_k = xi_k-1 - xi_k+1
 *   level:  u_k = (U.x*e.x + U.y*e.y) + U.z*e.z, v_k the same with nn,
 *     ux = (sum_k u_k*gx_k) / A2,  uy = (sum_k u_k*gy_k) / A2,
 *     vx = (sum_k v_k*gx_k) / A2,  vy = (sum_k v_k*gy_k) / A2
 *     (the trapezoid Green-Gauss sum with its halves cancelled; the signed A2
 *     makes the result independent of the polygon's orientation)
 *   outputs:  vorticity = vx - uy, divergence = ux + vy, sn = ux - vy,
 *     ss = vx + uy, s2 = sn*sn + ss*ss, strain = sqrt(s2),
 *     okubo_weiss = s2 - vorticity*vorticity
 * All four are invariant under a rotation of the frame; the frame is fixed so
 * that the bits are.  A cell with n < 3, A2 == 0 or a non-finite A2 gets NaN
 * at every level; nothing else is special-cased (NaN in, NaN out).
 * Consequences: boundary vertices carry zero velocity (quirk Q10), so coastal
 * cells see a no-slip wall; levels below the bottom hold whatever the field
 * holds there.
 *
 * Each output is a device array [C*L] in the caller's cell order; any may be
 * NULL, not all.  Enqueues on `stream` and does not synchronise.
 * MOPS_ERR_INVALID before any device work: a null mesh or field, all outputs
 * NULL, a field of another mesh. */
mops_status mops_velocity_gradient(const mops_mesh* mesh, const mops_field* field, double* d_vorticity,
                                   double* d_divergence, double* d_strain, double* d_okubo_weiss, void* stream);

/* mops_cell_to_vertex_attr without the clamp: the same barycentric weights of
 * the three cellsOnVertex centres, b.x*a0 + b.y*a1 + b.z*a2, the caller's
 * vertex order, 0 at boundary vertices; negative results stay.  For signed
 * cell arrays such as mops_velocity_gradient's.  Device pointers [C*L] ->
 * [V*L]; enqueues on `stream`.  MOPS_ERR_INVALID for a null argument or a mesh
 * without cellsOnVertex. */
mops_status mops_cell_to_vertex_signed(const mops_mesh* mesh, const double* d_cell, double* d_vertex, void* stream);

/* ---- eddy census: Okubo-Weiss cores as connected components --------------- */

/* The cells whose Okubo-Weiss parameter lies below a threshold, split by the
 * sign of their vorticity, grouped into the connected components of the
 * cellsOnCell graph, and one table row per component (no reference
 * counterpart).  FP64, no contraction; every expression as written here, left
 * to right; every sum starts from 0.0; only + - * / and sqrt.  All cell arrays
 * are in the caller's cell order.
 *
 * mops_cell_area: area[c] = 0.5 * |A2|, A2 exactly the velocity-gradient
 * section's: the same frame, xi_k / eta_k and sum over k = 0 .. n-1 of
 * (xi_k*eta_k+1 - xi_k+1*eta_k); NaN where that section refuses the cell
 * (n < 3, A2 == 0, A2 not finite).  Device array [C]; enqueues on `stream`
 * and does not synchronise. */
mops_status mops_cell_area(const mops_mesh* mesh, double* d_area, void* stream);

/* mops_eddy_classify: for level l over arrays [C*L] as mops_velocity_gradient
 * writes them, class[c] = +1 if ow[c*L+l] < threshold and vort[c*L+l] > 0,
 * -1 if ow[c*L+l] < threshold and vort[c*L+l] < 0, 0 otherwise (NaN compares
 * false: a NaN cell is class 0).  int32 [C] on the device; enqueues on
 * `stream` and does not synchronise.  MOPS_ERR_INVALID for a null argument or
 * a level outside 0 .. L-1. */
mops_status mops_eddy_classify(const mops_mesh* mesh, const double* d_okubo_weiss, const double* d_vorticity,
                               int32_t level, double threshold, int32_t* d_class, void* stream);

/* mops_label_components: connected components of any int32 class[C].  Cells c
 * and d are joined if d is in cellsOnCell[c][0 .. nEdgesOnCell[c]-1] or c in
 * d's list, both are valid cells (an entry outside 1 .. nCells joins nothing)
 * and class[c] == class[d] != 0.  label[c] = the smallest cell index of c's
 * component; -1 for a class-0 cell.  The result is unique: its bytes do not
 * depend on the launch.  Union-find with 32-bit atomic minima over d_label as
 * the parent array (parent[x] <= x always, so every chase is bounded; no
 * kernel waits on another workgroup); after every round the host reads one
 * flag that a checking kernel raises while an edge still joins two roots, so
 * the entry SYNCHRONISES `stream` (once per round; one round is the rule) and
 * returns MOPS_ERR_UNSUPPORTED, never looping on, if 16 rounds do not
 * converge.  h_rounds (host, may be NULL) receives the rounds used:
 * informational.  Any maxEdges up to 20. */
mops_status mops_label_components(const mops_mesh* mesh, const int32_t* d_class, int32_t* d_label, int32_t* h_rounds,
                                  void* stream);

/* mops_eddy_count: membership.  Components of fewer than min_cells cells are
 * dropped, the rest numbered 0 .. E-1 in ascending order of their root cell
 * (their label); eddy_of_cell[c] = that index or -1 (int32 [C], device);
 * *h_n_eddies = E.  The numbering is formed on the host from a copy of the
 * labels: SYNCHRONISES `stream`.  MOPS_ERR_INVALID for a null argument,
 * min_cells < 1, or an array that is not a label array (a label is -1 or a
 * cell <= c that is its own label). */
mops_status mops_eddy_count(const mops_mesh* mesh, const int32_t* d_label, int32_t min_cells, int32_t* d_eddy_of_cell,
                            int64_t* h_n_eddies, void* stream);

/* mops_eddy_table: one row per eddy e, into HOST arrays [n_eddies] (h_centre
 * [n_eddies*3]); every sum runs over the eddy's cells in ascending cell index,
 * one lane per eddy:
 *   root = the smallest member, n_cells, polarity = class[root],
 *   area = sum area[c],  circulation = sum vort[c*L+l] * area[c],
 *   ow_min / core_cell: w = +inf, then for each c: if ow[c*L+l] < w take it
 *     (the first strict minimum; core_cell -1 if none),
 *   S = sum area[c] * cellCoord[c] per component,
 *   centre = S / sqrt((Sx*Sx + Sy*Sy) + Sz*Sz) per component.
 * d_eddy_of_cell and n_eddies as mops_eddy_count gave them; d_class [C],
 * d_area [C] (mops_cell_area), d_vorticity / d_okubo_weiss [C*L].
 * SYNCHRONISES `stream` (the member lists are sorted on the host).  With
 * n_eddies == 0 nothing is written.  MOPS_ERR_INVALID for a null argument, a
 * level outside 0 .. L-1, n_eddies outside 0 .. C or an eddy index outside
 * -1 .. n_eddies-1. */
mops_status mops_eddy_table(const mops_mesh* mesh, const int32_t* d_eddy_of_cell, int64_t n_eddies,
                            const int32_t* d_class, const double* d_area, const double* d_vorticity,
                            const double* d_okubo_weiss, int32_t level, int32_t* h_root, int32_t* h_n_cells,
                            int32_t* h_polarity, int32_t* h_core_cell, double* h_area, double* h_circulation,
                            double* h_ow_min, double* h_centre, void* stream);

/* ---- colour mapping ------------------------------------------------------ */

/* MOPS::SaveToPNG's pixel work (src/Common/ImageBuffer.hpp:91-136) on the
 * device, bit for bit, for the channels of an [height][width][4] float64
 * device image (16-byte aligned) selected by channel_mask (bit c = channel c;
 * 0 = x .. 3 = alpha, SaveToPNG's default).  Per channel: the float min / max
 * of static_cast<float>(v) over the non-NaN pixels, starting from FLT_MAX /
 * -FLT_MAX, then `if (min >= max) max = min + 1e-5f` (:101-111); per pixel a
 * NaN gives {0, 0, 0, 0}, any other value norm = (f - min) / (max - min) in
 * float, tinycolormap's Viridis lerp in double (tinycolormap.hpp:162-171) and
 * {(unsigned char)(c * 255.0) for r, g, b; 255} (:115-132).  d_rgba receives
 * one [height][width][4] uint8 plane per selected channel, in ascending
 * channel order.  h_minmax (optional, host, [4][2] floats) receives every
 * channel's {min, max} as used (the sign of a zero may differ from the
 * reference's; no colour depends on it).  An infinite pixel makes the
 * reference index its table from a NaN (undefined behaviour); here a NaN norm
 * takes table entry 0.  The table is include/mops_viridis.h.  Synchronises
 * `stream`. */
mops_status mops_colormap_rgba8(const double* d_image, int32_t width, int32_t height, int32_t channel_mask,
                                uint8_t* d_rgba, float* h_minmax, void* stream);

/* mops_colormap_rgba8 with host buffers (the caller of MOPS::SaveToPNG holds
 * an ImageBuffer on the host): uploads h_image, runs the kernels, downloads
 * the planes into h_rgba. */
mops_status mops_colormap_image(const double* h_image, int32_t width, int32_t height, int32_t channel_mask,
                                uint8_t* h_rgba, float* h_minmax, void* stream);

/* ---- particle density maps ------------------------------------------------ */

/* How many trajectory samples fell into each lat / lon pixel of a window, and
 * the sum of a value over them (no reference counterpart: its Vis_PathLines,
 * tutorial/pyMOPSAPI.py:132-289, draws one matplotlib line per trajectory).
 *
 * A density accumulator belongs to a window: width, height, min_lat, max_lat,
 * min_lon, max_lon of a mops_remap_cfg (the other members are ignored).  It is
 * [height][width][2] 64-bit integers {count, qsum}, zeroed by the caller.
 *
 * A point (x, y, z) with r = sqrt(x*x + y*y + z*z) is skipped when a
 * coordinate is not finite or r == 0 (the zero-filled record slots of a dead
 * particle).  Otherwise
 *   lat = asin(clamp(z / r, -1, 1)) * (180 / pi),  lon = atan2(y, x) * (180 / pi)
 * (mops_lines_geo's expressions), lon -= 360 * floor((lon - min_lon) / 360)
 * (so windows given as [-180, 180], [0, 360] or across the date line all
 * work), and the pixel is the reference's inverse pixel map
 * (GeoConverter.hpp:78-79, convertDegreeLatLonToPixel):
 *   fr = (max_lat - lat) / (max_lat - min_lat) * height
 *   fc = (lon - min_lon) / (max_lon - min_lon) * width
 * The point is inside iff 0 <= fr < height and 0 <= fc < width; its pixel is
 * (floor(fr), floor(fc)).  This inverts the remapping's pixel -> lat / lon
 * map, so a density image overlays a mops_remap_fixed_depth image of the same
 * settings.
 *
 * Value kinds: MOPS_DENSITY_COUNT -- no value, count += 1;
 * MOPS_DENSITY_SPEED -- v = sqrt(vx*vx + vy*vy + vz*vz) of the velocity found
 * at components 3..5 of the point's strides; MOPS_DENSITY_VALUES -- v read
 * from d_values.  With a value, a non-finite v or |v| >= 2^38 skips the point
 * entirely; otherwise q = llrint(v * 2^24) (ties to even) and the pixel gets
 * count += 1, qsum += q.  Fixed point because integer sums are exact and order
 * independent: the accumulator is the same bytes for every particle order,
 * launch split, reorder and compaction, like every other result of this
 * engine.  The resolution is 2^-24 (6e-8) in the value's unit.  qsum does not
 * overflow while count * |v| < 2^39 per pixel (|q| <= 2^62 per point, so a
 * single point always fits); past that bound it wraps. */
enum { MOPS_DENSITY_COUNT = 0, MOPS_DENSITY_SPEED = 1, MOPS_DENSITY_VALUES = 2 };

/* Bytes of a width x height accumulator (16 per pixel), or -1 for a size
 * below 1 or width * height >= 2^31.  Host only. */
int64_t mops_density_bytes(int32_t width, int32_t height);

/* Bins points (k, i), k in [k_begin, k_end), i in [0, n): component c of
 * point (k, i) is d_points[k*sk + i*si + c*sc].  A record slab [K][6][stride]
 * is sk = 6*stride, si = 1, sc = stride (columns n .. stride-1, shard padding,
 * are never read); a line array [n][P][3] is sk = 3, si = 3*P, sc = 1.
 * d_seeds (optional, [n][3]) is one more point per particle, binned by a
 * MOPS_DENSITY_COUNT call only: a seed carries no value, so a map of another
 * kind leaves it out and its mean stays the mean of the sampled values (a
 * chain passes the seeds for its first pair only, so no pair's first sample
 * is counted twice).  MOPS_DENSITY_VALUES reads the value of point (k, i) at
 * d_values[k*vk + i*vi] (row a of an attribute slab [K][n_attr][stride]:
 * d_values = slab + a*stride, vk = n_attr*stride, vi = 1).  One lane per
 * particle walks its records, keeps {pixel, count, qsum} in registers while
 * the pixel stays the same and adds them to d_accum with 64-bit integer
 * atomics when it changes.  Enqueues on `stream` and does not synchronise.
 * MOPS_ERR_INVALID before any device work for a null cfg, d_points or
 * d_accum, width or height < 1, width * height >= 2^31, non-finite or empty
 * lat / lon ranges, max_lon - min_lon > 360, a negative n or k_begin, a bad
 * kind, or MOPS_DENSITY_VALUES without d_values; MOPS_OK without a launch for
 * n == 0 or k_end <= k_begin. */
mops_status mops_density_accumulate(const mops_remap_cfg* cfg, int64_t n, int64_t k_begin, int64_t k_end,
                                    const double* d_points, int64_t sk, int64_t si, int64_t sc,
                                    const double* d_seeds, int32_t value_kind, const double* d_values, int64_t vk,
                                    int64_t vi, void* d_accum, void* stream);

/* An accumulator as an [height][width][4] float64 image (16-byte aligned):
 * {count, mean = (qsum / 2^24) / count, qsum / 2^24, 1}.  With nan_empty != 0
 * channels 0-2 of a pixel without samples are NaN, so mops_colormap_rgba8 /
 * SaveToPNG leave it transparent; otherwise channels 0 and 2 are 0 there and
 * the mean is NaN.  Enqueues on `stream` and does not synchronise; argument
 * checks as mops_density_accumulate's for cfg, d_accum and d_image. */
mops_status mops_density_image(const mops_remap_cfg* cfg, const void* d_accum, int32_t nan_empty, double* d_image,
                               void* stream);

/* ---- flow-map lattices and FTLE ------------------------------------------- */

/* The finite-time Lyapunov exponent of a flow map seeded on an image's pixel
 * lattice: where the flow pulls neighbouring particles apart (forward run) or
 * squeezes them together (backward run).  No reference counterpart.
 *
 * Lattice.  A window is width, height, min_lat, max_lat, min_lon, max_lon of a
 * mops_remap_cfg (the other members are ignored).  Seed (i, j) is the
 * fixed-depth remapping's pixel position with the same bits:
 *   (R * cos(lat_i) * cos(lon_j), R * cos(lat_i) * sin(lon_j), R * sin(lat_i)),
 * R = 6371010 (GeoConverter.hpp:107), the cos / sin values from the host
 * tables of mops_remap_tables(cfg, 0, ...).  Row major, [height*width][3];
 * row 0 is max_lat and row i - 1 lies north of row i; column j + 1 lies east
 * of column j.  So an FTLE image overlays a mops_remap_fixed_depth image and
 * a density image of the same settings.
 *
 * Validity.  Particle (i, j) is valid iff its seed and its last point are
 * finite, both have non-zero length, and death[i*W + j] < 0 when a death
 * array is given.
 *
 * FTLE of pixel (i, j).  FP64 with + - * / sqrt only up to lambda, no
 * contraction, every dot product summed as (x*x + y*y) + z*z, every length
 * the sqrt of such a sum:
 *   1. s = seed / |seed|, u = last / |last|, component-wise.
 *   2. East pair: jm = j-1 if that column exists and its particle is valid,
 *      else j; jp = j+1 likewise.  With wrap_lon != 0, j-1 and j+1 are taken
 *      modulo W.
 *   3. North pair: im = i-1 and ip = i+1 by the same rule; rows never wrap.
 *   4. The centre must be valid.  jm == jp or im == ip: the pixel is invalid.
 *   5. hE = |s[i,jp] - s[i,jm]|, hN = |s[im,j] - s[ip,j]|; either 0: invalid.
 *   6. a = (u[i,jp] - u[i,jm]) / hE, b = (u[im,j] - u[ip,j]) / hN.
 *   7. C11 = a.a, C12 = a.b, C22 = b.b (the Cauchy-Green tensor in the
 *      east / north frame of the seed; the lattice is orthogonal there).
 *   8. m = 0.5*(C11 + C22), d = 0.5*(C11 - C22), q = sqrt(d*d + C12*C12).
 *   9. lambda_max = m + q, lambda_min = m - q.
 *  10. ftle = log(lambda_max) / (2 * horizon); horizon > 0 in the caller's
 *      unit (the Python layer passes days).
 * The image is [height][width][4] = {ftle, lambda_max, lambda_min, 1}; an
 * invalid pixel is {NaN, NaN, NaN, 1}, which mops_colormap_rgba8 leaves
 * transparent.  The one-sided rule treats image edges, coast and dead
 * neighbours the same way: the difference is taken over the neighbours that
 * exist, with the spacing they have. */

/* The lattice's seeds into d_points [height*width][3] (device): the tables of
 * mops_remap_tables on the host, then the remapping's position kernel.
 * Synchronises `stream` (the uploaded tables are freed on return).
 * MOPS_ERR_INVALID, nothing written, for a null pointer, width or height < 1
 * or width * height >= 2^31. */
mops_status mops_flowmap_lattice(const mops_remap_cfg* cfg, double* d_points, void* stream);

/* The FTLE image of a flow map: d_seeds and d_last [height*width][3], d_death
 * [height*width] int32 (NULL = none), all in lattice (seed) order; d_image
 * [height][width][4] doubles, 16-byte aligned.  One lane per pixel.  Enqueues
 * on `stream` and does not synchronise.  MOPS_ERR_INVALID, nothing written,
 * for a null cfg, d_seeds, d_last or d_image, width or height < 1,
 * width * height >= 2^31, horizon <= 0 or a non-finite horizon. */
mops_status mops_ftle_image(const mops_remap_cfg* cfg, const double* d_seeds, const double* d_last,
                            const int32_t* d_death, double horizon, int32_t wrap_lon, double* d_image, void* stream);

/* ---- path integrals and LAVD ------------------------------------------------ */

/* The Lagrangian-averaged vorticity deviation: the time integral of
 * |vorticity - its horizontal mean| along a pathline (Haller et al. 2016), the
 * objective detector of coherent Lagrangian eddies.  No reference counterpart.
 * Three entries: the weighted mean of a cell field per level, the sum of
 * |sample| * weight over a particle's record slots, and the sum as an image.
 * The deviation itself (field - mean[l], one IEEE subtraction per element) and
 * its cell-to-vertex interpolation (mops_cell_to_vertex_signed) are the
 * caller's; the samples are the attribute channel's (mops_traj_advance_sampled
 * / _captured, mops_run_pathline_attrs).
 *
 * The rule is a rectangle rule.  Slot j of a pair's attribute slab is sampled
 * at the start of step (j+1)*ri - 1 (ri = record_t / delta_t steps) and stands
 * for one record interval: the integral of a pair is the sum over its slots
 * [0, K) of |sample| * |record_t| seconds.  A particle's slots after its death
 * hold the reference's zeros and add nothing; a consumer masks such a particle
 * through the death array of mops_path_integral_image.
 *
 * FP64, no contraction: every product below is rounded before its sum. */

/* The order of mops_level_mean's sum is part of the ABI: cells in groups of
 * this many, ascending within a group, then the groups ascending. */
#define MOPS_MEAN_GROUP 64

/* mean[l] = sum_c w[c]*x[c*L+l] / sum_c w[c] per level l over the counting
 * cells.  Mesh-free: n_cells = C >= 1, n_levels = L >= 1, d_field [C*L],
 * d_weight [C], d_mean [L], d_wsum [L], all device doubles.  Term (c, l) counts
 * iff isfinite(field[c*L+l]) and isfinite(weight[c]) and weight[c] > 0.
 *   group g = cells [64g, min(64g+64, C)):
 *     num_g = 0.0, den_g = 0.0; for each counting cell c of the group in
 *     ascending order: num_g = num_g + (w * x), den_g = den_g + w
 *   level:  num = 0.0, den = 0.0; for g ascending: num = num + num_g,
 *     den = den + den_g
 *   mean[l] = num / den, NaN where den == 0;  wsum[l] = den
 * A caller confines the mean to a window or basin by zeroing weights.  Lanes
 * run over the levels (a row of [C][L] is one coalesced read): one wave per
 * group and per 64 levels, then one block per level over the group partials.
 * The partials are a temporary allocation of the call, so the entry
 * SYNCHRONISES `stream` before it frees them.  MOPS_ERR_INVALID before any
 * device work: a null pointer, C < 1, L < 1 (or more than 2^31 - 1 groups). */
mops_status mops_level_mean(int64_t n_cells, int32_t n_levels, const double* d_field, const double* d_weight,
                            double* d_mean, double* d_wsum, void* stream);

/* One lane per slot i < n:
 *   id = d_ids ? d_ids[i] : i
 *   s = accum[id]
 *   for k = k_begin .. k_end-1:  s = s + (fabs(values[k*vk + i*vi]) * weight)
 *   accum[id] = s
 * d_ids (int32, NULL = identity) is a permutation of 0 .. n-1 (a ParticleSet's
 * slot -> particle array), so no two lanes write one element: no atomics, and
 * the bytes do not depend on the schedule.  The sum starts from the
 * accumulator, so a chain that calls the entry once per pair equals one long
 * ascending sum.  A non-finite sample makes the sum non-finite; it is not
 * filtered.  The strides are mops_density_accumulate's: row a of an attribute
 * slab [K][n_attr][stride] is d_values = slab + a*stride, vk = n_attr*stride,
 * vi = 1; finished lines [n][P] are vk = 1, vi = P.  d_accum [n] doubles.
 * Enqueues on `stream` and does not synchronise.  MOPS_ERR_INVALID before any
 * device work: a null d_values or d_accum, n < 1, k_begin < 0,
 * k_end < k_begin, a non-finite weight or weight < 0.  k_begin == k_end:
 * MOPS_OK, nothing written. */
mops_status mops_path_integral_abs(int64_t n, int64_t k_begin, int64_t k_end, const double* d_values, int64_t vk,
                                   int64_t vi, const int32_t* d_ids, double weight, double* d_accum, void* stream);

/* Pixel i of d_image [n*4] (16-byte aligned) = {s, s / horizon, 0, 1} with
 * s = accum[i]; {NaN, NaN, NaN, 1} where d_death (int32 [n], may be NULL) has
 * death[i] >= 0 or s is not finite.  horizon in the unit channel 1 is wanted
 * per (seconds for a mean |deviation| in 1/s).  Enqueues on `stream` and does
 * not synchronise.  MOPS_ERR_INVALID before any device work: a null d_accum or
 * d_image, n < 1, a horizon that is not finite and positive. */
mops_status mops_path_integral_image(int64_t n, const double* d_accum, const int32_t* d_death, double horizon,
                                     double* d_image, void* stream);

/* Identity of the engine build: a hash of the engine's sources, headers,
 * compiler flags and ROCm version, stamped at compile time (no reference
 * counterpart).  The Python loader refuses a library whose id differs from
 * the sources next to it, so a stale binary never runs. */
const char* mops_build_id(void);

/* ---- host convenience (the backend plug point) ------------------------- */

/* MOPS::Factory::StreamLine / PathLine (src/Common/MOPSFactory.h:27-39)
 * with host buffers: seeds [n*3]; depths [n] or NULL (then `depth` for all,
 * BuildEffectiveDepths, TrajectoryCommon.h:29-41); cells [n] in/out or NULL
 * (entries < 0 are located, as default_cell_id); outputs as
 * mops_traj_finalize plus the final positions (the caller's
 * sample_points update in MOPSApp::runPathLine, MOPSApp.cpp:287-290) and
 * death steps.  Any output pointer except h_points may be NULL. */
mops_status mops_run_trajectories(const mops_mesh* mesh, const mops_field* front, const mops_field* back,
                                  const mops_traj_cfg* cfg, int64_t n, const double* h_seeds,
                                  const float* h_depths, float depth, int32_t* h_cells, double* h_points,
                                  double* h_velocity, double* h_temperature, double* h_salinity,
                                  double* h_last_point, double* h_final_pos, float* h_final_depth,
                                  int32_t* h_death_step, void* stream);

/* mops_run_trajectories in layer mode (mops_traj_advance_layer): the slices of `layer` are made from `front`
 * and `back` (NULL = a streamline) inside the call; `depth` / h_depths are carried, because the records keep
 * their radius.  MOPS_ERR_INVALID before any device work for a layer outside [0, nVertLevels). */
mops_status mops_run_trajectories_layer(const mops_mesh* mesh, const mops_field* front, const mops_field* back,
                                        const mops_traj_cfg* cfg, int32_t layer, int64_t n, const double* h_seeds,
                                        const float* h_depths, float depth, int32_t* h_cells, double* h_points,
                                        double* h_velocity, double* h_temperature, double* h_salinity,
                                        double* h_last_point, double* h_final_pos, float* h_final_depth,
                                        int32_t* h_death_step, void* stream);

/* mops_run_trajectories / mops_run_trajectories_layer with the random walk (mops_diffusion above): the particle
 * ids are id_base + the seed index (d_id is not read).  kh == 0 is the call without it; MOPS_ERR_INVALID for a
 * negative or non-finite kh, MOPS_ERR_UNSUPPORTED for a depth-mode streamline with kh > 0, before any device work. */
mops_status mops_run_trajectories_diffuse(const mops_mesh* mesh, const mops_field* front, const mops_field* back,
                                          const mops_traj_cfg* cfg, const mops_diffusion* diffusion, int64_t n,
                                          const double* h_seeds, const float* h_depths, float depth,
                                          int32_t* h_cells, double* h_points, double* h_velocity,
                                          double* h_temperature, double* h_salinity, double* h_last_point,
                                          double* h_final_pos, float* h_final_depth, int32_t* h_death_step,
                                          void* stream);
mops_status mops_run_trajectories_layer_diffuse(const mops_mesh* mesh, const mops_field* front,
                                                const mops_field* back, const mops_traj_cfg* cfg, int32_t layer,
                                                const mops_diffusion* diffusion, int64_t n, const double* h_seeds,
                                                const float* h_depths, float depth, int32_t* h_cells,
                                                double* h_points, double* h_velocity, double* h_temperature,
                                                double* h_salinity, double* h_last_point, double* h_final_pos,
                                                float* h_final_depth, int32_t* h_death_step, void* stream);

/* mops_run_trajectories for a PathLine with the attribute channel
 * (Kernel::PathLine's current_attrs, MPASOVisualizerKernels.cpp:1288-1324,
 * :1431, :1453-1456, :1476-1478): the same arguments and outputs -- h_temperature
 * / h_salinity keep the velocity x / y of quirk Q9 -- plus n_attr (1..
 * MOPS_MAX_SAMPLE_ATTRS) pairs of DEVICE vertex attribute arrays [V*L]
 * (mops_cell_to_vertex_attr) and h_attr_lines [n_attr][n*(K+1)], the sampled
 * attribute lines after the reference's cleanup (mops_traj_finalize_attrs).
 * MOPS_ERR_UNSUPPORTED for back == NULL. */
mops_status mops_run_pathline_attrs(const mops_mesh* mesh, const mops_field* front, const mops_field* back,
                                    const mops_traj_cfg* cfg, int64_t n, const double* h_seeds,
                                    const float* h_depths, float depth, int32_t* h_cells, double* h_points,
                                    double* h_velocity, double* h_temperature, double* h_salinity,
                                    double* h_last_point, double* h_final_pos, float* h_final_depth,
                                    int32_t* h_death_step, int32_t n_attr, const double* const* d_front_attrs,
                                    const double* const* d_back_attrs, double* h_attr_lines, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOPS_TRAJ_H */
