"""Device-resident trajectory engine: thin owner objects over the C ABI.

``DeviceMesh`` / ``DeviceField`` keep the mesh and derived snapshots resident
in HBM (uploaded once, unlike the reference's HIP backend which re-uploads
every array per call, src/GPU/HIP/Kernel/MPASOVisualizerKernels.cu:1369-1431).
``ParticleSet`` is the SoA particle state + record slab as torch tensors
(torch is plumbing: allocation and streams), driven segment by segment by
``advance`` so records can be gathered while the next segment computes.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses

import numpy as np

from . import _lib as L


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _stream_handle(stream) -> C.c_void_p:
    if stream is None:
        return C.c_void_p(0)
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(int(stream.cuda_stream))


def _torch_stream(stream):
    """``stream`` (None, a raw handle or a torch stream) as a torch stream; None / 0 is the default stream."""
    import torch
    if stream is None or (isinstance(stream, int) and stream == 0):
        return torch.cuda.default_stream()
    if isinstance(stream, int):
        return torch.cuda.ExternalStream(stream)
    return stream


# The stream rule of the analysis and imaging entries: the library call and the temporaries' torch work run on
# ``stream`` when one is given, else on torch's current stream; results are allocated under torch's current stream.
def _current_or(stream, dev=None):
    """``stream``, or torch's current stream on ``dev`` (None: the current device): what an entry hands on as the
    ``stream=`` of the entries it calls, where None would mean stream 0."""
    import torch
    return stream if stream is not None else torch.cuda.current_stream(dev)


def _stream_or_current(stream, dev=None) -> C.c_void_p:
    """... as the handle the library takes."""
    return _stream_handle(_current_or(stream, dev))


def _on_stream(stream):
    """The context an entry's torch work runs in: ``stream`` when one is given, otherwise nothing."""
    if stream is None:
        return contextlib.nullcontext()
    import torch
    return torch.cuda.stream(_torch_stream(stream))


def _release_on(t, stream):
    """``t`` was allocated under torch's current stream and is released here while ``stream`` may still read it."""
    if stream is not None:
        t.record_stream(_torch_stream(stream))


def _tensor_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _image_size(width, height):
    width, height = int(width), int(height)
    if width < 1 or height < 1 or width * height >= 2 ** 31:
        raise ValueError(f"invalid image size {width} x {height}")
    return width, height


@dataclasses.dataclass
class TrajectoryConfig:
    """TrajectorySettings (src/Core/MPASOVisualizer.h:90-103)."""
    deltaT: int = 120
    simulationDuration: int = 86400
    recordT: int = 3600
    depth: float = 0.0
    direction: int = L.MOPS_FORWARD
    method: int = L.MOPS_EULER          # reference default (MPASOVisualizer.h:99); L.MOPS_RK4_RELOCATE: pathlines only
    layer: int | None = None            # the layer mode (mops_traj_advance_layer): advect within model layer `layer`
                                        # with w = 0; ``depth`` is still carried (records keep their radius).  There
                                        # MOPS_RK4_RELOCATE runs for streamlines too.  None: the depth mode
    diffusivity: float = 0.0            # horizontal eddy diffusivity Kh (m^2/s) of the random walk (mops_diffusion in
                                        # mops_traj.h); 0: none, the existing kernels
    seed: int = 0                       # ... its 64-bit Philox key
    epoch: int = 0                      # ... and the counter word the caller owns (a chain: the pair index)

    def diffusion(self, d_id=None, id_base: int = 0):
        """The mops_diffusion of this configuration (``d_id``: a device pointer to the particles' int32 ids), or
        None where ``diffusivity`` is 0.  ValueError for a negative or non-finite diffusivity."""
        kh = float(self.diffusivity)
        if not (kh >= 0.0) or not np.isfinite(kh):
            raise ValueError(f"diffusivity must be finite and >= 0, not {self.diffusivity!r}")
        if kh == 0.0:
            return None
        return L.Diffusion(kh, int(self.seed) & 0xFFFFFFFFFFFFFFFF, int(self.epoch) & 0xFFFFFFFF, int(id_base),
                           None if d_id is None else C.c_void_p(int(d_id)))

    def ctype(self) -> L.TrajCfg:
        return L.TrajCfg(int(self.deltaT), int(self.simulationDuration), int(self.recordT), int(self.direction),
                         int(self.method))

    @property
    def n_records(self) -> int:
        return int(self.simulationDuration // self.recordT) if self.recordT > 0 else 0

    @property
    def n_steps(self) -> int:
        return int(self.simulationDuration // self.deltaT) if self.deltaT > 0 else 0


class DeviceMesh:
    """MPAS-O mesh resident on the current HIP device (mops_mesh_create)."""

    def __init__(self, *, nCells, nVertices, maxEdges, nVertLevels, nEdgesOnCell, verticesOnCell, cellsOnCell,
                 cellsOnVertex, cellCoord, vertexCoord, stream=None):
        lib = L.load()
        self._arrays = dict(
            ne=np.ascontiguousarray(nEdgesOnCell, dtype=np.uint64),
            voc=np.ascontiguousarray(verticesOnCell, dtype=np.uint64),
            coc=np.ascontiguousarray(cellsOnCell, dtype=np.uint64),
            cov=None if cellsOnVertex is None else np.ascontiguousarray(cellsOnVertex, dtype=np.uint64),
            cc=np.ascontiguousarray(cellCoord, dtype=np.float64).reshape(-1),
            vc=np.ascontiguousarray(vertexCoord, dtype=np.float64).reshape(-1))
        a = self._arrays
        desc = L.MeshDesc(int(nCells), int(nVertices), int(maxEdges), int(nVertLevels), _ptr(a["ne"]), _ptr(a["voc"]),
                          _ptr(a["coc"]), _ptr(a["cov"]), _ptr(a["cc"]), _ptr(a["vc"]))
        h = C.c_void_p()
        L.check(lib.mops_mesh_create(C.byref(desc), _stream_handle(stream), C.byref(h)), "mops_mesh_create")
        self.handle = h
        self.nCells, self.nVertices, self.maxEdges, self.nVertLevels = int(nCells), int(nVertices), int(maxEdges), \
            int(nVertLevels)
        self._arrays = None  # the library copied everything

    @classmethod
    def from_mesh(cls, m, stream=None):
        dm = cls(nCells=m.nCells, nVertices=m.nVertices, maxEdges=m.maxEdges, nVertLevels=m.nVertLevels,
                 nEdgesOnCell=m.nEdgesOnCell, verticesOnCell=m.verticesOnCell, cellsOnCell=m.cellsOnCell,
                 cellsOnVertex=m.cellsOnVertex, cellCoord=m.cellCoord, vertexCoord=m.vertexCoord, stream=stream)
        ref = getattr(m, "refBottomDepth", None)  # the default depth range of remap_section
        dm.refBottomDepth = None if ref is None else np.array(ref, dtype=np.float64).reshape(-1)
        return dm

    def set_edges(self, nEdges, edgesOnCell, cellsOnEdge, edgeCoord, stream=None):
        """Upload the mesh's edges for the RBF velocity reconstruction (mops_mesh_set_edges)."""
        eoc = np.ascontiguousarray(edgesOnCell, dtype=np.uint64)
        coe = np.ascontiguousarray(cellsOnEdge, dtype=np.uint64)
        ec = np.ascontiguousarray(edgeCoord, dtype=np.float64).reshape(-1)
        L.check(L.load().mops_mesh_set_edges(self.handle, int(nEdges), _ptr(eoc), _ptr(coe), _ptr(ec),
                                             _stream_handle(stream)), "mops_mesh_set_edges")
        self.nEdges = int(nEdges)
        return self

    @property
    def nbytes(self) -> int:
        return int(L.load().mops_mesh_bytes(self.handle))

    def locate(self, d_points, d_cells, n: int, stream=None, d_hint=None):
        """Device pointers (ints) -> nearest cell ids (mops_locate_cells; with a
        candidate cell per point, mops_locate_cells_hinted -- same answer)."""
        if d_hint is None:
            L.check(L.load().mops_locate_cells(self.handle, n, C.c_void_p(d_points), C.c_void_p(d_cells),
                                               _stream_handle(stream)), "mops_locate_cells")
        else:
            L.check(L.load().mops_locate_cells_hinted(self.handle, n, C.c_void_p(d_points), C.c_void_p(d_hint),
                                                      C.c_void_p(d_cells), _stream_handle(stream)),
                    "mops_locate_cells_hinted")

    def tile_selection(self, stream=None):
        """``(flag, count)`` of the pathline launches on ``stream`` (None: stream 0) -- a blocking test / diagnostic
        entry (mops_traj_selection).  ``count``: how many launches on this mesh and stream ran the cooperative-tile
        selection so far; ``flag``: how the last of them fell once the stream has drained, 1 = the tile kernels,
        0 = the plain kernel, -1 while ``count`` is 0.  A launch with a processing order (``run_trajectories``), a
        streamline, MOPS_RK4_RELOCATE, the layer and diffusive entries and a mesh past maxEdges 7 never select."""
        flag, count = C.c_int32(-1), C.c_int64(0)
        L.check(L.load().mops_traj_selection(self.handle, _stream_handle(stream), C.byref(flag), C.byref(count)),
                "mops_traj_selection")
        return int(flag.value), int(count.value)

    def close(self):
        if getattr(self, "handle", None):
            L.load().mops_mesh_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceField:
    """One derived snapshot resident in HBM (mops_field_create[_derived])."""

    def __init__(self, mesh: DeviceMesh, handle):
        self.mesh = mesh
        self.handle = handle
        self._layers = {}     # layer -> its slice (layer_velocity), kept while the field lives
        self._layer_made = {}  # layer -> (stream handle the slice was written on, event recorded behind the write)
        self._stale = set()   # slices made before the last rebuild_from_device

    @classmethod
    def from_snapshot(cls, mesh: DeviceMesh, snap, stream=None, velocity: str = "zonal"):
        """``velocity``: "zonal" -- the cell velocity from zonal/meridional components (the reference's
        live path, MOPSApp.cpp:113); "rbf" -- reconstructed from ``snap.normalVelocity`` on the edges
        (MPASOSolution::calcCellCenterVelocity; the mesh needs ``DeviceMesh.set_edges``)."""
        lib = L.load()
        rbf = velocity == "rbf"
        keep = [np.ascontiguousarray(x, dtype=np.float64) if x is not None else None for x in
                (snap.layerThickness, snap.bottomDepth, getattr(snap, "surfaceHeight", None),
                 None if rbf else snap.zonalVelocity, None if rbf else snap.meridionalVelocity, snap.vertVelocityTop,
                 getattr(snap, "normalVelocity", None) if rbf else None)]
        desc = L.SnapshotDesc(int(snap.timestep), *[_ptr(x) for x in keep])
        h = C.c_void_p()
        L.check(lib.mops_field_create(mesh.handle, C.byref(desc), _stream_handle(stream), C.byref(h)),
                "mops_field_create")
        return cls(mesh, h)

    @staticmethod
    def _device_desc(snap: dict, timestep: int):
        def dp(k):
            t = snap.get(k)
            if t is None:
                return None
            if not (t.is_cuda and t.dtype.is_floating_point and t.element_size() == 8 and t.is_contiguous()):
                raise ValueError(f"{k}: expected a contiguous float64 CUDA tensor")
            return C.c_void_p(t.data_ptr())
        return L.SnapshotDesc(int(timestep), dp("layerThickness"), dp("bottomDepth"), dp("surfaceHeight"),
                              dp("zonalVelocity"), dp("meridionalVelocity"), dp("vertVelocityTop"),
                              dp("normalVelocity"))

    @classmethod
    def from_device_snapshot(cls, mesh: DeviceMesh, snap: dict, timestep: int = 0, stream=None):
        """Raw fields already in HBM (float64 CUDA tensors keyed like synth.Snapshot:
        layerThickness, bottomDepth, zonalVelocity, meridionalVelocity, vertVelocityTop;
        optional surfaceHeight) -- mops_field_create_device, no host round trip.
        Synchronises ``stream`` before returning."""
        desc = cls._device_desc(snap, timestep)
        h = C.c_void_p()
        L.check(L.load().mops_field_create_device(mesh.handle, C.byref(desc), _stream_handle(stream), C.byref(h)),
                "mops_field_create_device")
        return cls(mesh, h)

    def rebuild_from_device(self, snap: dict, timestep: int = 0, stream=None):
        """Re-derive this field in place from another snapshot's HBM tensors
        (mops_field_rebuild_device): asynchronous on ``stream``, stream-ordered
        after every earlier launch that reads this field there."""
        desc = self._device_desc(snap, timestep)
        L.check(L.load().mops_field_rebuild_device(self.handle, C.byref(desc), _stream_handle(stream)),
                "mops_field_rebuild_device")
        self._stale = set(self._layers)
        return self

    def layer_velocity(self, k: int, out=None, stream=None):
        """This snapshot's velocity at layer ``k`` as the compact per-vertex slice the layer kernels read
        (mops_field_layer_velocity): an opaque CUDA tensor of mops_layer_velocity_bytes bytes, written into
        ``out`` when given (a contiguous CUDA tensor of at least that size, 16-byte aligned).  Asynchronous on
        ``stream``; the field remembers the slice with an event recorded behind the write, so a layer run
        (``TrajectoryConfig.layer``) finds it and, on another stream, first waits for that event.  A caller that
        reads the returned tensor itself on another stream orders that read.  After ``rebuild_from_device`` the
        slice is made again."""
        import torch
        lib = L.load()
        nb = int(lib.mops_layer_velocity_bytes(self.mesh.handle))
        if out is None:
            out = torch.empty((max(nb, 8) // 8,), dtype=torch.float64, device=torch.device("cuda",
                                                                                        torch.cuda.current_device()))
        elif not (out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= nb):
            raise ValueError(f"layer_velocity: out must be a contiguous CUDA tensor of at least {nb} bytes")
        L.check(lib.mops_field_layer_velocity(self.mesh.handle, self.handle, int(k), C.c_void_p(out.data_ptr()),
                                              _stream_handle(stream)), "mops_field_layer_velocity")
        ts = _torch_stream(stream)
        ev = torch.cuda.Event()
        ev.record(ts)
        self._layers[int(k)] = out
        self._layer_made[int(k)] = (int(ts.cuda_stream), ev)
        self._stale.discard(int(k))
        return out

    def _layer_slice(self, k: int, stream):
        """The remembered slice of layer ``k`` for a launch on ``stream``: made on ``stream`` first where there is
        none or the field was rebuilt since; one written on another stream is waited for on ``stream`` (an event
        wait on the device, no host synchronisation)."""
        k = int(k)
        t = self._layers.get(k)
        if t is None or k in self._stale:
            return self.layer_velocity(k, out=t, stream=stream)
        made_on, ev = self._layer_made[k]
        ts = _torch_stream(stream)
        if int(ts.cuda_stream) != made_on:
            ts.wait_event(ev)
        return t

    @classmethod
    def from_derived(cls, mesh: DeviceMesh, vertex_ztop, vertex_vel, vertex_w=None, stream=None):
        lib = L.load()
        zt = np.ascontiguousarray(vertex_ztop, dtype=np.float64)
        ve = np.ascontiguousarray(vertex_vel, dtype=np.float64)
        w = None if vertex_w is None else np.ascontiguousarray(vertex_w, dtype=np.float64)
        h = C.c_void_p()
        L.check(lib.mops_field_create_derived(mesh.handle, _ptr(zt), _ptr(ve), _ptr(w), _stream_handle(stream),
                                              C.byref(h)), "mops_field_create_derived")
        return cls(mesh, h)

    def export(self, stream=None):
        V, Lv = self.mesh.nVertices, self.mesh.nVertLevels
        zt = np.empty(V * Lv); ve = np.empty(V * Lv * 3); w = np.empty(V * (Lv + 1))
        L.check(L.load().mops_field_export(self.handle, _ptr(zt), _ptr(ve), _ptr(w), _stream_handle(stream)),
                "mops_field_export")
        return zt, ve, w

    @property
    def nbytes(self) -> int:
        return int(L.load().mops_field_bytes(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            L.load().mops_field_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_trajectories(mesh: DeviceMesh, front: DeviceField, back: DeviceField | None, cfg: TrajectoryConfig,
                     seeds: np.ndarray, depths: np.ndarray | None = None, cells: np.ndarray | None = None,
                     stream=None, attrs=None):
    """Host-in/host-out StreamLine (back None) or PathLine (mops_run_trajectories).

    Returns a dict of numpy arrays shaped like the reference's finalized
    lines: points/velocity [N, K+1, 3], temperature/salinity [N, K+1],
    lastPoint [N, 3], plus final_pos, final_depth, death_step, cells.

    ``attrs`` (pathlines only, mops_run_pathline_attrs): a mapping name -> (front_vertex_tensor,
    back_vertex_tensor), at most 4 entries in the order given, each a [nVertices, nVertLevels] float64 CUDA
    tensor as ``cell_to_vertex_attr`` makes it.  The attributes are sampled along every pathline
    (Kernel::PathLine's current_attrs) and returned as ``attributes[name]`` [N, K+1]; ``temperature`` /
    ``salinity`` then hold the attributes of those NAMES (zeros where that name is not sampled) instead of
    the velocity x / y of quirk Q9.  None: the outputs above, unchanged.
    """
    lib = L.load()
    seeds = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 3)
    n = seeds.shape[0]
    K = cfg.n_records
    P = K + 1
    out = dict(points=np.empty((n, P, 3)), velocity=np.empty((n, P, 3)), temperature=np.empty((n, P)),
               salinity=np.empty((n, P)), lastPoint=np.empty((n, 3)), final_pos=np.empty((n, 3)),
               final_depth=np.empty(n, dtype=np.float32), death_step=np.empty(n, dtype=np.int32))
    dep = None if depths is None else np.ascontiguousarray(depths, dtype=np.float32)
    cl = np.full(n, -1, dtype=np.int32) if cells is None else np.ascontiguousarray(cells, dtype=np.int32).copy()
    c = cfg.ctype()
    dif = _diffusion_of(cfg, back, attrs, "run_trajectories")
    if dif is not None:  # the seed indices are the particle ids
        hb = None if back is None else back.handle
        tail = (n, _ptr(seeds), _ptr(dep), C.c_float(cfg.depth), _ptr(cl), _ptr(out["points"]), _ptr(out["velocity"]),
                _ptr(out["temperature"]), _ptr(out["salinity"]), _ptr(out["lastPoint"]), _ptr(out["final_pos"]),
                _ptr(out["final_depth"]), _ptr(out["death_step"]), _stream_handle(stream))
        if cfg.layer is not None:
            L.check(lib.mops_run_trajectories_layer_diffuse(mesh.handle, front.handle, hb, C.byref(c), int(cfg.layer),
                                                            C.byref(dif), *tail), "mops_run_trajectories_layer_diffuse")
        else:
            L.check(lib.mops_run_trajectories_diffuse(mesh.handle, front.handle, hb, C.byref(c), C.byref(dif), *tail),
                    "mops_run_trajectories_diffuse")
        out["cells"] = cl
        return out
    if cfg.layer is not None:
        _refuse_attrs_layer(attrs, "run_trajectories")
        st = lib.mops_run_trajectories_layer(mesh.handle, front.handle, None if back is None else back.handle,
                                             C.byref(c), int(cfg.layer), n, _ptr(seeds), _ptr(dep),
                                             C.c_float(cfg.depth), _ptr(cl), _ptr(out["points"]),
                                             _ptr(out["velocity"]), _ptr(out["temperature"]), _ptr(out["salinity"]),
                                             _ptr(out["lastPoint"]), _ptr(out["final_pos"]),
                                             _ptr(out["final_depth"]), _ptr(out["death_step"]),
                                             _stream_handle(stream))
        L.check(st, "mops_run_trajectories_layer")
        out["cells"] = cl
        return out
    if attrs is not None:
        _refuse_attrs_relocate(cfg, "run_trajectories")
        names = list(attrs)
        fa, ba = _attr_ptr_lists(mesh, [attrs[k][0] for k in names], [attrs[k][1] for k in names])
        lines = np.zeros((len(names), n, P))
        st = lib.mops_run_pathline_attrs(mesh.handle, front.handle, None if back is None else back.handle,
                                         C.byref(c), n, _ptr(seeds), _ptr(dep), C.c_float(cfg.depth), _ptr(cl),
                                         _ptr(out["points"]), _ptr(out["velocity"]), _ptr(out["temperature"]),
                                         _ptr(out["salinity"]), _ptr(out["lastPoint"]), _ptr(out["final_pos"]),
                                         _ptr(out["final_depth"]), _ptr(out["death_step"]), len(names), fa, ba,
                                         _ptr(lines), _stream_handle(stream))
        L.check(st, "mops_run_pathline_attrs")
        out["attributes"] = {k: lines[i] for i, k in enumerate(names)}
        for k in ("temperature", "salinity"):  # by name, never by position (map order puts salinity first)
            out[k] = out["attributes"][k].copy() if k in out["attributes"] else np.zeros((n, P))
        out["cells"] = cl
        return out
    st = lib.mops_run_trajectories(mesh.handle, front.handle, None if back is None else back.handle, C.byref(c), n,
                                   _ptr(seeds), _ptr(dep), C.c_float(cfg.depth), _ptr(cl), _ptr(out["points"]),
                                   _ptr(out["velocity"]), _ptr(out["temperature"]), _ptr(out["salinity"]),
                                   _ptr(out["lastPoint"]), _ptr(out["final_pos"]), _ptr(out["final_depth"]),
                                   _ptr(out["death_step"]), _stream_handle(stream))
    L.check(st, "mops_run_trajectories")
    out["cells"] = cl
    return out


MAX_SAMPLE_ATTRS = 4  # MOPS_MAX_SAMPLE_ATTRS


def _refuse_attrs_relocate(cfg: TrajectoryConfig, who: str):
    """Attribute sampling evaluates every RK4 stage in the step's cell: refused with MOPS_RK4_RELOCATE, before
    any launch (the C entries return MOPS_ERR_UNSUPPORTED)."""
    if int(cfg.method) == L.MOPS_RK4_RELOCATE:
        raise ValueError(f"{who}: attrs are not sampled with method MOPS_RK4_RELOCATE")


def _diffusion_of(cfg: TrajectoryConfig, back, attrs, who: str, d_id=None, id_base: int = 0):
    """The launch's mops_diffusion (None for diffusivity 0: the existing entries) after the refusals of the random
    walk, all before any launch: a negative or non-finite diffusivity, attribute sampling with it, and a depth-mode
    streamline with it."""
    dif = cfg.diffusion(d_id, id_base)
    if dif is None:
        return None
    if attrs is not None:
        raise ValueError(f"{who}: attrs are not sampled with diffusivity > 0")
    if cfg.layer is None and back is None:
        raise ValueError(f"{who}: a depth-mode streamline has no diffusion (use the layer mode, or a pathline)")
    return dif


def _refuse_attrs_layer(attrs, who: str):
    """The layer mode has no attribute channel yet: refused before any launch."""
    if attrs is not None:
        raise ValueError(f"{who}: attrs are not sampled in the layer mode (TrajectoryConfig.layer)")


def _layer_ptrs(front: DeviceField, back: DeviceField | None, layer: int, stream):
    """The two slice pointers of a layer launch on ``stream`` (the back one None for a streamline), ordered before
    it: made there, or waited for there (DeviceField._layer_slice)."""
    f = front._layer_slice(layer, stream)
    b = None if back is None else back._layer_slice(layer, stream)
    return C.c_void_p(f.data_ptr()), (None if b is None else C.c_void_p(b.data_ptr()))


def _attr_ptr_lists(mesh: DeviceMesh, front_list, back_list):
    """Two ctypes arrays of device pointers for the sampling entries' d_front_attrs / d_back_attrs."""
    na = len(front_list)
    if len(back_list) != na or not 1 <= na <= MAX_SAMPLE_ATTRS:
        raise ValueError(f"1..{MAX_SAMPLE_ATTRS} attributes, each with a front and a back vertex array")
    fa = (C.c_void_p * na)(*[_vertex_attr_ptr(mesh, t, f"front attribute {i}").value
                             for i, t in enumerate(front_list)])
    ba = (C.c_void_p * na)(*[_vertex_attr_ptr(mesh, t, f"back attribute {i}").value
                             for i, t in enumerate(back_list)])
    return fa, ba


class ParticleSet:
    """Device-resident SoA particle state + [K][6][n] record slab (torch tensors).

    This is the bench / multi-GPU driver: inputs stay in HBM, ``advance``
    launches the trajectory kernel over a step range on a given stream.
    """

    def __init__(self, mesh: DeviceMesh, seeds_xyz, depth: float | np.ndarray, cfg: TrajectoryConfig, device=None,
                 cells=None, use_order: bool = True, record_stride: int | None = None, n_attr: int = 0,
                 capture_slots: int = 0, id_base: int = 0):
        """``record_stride``: columns of the [K][6][stride] record slab (default n); a multi-GPU
        shard pads it to the largest shard so every rank's slab has one shape
        (distributed.RecordGather).  ``n_attr`` (pathlines, at most 4): also keep a zero-filled
        [K][n_attr][stride] attribute slab, which ``advance(..., attrs=...)`` samples into.
        ``capture_slots`` > 0 (with ``n_attr``): also a capture slab of that many window slots (32 B per
        particle and slot, mops_traj_capture_bytes); ``advance(attrs=)`` then runs one trajectory launch per
        window instead of one per sample step (mops_traj_advance_captured), with the same bytes.
        ``id_base``: the global id of this set's first seed -- the random walk (``cfg.diffusivity``) draws particle
        i's deviates for the id ``id_base + i``, so the parts of a split ensemble continue one numbering."""
        import torch
        self.use_order = use_order
        self.id_base = int(id_base)
        self.torch = torch
        dev = device or torch.device("cuda", torch.cuda.current_device())
        if isinstance(seeds_xyz, torch.Tensor):  # already resident: no host round trip
            s = seeds_xyz.to(device=dev, dtype=torch.float64).reshape(-1, 3).clone()
        else:
            s = torch.as_tensor(np.ascontiguousarray(seeds_xyz, dtype=np.float64).reshape(-1, 3), device=dev)
        self.n = int(s.shape[0])
        self.mesh = mesh
        self.cfg = cfg
        self.seeds = s.contiguous()
        self.x = s[:, 0].contiguous(); self.y = s[:, 1].contiguous(); self.z = s[:, 2].contiguous()
        if np.isscalar(depth):
            self.depth = torch.full((self.n,), float(depth), dtype=torch.float32, device=dev)
        else:
            self.depth = torch.as_tensor(np.asarray(depth, dtype=np.float32), device=dev).contiguous()
        self.death = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        if cells is None:
            self.cell = torch.empty((self.n,), dtype=torch.int32, device=dev)
            mesh.locate(self.seeds.data_ptr(), self.cell.data_ptr(), self.n,
                        stream=torch.cuda.current_stream(dev).cuda_stream)
        else:
            self.cell = torch.as_tensor(np.asarray(cells, dtype=np.int32), device=dev).contiguous()
        self.K = cfg.n_records
        self.rec_stride = self.n if record_stride is None else int(record_stride)
        if self.rec_stride < self.n:
            raise ValueError("record_stride below the particle count")
        self.records = torch.zeros((max(self.K, 1), 6, self.rec_stride), dtype=torch.float64, device=dev)
        self.n_attr = int(n_attr)
        if not 0 <= self.n_attr <= MAX_SAMPLE_ATTRS:
            raise ValueError(f"n_attr must be 0..{MAX_SAMPLE_ATTRS}")
        self.attr_records = None if self.n_attr == 0 else torch.zeros(
            (max(self.K, 1), self.n_attr, self.rec_stride), dtype=torch.float64, device=dev)
        self.capture_slots = int(capture_slots)
        if self.capture_slots < 0 or (self.capture_slots > 0 and self.n_attr == 0):
            raise ValueError("capture_slots must be >= 0 and needs n_attr > 0")
        self.capture = None
        if self.capture_slots > 0:
            nb = int(L.load().mops_traj_capture_bytes(self.n, self.capture_slots))
            if nb < 0:
                raise ValueError("capture slab size overflows")
            self.capture = torch.empty((max(nb, 1),), dtype=torch.uint8, device=dev)
        self.order = torch.empty((self.n,), dtype=torch.int32, device=dev)
        # slot -> particle index: with use_order the state is kept PHYSICALLY in
        # locality order (state loads/stores and record stores coalesce);
        # finalize() writes line ids[slot], so outputs keep the seed order
        self.ids = torch.arange(self.n, dtype=torch.int32, device=dev)
        self._compact_scratch = {}
        self._spare = {}  # second buffers for the permutations (_apply_order)
        self._n_live = {}  # (lo, hi) -> device int32: live particles at the front of the range after compact()
        self._written = False
        self._c = cfg.ctype()
        self.reorder(stream=torch.cuda.current_stream(dev).cuda_stream)

    def reorder(self, stream=None, records_written: int | None = None):
        """Locality order of the particles by their current cell (mops_order_particles), applied by permuting
        the SoA state (and the records once written: every slot -- a particle that died already holds
        the reference's zeros in its later slots -- or the first ``records_written`` when no particle can
        have died yet) so slot s holds particle ids[s]."""
        L.check(L.load().mops_order_particles(self.mesh.handle, self.n, C.c_void_p(self.cell.data_ptr()),
                                              C.c_void_p(self.order.data_ptr()), _stream_handle(stream)),
                "mops_order_particles")
        if not self.use_order or self.n == 0:
            return
        slots = self.records.shape[0] if self._written else 0
        if records_written is not None:
            slots = min(slots, max(0, int(records_written)))
        self._apply_order(self.order, 0, self.n, stream, slots)

    _STATE = (("x", 8), ("y", 8), ("z", 8), ("depth", 4), ("cell", 4), ("death", 4), ("ids", 4), ("seeds", 24))

    def _apply_order(self, order, lo: int, hi: int, stream, record_slots: int, attr_slots: int | None = None):
        """Permute slots [lo, hi) of the SoA state, seeds, slot ids and the first ``record_slots`` record
        slots (and the first ``attr_slots`` attribute slots, default the same count) by ``order`` (local
        indices) with one mops_permute_arrays launch into the spare buffers; the whole set swaps buffers, a
        sub-range is copied back with a second launch."""
        torch = self.torch
        n = hi - lo
        if n <= 0:
            return
        if isinstance(stream, int):
            s = torch.cuda.ExternalStream(stream) if stream else torch.cuda.current_stream(self.seeds.device)
        else:
            s = stream if stream is not None else torch.cuda.current_stream(self.seeds.device)
        names = [(k, e) for k, e in self._STATE] + ([("records", 8)] if record_slots > 0 else [])
        if attr_slots is None:
            attr_slots = record_slots
        elif self.attr_records is not None:
            attr_slots = min(int(attr_slots), self.attr_records.shape[0])
        if attr_slots > 0 and self.attr_records is not None:
            names.append(("attr_records", 8))  # (attribute slot k is written at the steps that write record slot k)
        with torch.cuda.stream(s):
            for k, _ in names:
                if k not in self._spare:  # (allocated on first use, then kept)
                    # (the attribute slab's second buffer is zero-filled like the first, see compact)
                    self._spare[k] = (torch.zeros_like if k == "attr_records" else torch.empty_like)(getattr(self, k))

        def desc(src, dst, name, eb):
            if name == "records":
                return L.PermArray(src.data_ptr() + 8 * lo, dst.data_ptr() + 8 * lo, 8, int(record_slots) * 6,
                                   self.rec_stride)
            if name == "attr_records":
                return L.PermArray(src.data_ptr() + 8 * lo, dst.data_ptr() + 8 * lo, 8,
                                   int(attr_slots) * self.n_attr, self.rec_stride)
            return L.PermArray(src.data_ptr() + eb * lo, dst.data_ptr() + eb * lo, eb, 1, n)

        lib = L.load()
        arr = (L.PermArray * len(names))(*[desc(getattr(self, k), self._spare[k], k, e) for k, e in names])
        L.check(lib.mops_permute_arrays(n, C.c_void_p(order.data_ptr() + 4 * lo), len(names), arr, _stream_handle(s)),
                "mops_permute_arrays")
        if lo == 0 and hi == self.n:
            for k, _ in names:  # the gathered copies become the state
                cur = getattr(self, k)
                setattr(self, k, self._spare[k])
                self._spare[k] = cur
        else:
            back = (L.PermArray * len(names))(*[desc(self._spare[k], getattr(self, k), k, e) for k, e in names])
            L.check(lib.mops_permute_arrays(n, None, len(names), back, _stream_handle(s)), "mops_permute_arrays")

    def original(self, t, stream=None):
        """A per-slot tensor back in the particles' seed order.  Torch work (an allocation and an indexed store) on
        ``stream`` -- None, a raw handle or a torch stream; default torch's current one -- without a host
        synchronisation: ``t`` and the slot ids must be ordered on that stream, as an ``advance`` / ``compact``
        there leaves them.  The result is allocated under that stream, so it may be dropped while the stream still
        reads it."""
        torch = self.torch
        with _on_stream(stream):
            out = torch.empty_like(t)
            out[self.ids.long()] = t
        return out

    def compact(self, lo: int, hi: int, stream, records_written: int, attr_slots_written: int | None = None):
        """Dead-particle compaction of slots [lo, hi) on ``stream`` (mops_order_particles_live):
        live particles in the Morton order of their current cell first, dead ones after them, so
        the next launches run full waves of live lanes and all-dead waves exit at once.  The SoA
        state, seeds, slot ids and the first ``records_written`` record slots are permuted with
        them; the dead particles' later slots are cleared again where they land
        (mops_records_clear_dead: they hold no samples, the live particles' ones are written by
        the next launches).  Results are unchanged (every particle is independent, finalize
        writes each slot's line at its id).  Re-entrant across disjoint ranges on different
        streams (each range has its own scratch).

        A set with an attribute slab needs ``attr_slots_written``: the first that many attribute slots move
        with their particles (at a step boundary s0 the records' count, min(K, s0 // period + 1)).  The
        attribute slab needs no clearing pass: it is zero-filled at ``reset`` / ``reseed`` and a dead lane
        writes nothing, so every slot not yet written is zero in every column, wherever a particle lands.
        That holds for the permutation's second buffer too, which becomes the slab when the whole set is
        compacted: it is allocated zero-filled and zero-filled again at ``reset`` / ``reseed``, and between
        those only slots below a written count -- which every later permutation overwrites -- are stored to it."""
        torch = self.torch
        if self.attr_records is not None and attr_slots_written is None:
            raise ValueError("compact: not supported for a particle set with an attribute slab")
        n = hi - lo
        if n <= 1:
            return
        lib = L.load()
        s = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream))
        key = (lo, hi)
        if key not in self._compact_scratch:
            nb = int(lib.mops_order_scratch_bytes(n))
            if nb <= 0:
                raise L.MopsError("mops_order_scratch_bytes failed")
            with torch.cuda.stream(s):
                self._compact_scratch[key] = torch.empty((nb,), dtype=torch.uint8, device=self.seeds.device)
        scratch = self._compact_scratch[key]
        if key not in self._n_live:
            with torch.cuda.stream(s):
                self._n_live[key] = torch.zeros((1,), dtype=torch.int32, device=self.seeds.device)
        e4 = 4
        L.check(lib.mops_order_particles_live(self.mesh.handle, n, C.c_void_p(self.cell.data_ptr() + e4 * lo),
                                              C.c_void_p(self.death.data_ptr() + e4 * lo),
                                              C.c_void_p(self.order.data_ptr() + e4 * lo),
                                              C.c_void_p(self._n_live[key].data_ptr()),
                                              C.c_void_p(scratch.data_ptr()), scratch.numel(), _stream_handle(s)),
                "mops_order_particles_live")
        kw = min(int(records_written), self.records.shape[0])
        self._apply_order(self.order, lo, hi, s, kw,
                          None if self.attr_records is None else max(0, int(attr_slots_written)))
        L.check(lib.mops_records_clear_dead(n, C.c_void_p(self._n_live[key].data_ptr()), kw, self.K,
                                            C.c_void_p(self.records.data_ptr() + 8 * lo), self.rec_stride,
                                            _stream_handle(s)), "mops_records_clear_dead")
        return self._n_live[key]

    def set_config(self, cfg: TrajectoryConfig):
        """Run the next call with ``cfg`` (a chained pair's own simulationDuration: its step and
        record counts and alpha ramp); its records must fit the slab allocated at creation."""
        if cfg.n_records > self.records.shape[0]:
            raise ValueError(f"{cfg.n_records} records do not fit the slab of {self.records.shape[0]}")
        self.cfg = cfg
        self._c = cfg.ctype()
        self.K = cfg.n_records

    def swap_records(self, slab):
        """Install another [K][6][stride] slab as the record buffer and return the current one
        (RecordGather: the slab just completed is gathered while the next call writes this one)."""
        if tuple(slab.shape) != tuple(self.records.shape) or slab.dtype != self.records.dtype:
            raise ValueError("record slab shape/dtype mismatch")
        old, self.records = self.records, slab
        return old

    def swap_attr_records(self, slab):
        """``swap_records`` for the attribute slab [K][n_attr][stride] (a chain's deferred assembly); the
        installed slab must be zero-filled, as ``reseed`` leaves it."""
        if self.attr_records is None:
            raise ValueError("swap_attr_records: the particle set has no attribute slab")
        if tuple(slab.shape) != tuple(self.attr_records.shape) or slab.dtype != self.attr_records.dtype:
            raise ValueError("attribute slab shape/dtype mismatch")
        old, self.attr_records = self.attr_records, slab
        return old

    def reset(self, depth=None):
        self.x.copy_(self.seeds[:, 0]); self.y.copy_(self.seeds[:, 1]); self.z.copy_(self.seeds[:, 2])
        if depth is not None:
            self.depth.fill_(float(depth))
        self.death.fill_(-1)
        self._written = False  # (records: every slot is rewritten by the launches from step 0)
        if self.attr_records is not None:
            self.attr_records.zero_()  # (a particle that never reaches a slot leaves its zero there)
            if "attr_records" in self._spare:
                self._spare["attr_records"].zero_()  # (the slab after the next whole-set permutation)

    def reseed(self, seeds, depth, stream=None, hint_cells: bool = False):
        """Start a new run from device-resident seeds [n,3] (f64) and depth (scalar
        or [n] f32): state <- seeds, death cleared (records need no clearing), seed cells
        located (the reference's calcInWhichCells per run) and re-ordered.
        ``hint_cells``: the seeds continue this set's particles (a chained pair),
        so each particle's current cell seeds the exact locate (same answer)."""
        torch = self.torch
        s = seeds.reshape(-1, 3)
        if int(s.shape[0]) != self.n:
            raise ValueError("reseed: particle count changed")
        h = stream if stream is not None else torch.cuda.current_stream(self.seeds.device).cuda_stream
        # slot order -> particle order, before the ids reset (same stream as the copies below)
        hint = self.original(self.cell) if hint_cells else None
        self.seeds.copy_(s)
        self.ids.copy_(torch.arange(self.n, dtype=torch.int32, device=self.ids.device))
        self.x.copy_(s[:, 0]); self.y.copy_(s[:, 1]); self.z.copy_(s[:, 2])
        if isinstance(depth, torch.Tensor):
            self.depth.copy_(depth.to(torch.float32))
        else:
            self.depth.fill_(float(np.float32(depth)))
        self.death.fill_(-1)
        self._written = False
        if self.attr_records is not None:
            self.attr_records.zero_()
            if "attr_records" in self._spare:
                self._spare["attr_records"].zero_()
        self.mesh.locate(self.seeds.data_ptr(), self.cell.data_ptr(), self.n, stream=h,
                         d_hint=None if hint is None else hint.data_ptr())
        self.reorder(stream=h)

    def particles(self) -> L.Particles:
        return L.Particles(self.n, self.x.data_ptr(), self.y.data_ptr(), self.z.data_ptr(), self.depth.data_ptr(),
                           self.cell.data_ptr(), self.death.data_ptr(), None, None)  # physically ordered

    def advance(self, front: DeviceField, back: DeviceField | None, step_begin: int, step_end: int, stream=None,
                live_count=None, attrs=None):
        """Launch steps [step_begin, step_end) over every slot; ``live_count``: the device live count
        compact(0, n) returned (only the leading live slots are spread over the XCDs).  ``attrs``: a pair
        (front_list, back_list) of n_attr vertex attribute tensors each (``cell_to_vertex_attr``) -- the
        range's sample steps are sampled into the attribute slab (mops_traj_advance_sampled); positions,
        records, depths and death steps are those of the plain call.  In the layer mode (``cfg.layer``) the
        fields' slices of that layer are made on ``stream`` where they are missing or stale; one made earlier on
        another stream (``DeviceField.layer_velocity``) is waited for on ``stream`` through its event."""
        p = self.particles() if live_count is None else self._sub_particles(0, self.n, live_count)
        dif = _diffusion_of(self.cfg, back, attrs, "advance", self.ids.data_ptr(), self.id_base)
        if dif is not None:
            if self.attr_records is not None:
                raise ValueError("advance: diffusivity > 0 does not run a particle set with an attribute slab")
            self._advance_diffuse(front, back, p, 0, int(step_begin), int(step_end), dif, None, stream)
            self._written = True
            return
        if self.cfg.layer is not None:  # the layer mode: the mesh and the two snapshots' slices only
            _refuse_attrs_layer(attrs, "advance")
            if self.attr_records is not None:
                raise ValueError("advance: the layer mode does not run a particle set with an attribute slab")
            fl, bl = _layer_ptrs(front, back, self.cfg.layer, stream)
            st = L.load().mops_traj_advance_layer(self.mesh.handle, fl, bl, C.byref(self._c), C.byref(p),
                                                  int(step_begin), int(step_end),
                                                  C.c_void_p(self.records.data_ptr()), self.rec_stride,
                                                  _stream_handle(stream))
            L.check(st, "mops_traj_advance_layer")
            self._written = True
            return
        if attrs is not None:
            _refuse_attrs_relocate(self.cfg, "advance")
            if self.attr_records is None or len(attrs[0]) != self.n_attr:
                raise ValueError("advance: attrs needs a particle set created with n_attr = the number of attributes")
            fa, ba = _attr_ptr_lists(self.mesh, list(attrs[0]), list(attrs[1]))
            self._advance_attrs(front, back, p, 0, int(step_begin), int(step_end), fa, ba, stream)
            self._written = True
            return
        st = L.load().mops_traj_advance(self.mesh.handle, front.handle, None if back is None else back.handle,
                                        C.byref(self._c), C.byref(p), int(step_begin), int(step_end),
                                        C.c_void_p(self.records.data_ptr()), self.rec_stride, _stream_handle(stream))
        L.check(st, "mops_traj_advance")
        self._written = True

    def _advance_diffuse(self, front, back, p, lo: int, step_begin: int, step_end: int, dif, layer_ptrs, stream):
        """The advance with the random walk of the slots ``p`` describes, which begin at slot ``lo`` (``dif``: the
        mops_diffusion whose id pointer is already that part's): mops_traj_advance_layer_diffuse in the layer mode
        (``layer_ptrs``: the slices, made here when None), else mops_traj_advance_diffuse."""
        lib = L.load()
        rec = C.c_void_p(self.records.data_ptr() + 8 * lo)
        if self.cfg.layer is not None:
            fl, bl = layer_ptrs if layer_ptrs is not None else _layer_ptrs(front, back, self.cfg.layer, stream)
            L.check(lib.mops_traj_advance_layer_diffuse(self.mesh.handle, fl, bl, C.byref(self._c), C.byref(p),
                                                        C.byref(dif), step_begin, step_end, rec, self.rec_stride,
                                                        _stream_handle(stream)), "mops_traj_advance_layer_diffuse")
        else:
            L.check(lib.mops_traj_advance_diffuse(self.mesh.handle, front.handle, None if back is None else back.handle,
                                                  C.byref(self._c), C.byref(p), C.byref(dif), step_begin, step_end, rec,
                                                  self.rec_stride, _stream_handle(stream)), "mops_traj_advance_diffuse")

    def _advance_attrs(self, front, back, p, lo: int, step_begin: int, step_end: int, fa, ba, stream):
        """The sampled advance of the slots ``p`` describes, which begin at slot ``lo``: through the capture
        slab when the set has one (mops_traj_advance_captured; the part's own piece of it, 32 B x
        capture_slots per slot), else with a launch boundary per sample step (mops_traj_advance_sampled)."""
        lib = L.load()
        bh = None if back is None else back.handle
        rec = C.c_void_p(self.records.data_ptr() + 8 * lo)
        slab = C.c_void_p(self.attr_records.data_ptr() + 8 * lo)
        if self.capture is not None:
            L.check(lib.mops_traj_advance_captured(
                self.mesh.handle, front.handle, bh, C.byref(self._c), C.byref(p), step_begin, step_end, rec,
                self.rec_stride, self.n_attr, fa, ba, slab, self.rec_stride,
                C.c_void_p(self.capture.data_ptr() + 32 * self.capture_slots * lo), self.capture_slots,
                _stream_handle(stream)), "mops_traj_advance_captured")
        else:
            L.check(lib.mops_traj_advance_sampled(
                self.mesh.handle, front.handle, bh, C.byref(self._c), C.byref(p), step_begin, step_end, rec,
                self.rec_stride, self.n_attr, fa, ba, slab, self.rec_stride, _stream_handle(stream)),
                "mops_traj_advance_sampled")

    def _sub_particles(self, lo: int, hi: int, live_count=None) -> L.Particles:
        """Slots [lo, hi) as a launch argument; ``live_count``: the range's device live count after a
        compaction (only its leading live slots are launched over the XCDs)."""
        e4, e8 = 4, 8
        return L.Particles(hi - lo, self.x.data_ptr() + e8 * lo, self.y.data_ptr() + e8 * lo,
                           self.z.data_ptr() + e8 * lo, self.depth.data_ptr() + e4 * lo,
                           self.cell.data_ptr() + e4 * lo, self.death.data_ptr() + e4 * lo, None,
                           None if live_count is None else live_count.data_ptr())

    def advance_pipelined(self, front: DeviceField, back: DeviceField | None, step_begin: int, step_end: int,
                          streams, chunks: int, timing=None, compact: bool = False, compact_priority: bool = False,
                          attrs=None):
        """``advance`` split into len(streams) contiguous particle parts (whole waves), each on its own
        stream, and ``chunks`` step ranges per part, enqueued chunk-major.

        One launch over all particles ends in a partial round of waves: 1e6 particles are 15625
        waves over 3072 resident slots (5.09 rounds), so the last 9% of a round runs alone for a
        whole wave lifetime.  Shorter launches on several streams let one part's tail overlap the
        other parts' next chunk (kernel boundaries order each part's chunks; results are
        identical for any split: every particle is independent and records are indexed by
        absolute step).  The streams must already be ordered after the state's producers; the
        caller joins them afterwards.  ``timing`` receives (start, end) events per launch.
        ``compact``: before every chunk but the first, each part is re-sorted on its own stream
        with its dead particles last (``compact``): RK4 kills particles at cell crossings
        (quirk Q1, half of them in a day at config 2), and a wave keeps its slots until its
        last live lane finishes.  ``attrs`` (as ``advance``; required for a set with an attribute slab):
        each part runs the sampled advance on its own stream, into its columns of the attribute slab and
        its own piece of the capture slab; a compaction moves the attribute slots written so far."""
        torch = self.torch
        fl = bl = None
        diffuse = _diffusion_of(self.cfg, back, attrs, "advance_pipelined") is not None
        if diffuse and self.attr_records is not None:
            raise ValueError("advance_pipelined: diffusivity > 0 does not run a particle set with an attribute slab")
        if self.cfg.layer is not None:
            _refuse_attrs_layer(attrs, "advance_pipelined")
            if self.attr_records is not None:
                raise ValueError("advance_pipelined: the layer mode does not run a particle set with an attribute "
                                 "slab")
            # (made on the first part's stream where missing; every part's stream waits for the slices' events)
            for st in (list(streams) or [None]):
                fl, bl = _layer_ptrs(front, back, self.cfg.layer, st)
        if self.attr_records is not None and attrs is None:
            raise ValueError("advance_pipelined: not supported for a particle set with an attribute slab")
        fa = ba = None
        if attrs is not None:
            _refuse_attrs_relocate(self.cfg, "advance_pipelined")
            if self.attr_records is None or len(attrs[0]) != self.n_attr:
                raise ValueError("advance_pipelined: attrs needs a particle set created with n_attr = the number "
                                 "of attributes")
            fa, ba = _attr_ptr_lists(self.mesh, list(attrs[0]), list(attrs[1]))
        nparts = max(1, len(streams))
        pb = self.part_bounds(nparts)
        span = int(step_end) - int(step_begin)
        chunks = max(1, min(int(chunks), span))
        tb = [int(step_begin) + span * k // chunks for k in range(chunks + 1)]
        period = self.record_period(pathline=back is not None)
        lib = L.load()
        if compact and chunks > 1 and compact_priority:
            # optionally the re-sort runs on a high-priority stream per part: its short kernels otherwise
            # queue behind the other parts' trajectory waves (measured: the key kernel then waits ~5 ms)
            dev = self.seeds.device
            if getattr(self, "_hp_streams", None) is None or len(self._hp_streams) < nparts:
                prio = torch.cuda.Stream.priority_range()[1]  # the numerically lowest = highest priority
                self._hp_streams = [torch.cuda.Stream(device=dev, priority=prio) for _ in range(nparts)]
        for t in range(chunks):
            for k in range(nparts):
                lo, hi = pb[k], pb[k + 1]
                if hi <= lo or tb[t + 1] <= tb[t]:
                    continue
                st = streams[k]
                if compact and t > 0:
                    # slots written so far: slot 0 (step-0 pre-writes) .. the last completed record
                    nrec = min(self.K, tb[t] // period + 1) if period else 1
                    if compact_priority:
                        hp = self._hp_streams[k]
                        hp.wait_stream(st)
                        self.compact(lo, hi, hp, records_written=nrec,
                                     attr_slots_written=None if attrs is None else nrec)
                        st.wait_stream(hp)
                    else:
                        self.compact(lo, hi, st, records_written=nrec,
                                     attr_slots_written=None if attrs is None else nrec)
                if timing is not None:
                    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                p = self._sub_particles(lo, hi, self._n_live.get((lo, hi)) if (compact and t > 0) else None)
                if attrs is not None:
                    self._advance_attrs(front, back, p, lo, tb[t], tb[t + 1], fa, ba, st)
                elif diffuse:  # (the part's ids: the id pointer offset by its first slot)
                    dif = self.cfg.diffusion(self.ids.data_ptr() + 4 * lo, self.id_base)
                    self._advance_diffuse(front, back, p, lo, tb[t], tb[t + 1], dif,
                                          None if fl is None else (fl, bl), st)
                elif fl is not None:
                    rc = lib.mops_traj_advance_layer(self.mesh.handle, fl, bl, C.byref(self._c), C.byref(p), tb[t],
                                                     tb[t + 1], C.c_void_p(self.records.data_ptr() + 8 * lo),
                                                     self.rec_stride, _stream_handle(st))
                    L.check(rc, "mops_traj_advance_layer")
                else:
                    rc = lib.mops_traj_advance(self.mesh.handle, front.handle, None if back is None else back.handle,
                                               C.byref(self._c), C.byref(p), tb[t], tb[t + 1],
                                               C.c_void_p(self.records.data_ptr() + 8 * lo), self.rec_stride,
                                               _stream_handle(st))
                    L.check(rc, "mops_traj_advance")
                if timing is not None:
                    e1.record(st)
                    timing.append((e0, e1))
        self._written = True

    def part_bounds(self, nparts: int):
        """Slot bounds of ``nparts`` contiguous particle parts in whole waves (advance_pipelined)."""
        nparts = max(1, int(nparts))
        waves = -(-self.n // 64)
        return [min(self.n, 64 * (waves * k // nparts)) for k in range(nparts + 1)]

    def record_period(self, pathline: bool) -> int:
        import math
        if pathline:
            return int(self.cfg.recordT // self.cfg.deltaT)
        return int(self.cfg.recordT // math.gcd(int(self.cfg.recordT), int(self.cfg.deltaT)))

    def last_points(self, stream=None):
        """Each particle's cleaned last point in seed order (mops_traj_last_points): finalize's lastPoint
        without the lines.  One launch on ``stream`` (default the null stream) without a host synchronisation;
        no torch work beyond allocating the result under torch's current stream."""
        torch = self.torch
        last = torch.empty((self.n, 3), dtype=torch.float64, device=self.seeds.device)
        L.check(L.load().mops_traj_last_points(self.n, self.K, C.c_void_p(self.seeds.data_ptr()),
                                               C.c_void_p(self.records.data_ptr()), self.rec_stride,
                                               C.c_void_p(self.ids.data_ptr()), C.c_void_p(last.data_ptr()),
                                               _stream_handle(stream)), "mops_traj_last_points")
        return last

    def _attr_lines(self, n, seeds_ptr, records_ptr, attr_ptr, ids_ptr, stream):
        """The attribute lines [n_attr, n, K + 1] of n slots (mops_traj_finalize_attrs)."""
        out = self.torch.empty((self.n_attr, n, self.K + 1), dtype=self.torch.float64, device=self.seeds.device)
        L.check(L.load().mops_traj_finalize_attrs(n, self.K, C.c_void_p(seeds_ptr), C.c_void_p(records_ptr),
                                                  self.rec_stride, self.n_attr, C.c_void_p(attr_ptr), self.rec_stride,
                                                  None if ids_ptr is None else C.c_void_p(ids_ptr),
                                                  C.c_void_p(out.data_ptr()), _stream_handle(stream)),
                "mops_traj_finalize_attrs")
        return out

    def finalize_from(self, seeds, ids, records, pathline: bool, stream=None, attr_records=None):
        """finalize over another set's seeds, slot ids and record slab (a chain's deferred assembly: the
        buffers of a finished pair while this set runs the next); with that set's attribute slab
        (``attr_records``) also ``attributes`` [n_attr, n, K + 1]."""
        torch = self.torch
        dev = self.seeds.device
        P = self.K + 1
        pts = torch.empty((self.n, P, 3), dtype=torch.float64, device=dev)
        vel = torch.empty_like(pts)
        tmp = torch.empty((self.n, P), dtype=torch.float64, device=dev)
        sal = torch.empty_like(tmp)
        L.check(L.load().mops_traj_finalize(self.n, self.K, C.c_void_p(seeds.data_ptr()), C.c_void_p(records.data_ptr()),
                                            self.rec_stride, 1 if pathline else 0, C.c_void_p(ids.data_ptr()),
                                            C.c_void_p(pts.data_ptr()), C.c_void_p(vel.data_ptr()),
                                            C.c_void_p(tmp.data_ptr()), C.c_void_p(sal.data_ptr()), None,
                                            _stream_handle(stream)), "mops_traj_finalize")
        out = dict(points=pts, velocity=vel, temperature=tmp, salinity=sal)
        if attr_records is not None:
            out["attributes"] = self._attr_lines(self.n, seeds.data_ptr(), records.data_ptr(), attr_records.data_ptr(),
                                                 ids.data_ptr(), stream)
        return out

    def finalize_range(self, lo: int, hi: int, out: dict, pathline: bool, stream=None):
        """The lines of slots [lo, hi) into ``out`` (device tensors points [m, P, 3], velocity [m, P, 3],
        temperature / salinity [m, P], m = hi - lo) in slot order -- row i is particle ids[lo + i] -- a
        bounded piece of finalize (PathlineChain's writer hook).  A set with an attribute slab also stores
        ``out["attributes"]`` [n_attr, m, P]."""
        m = hi - lo
        if m <= 0:
            return out
        if self.attr_records is not None:
            out["attributes"] = self._attr_lines(m, self.seeds.data_ptr() + 24 * lo, self.records.data_ptr() + 8 * lo,
                                                 self.attr_records.data_ptr() + 8 * lo, None, stream)
        L.check(L.load().mops_traj_finalize(m, self.K, C.c_void_p(self.seeds.data_ptr() + 24 * lo),
                                            C.c_void_p(self.records.data_ptr() + 8 * lo), self.rec_stride,
                                            1 if pathline else 0, None, C.c_void_p(out["points"].data_ptr()),
                                            C.c_void_p(out["velocity"].data_ptr()),
                                            C.c_void_p(out["temperature"].data_ptr()),
                                            C.c_void_p(out["salinity"].data_ptr()), None, _stream_handle(stream)),
                "mops_traj_finalize")
        return out

    def finalize(self, pathline: bool, stream=None, streams=None, timing=None):
        """Lines of every particle in seed order (mops_traj_finalize).  ``streams``: the
        advance_pipelined part streams -- each part's lines are assembled on its own stream right
        after its last chunk, so one part's assembly overlaps the other parts' final waves (the
        caller joins the streams afterwards); ``timing`` receives (start, end) events per launch.  A set with
        an attribute slab also returns ``attributes`` [n_attr, n, K + 1] (mops_traj_finalize_attrs; one
        stream only)."""
        torch = self.torch
        if streams and self.attr_records is not None:
            raise ValueError("finalize: part streams are not supported for a particle set with an attribute slab")
        dev = self.seeds.device
        P = self.K + 1
        pts = torch.empty((self.n, P, 3), dtype=torch.float64, device=dev)
        vel = torch.empty_like(pts)
        tmp = torch.empty((self.n, P), dtype=torch.float64, device=dev)
        sal = torch.empty_like(tmp)
        last = torch.empty((self.n, 3), dtype=torch.float64, device=dev)
        outs = (pts, vel, tmp, sal, last)
        if streams:
            pb = self.part_bounds(len(streams))
            parts = [(pb[k], pb[k + 1], streams[k]) for k in range(len(streams))]
            for t in outs:  # written on the part streams: the allocator must wait for them
                for st in streams:
                    t.record_stream(st if isinstance(st, torch.cuda.Stream) else torch.cuda.ExternalStream(int(st)))
        else:
            parts = [(0, self.n, stream)]
        lib = L.load()
        for lo, hi, st in parts:
            if hi <= lo:
                continue
            if timing is not None:
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                ts = st if isinstance(st, torch.cuda.Stream) else (
                    torch.cuda.ExternalStream(int(st)) if st else torch.cuda.default_stream(dev))
                e0.record(ts)
            # a part's slots write the lines ids[slot] of the full outputs
            rc = lib.mops_traj_finalize(hi - lo, self.K, C.c_void_p(self.seeds.data_ptr() + 24 * lo),
                                        C.c_void_p(self.records.data_ptr() + 8 * lo), self.rec_stride,
                                        1 if pathline else 0,
                                        C.c_void_p(self.ids.data_ptr() + 4 * lo), C.c_void_p(pts.data_ptr()),
                                        C.c_void_p(vel.data_ptr()), C.c_void_p(tmp.data_ptr()),
                                        C.c_void_p(sal.data_ptr()), C.c_void_p(last.data_ptr()), _stream_handle(st))
            L.check(rc, "mops_traj_finalize")
            if timing is not None:
                e1.record(ts)
                timing.append((e0, e1))
        out = dict(points=pts, velocity=vel, temperature=tmp, salinity=sal, lastPoint=last)
        if self.attr_records is not None:
            out["attributes"] = self._attr_lines(self.n, self.seeds.data_ptr(), self.records.data_ptr(),
                                                 self.attr_records.data_ptr(), self.ids.data_ptr(), stream)
        return out


LAYER_RULES = {"reference": L.MOPS_LAYER_REFERENCE, "bracket": L.MOPS_LAYER_BRACKET}


def _remap_cfg(width, height, lat_range=(0.0, 0.0), lon_range=(0.0, 0.0), depth=0.0, latitude=0.0,
               depth_range=(0.0, 0.0), layer_rule="reference", layer=0.0) -> L.RemapCfg:
    if layer_rule not in LAYER_RULES:
        raise ValueError(f"layer_rule must be one of {sorted(LAYER_RULES)}, not {layer_rule!r}")
    width, height = _image_size(width, height)
    return L.RemapCfg(width, height, float(lat_range[0]), float(lat_range[1]), float(lon_range[0]),
                      float(lon_range[1]), float(depth), float(latitude), float(depth_range[0]),
                      float(depth_range[1]), LAYER_RULES[layer_rule], float(layer))


def remap_tables(width, height, lat_range=(0.0, 0.0), lon_range=(0.0, 0.0), latitude=None):
    """The host cos / sin tables the remapping kernels form pixel positions from (mops_remap_tables; no
    device work): (row_cos, row_sin, col_cos, col_sin).  ``latitude`` None: the fixed-depth image's rows
    and columns; else the fixed-latitude image's one row and its columns."""
    cfg = _remap_cfg(width, height, lat_range, lon_range, latitude=0.0 if latitude is None else latitude)
    rows = int(height) if latitude is None else 1
    rc, rs = np.empty(rows), np.empty(rows)
    cc, cs = np.empty(int(width)), np.empty(int(width))
    L.check(L.load().mops_remap_tables(C.byref(cfg), 0 if latitude is None else 1, _ptr(rc), _ptr(rs), _ptr(cc),
                                       _ptr(cs)), "mops_remap_tables")
    return rc, rs, cc, cs


def cell_to_vertex_attr(mesh: DeviceMesh, cell_attr, signed: bool = False):
    """CalcCellCenterToVertex for one double attribute (mops_cell_to_vertex_attr): a [C*L] array (numpy or
    CUDA tensor) -> a [V, L] float64 CUDA tensor in the caller's vertex order, on torch's current stream.
    Negative results are clamped to 0, the reference's rule for temperature and salinity; ``signed`` keeps them
    (mops_cell_to_vertex_signed), for signed fields such as ``velocity_gradient``'s."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(cell_attr, torch.Tensor):
        cell_attr = torch.as_tensor(np.ascontiguousarray(cell_attr, dtype=np.float64).reshape(-1))
    src = cell_attr.to(device=dev, dtype=torch.float64).contiguous()
    if src.numel() != mesh.nCells * mesh.nVertLevels:
        raise ValueError("attribute is not [nCells * nVertLevels]")
    out = torch.empty((mesh.nVertices, mesh.nVertLevels), dtype=torch.float64, device=dev)
    name = "mops_cell_to_vertex_signed" if signed else "mops_cell_to_vertex_attr"
    L.check(getattr(L.load(), name)(mesh.handle, _tensor_ptr(src), _tensor_ptr(out), _stream_or_current(None, dev)),
            name)
    return out


EDDY_FIELDS = ("vorticity", "divergence", "strain", "okubo_weiss")


def velocity_gradient(mesh: DeviceMesh, field: DeviceField, which=EDDY_FIELDS, vertex: bool = False, stream=None):
    """Relative vorticity, horizontal divergence, strain rate and the Okubo-Weiss parameter of every cell and
    level (mops_velocity_gradient; the operator is stated in include/mops_traj.h): a dict of float64 CUDA
    tensors [nCells, nVertLevels] for the names in ``which``.  ``vertex``: [nVertices, nVertLevels] instead,
    through the signed cell-to-vertex interpolation (``cell_to_vertex_attr(signed=True)``), ready to pass as
    ``vertex_attrs`` / ``attrs=`` to the remapping, section and pathline entries.  A cell the operator refuses
    (fewer than three vertices, zero area) is NaN at every level.  ValueError for an unknown or missing name."""
    import torch
    if isinstance(which, str):
        which = (which,)
    names = tuple(which)
    bad = [w for w in names if w not in EDDY_FIELDS]
    if bad or not names:
        raise ValueError(f"which: expected names out of {EDDY_FIELDS}, not {tuple(which)!r}")
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _stream_or_current(stream, dev)
    out = {w: torch.empty((mesh.nCells, mesh.nVertLevels), dtype=torch.float64, device=dev) for w in names}
    ptr = [_tensor_ptr(out.get(w)) for w in EDDY_FIELDS]
    L.check(L.load().mops_velocity_gradient(mesh.handle, field.handle, *ptr, h), "mops_velocity_gradient")
    if vertex:
        lib = L.load()
        for w in names:
            vt = torch.empty((mesh.nVertices, mesh.nVertLevels), dtype=torch.float64, device=dev)
            L.check(lib.mops_cell_to_vertex_signed(mesh.handle, _tensor_ptr(out[w]), _tensor_ptr(vt), h),
                    "mops_cell_to_vertex_signed")
            _release_on(out[w], stream)  # the cell array
            out[w] = vt
    return out


def _census_args(mesh: DeviceMesh, layer, min_cells=1, threshold=None):
    """The checks eddy_classify, eddy_table and eddy_census share; returns (layer, min_cells) as ints."""
    import math
    layer, min_cells = int(layer), int(min_cells)
    if not 0 <= layer < mesh.nVertLevels:
        raise ValueError(f"layer {layer} outside the {mesh.nVertLevels} levels")
    if min_cells < 1:
        raise ValueError(f"min_cells {min_cells} < 1")
    if threshold is not None and not math.isfinite(float(threshold)):
        raise ValueError(f"threshold {threshold!r} is not finite")
    return layer, min_cells


def _cell_tensor(mesh: DeviceMesh, t, name: str, dtype, per_level: bool = False):
    import torch
    n = mesh.nCells * (mesh.nVertLevels if per_level else 1)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == n):
        shape = "[nCells, nVertLevels]" if per_level else "[nCells]"
        raise ValueError(f"{name}: expected a contiguous {dtype} CUDA tensor {shape}")
    return C.c_void_p(t.data_ptr())


def cell_area(mesh: DeviceMesh, stream=None):
    """The planar area of every cell in its centre's east / north frame (mops_cell_area: half the magnitude of
    the velocity-gradient operator's ``A2``): a float64 CUDA tensor [nCells], NaN where that operator refuses
    the cell."""
    import torch
    out = torch.empty((mesh.nCells,), dtype=torch.float64, device="cuda")
    L.check(L.load().mops_cell_area(mesh.handle, _tensor_ptr(out), _stream_or_current(stream)), "mops_cell_area")
    return out


def level_mean(field, weight, stream=None):
    """The weighted mean of a cell field per level (mops_level_mean; the order of its sum is stated in
    include/mops_traj.h): ``field`` a float64 CUDA tensor [C, L], ``weight`` a float64 CUDA tensor [C].  A term
    counts where the field value and the weight are finite and the weight is positive, so a caller confines the
    mean to a window or basin by zeroing weights.  Returns ``(mean [L], wsum [L])`` as float64 CUDA tensors; the
    mean of a level without a counting cell is NaN and its ``wsum`` 0.  Mesh-free: any [C, L].  The library call
    runs on ``stream`` (default torch's current one) and synchronises it (the group partials are a temporary
    allocation of the call)."""
    import torch
    for t, name, nd in ((field, "field", 2), (weight, "weight", 1)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                and t.dim() == nd):
            raise ValueError(f"level_mean: {name} must be a contiguous float64 CUDA tensor "
                             f"{'[C, L]' if nd == 2 else '[C]'}")
    C_, L_ = int(field.shape[0]), int(field.shape[1])
    if C_ < 1 or L_ < 1 or int(weight.shape[0]) != C_ or weight.device != field.device:
        raise ValueError("level_mean: field [C, L] and weight [C] with C, L >= 1 on one device")
    with torch.cuda.device(field.device):
        mean = torch.empty((L_,), dtype=torch.float64, device=field.device)
        wsum = torch.empty((L_,), dtype=torch.float64, device=field.device)
        L.check(L.load().mops_level_mean(C_, L_, _tensor_ptr(field), _tensor_ptr(weight), _tensor_ptr(mean),
                                         _tensor_ptr(wsum), _stream_or_current(stream, field.device)),
                "mops_level_mean")
    return mean, wsum


def vorticity_deviation(mesh: DeviceMesh, field: DeviceField, weight=None, vertex: bool = True, stream=None):
    """``(deviation, mean)``: the relative vorticity of ``velocity_gradient`` minus its weighted horizontal mean
    per level (``level_mean``), the integrand of the Lagrangian-averaged vorticity deviation; ``mean`` is the
    float64 CUDA tensor [nVertLevels] that was subtracted.  ``weight`` [nCells]: None = ``cell_area(mesh)``; a
    caller confines the mean to a window or basin by zeroing weights.  ``vertex`` (the default): the deviation as
    [nVertices, nVertLevels] through ``cell_to_vertex_attr(signed=True)``'s interpolation, ready for the
    samplers; else [nCells, nVertLevels].  All of it runs on ``stream`` (default torch's current one); the
    subtraction is one IEEE operation per element, a torch broadcast under that stream."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    h = _current_or(stream, dev)
    vort = velocity_gradient(mesh, field, "vorticity", stream=h)["vorticity"]
    own_weight = weight is None
    if own_weight:
        weight = cell_area(mesh, stream=h)
    elif not (isinstance(weight, torch.Tensor) and weight.is_cuda and weight.dtype == torch.float64
              and weight.is_contiguous() and weight.numel() == mesh.nCells):
        raise ValueError("vorticity_deviation: weight must be a contiguous float64 CUDA tensor [nCells]")
    mean, _ = level_mean(vort, weight.reshape(-1), stream=h)
    dev_c = torch.empty_like(vort)
    with _on_stream(h):
        torch.sub(vort, mean[None, :], out=dev_c)
    _release_on(vort, stream)
    if own_weight:
        _release_on(weight, stream)
    if not vertex:
        return dev_c, mean
    vt = torch.empty((mesh.nVertices, mesh.nVertLevels), dtype=torch.float64, device=dev)
    L.check(L.load().mops_cell_to_vertex_signed(mesh.handle, _tensor_ptr(dev_c), _tensor_ptr(vt), _stream_handle(h)),
            "mops_cell_to_vertex_signed")
    _release_on(dev_c, stream)
    return vt, mean


def eddy_classify(mesh: DeviceMesh, okubo_weiss, vorticity, layer: int, threshold: float, stream=None):
    """+1 / -1 / 0 per cell at ``layer`` (mops_eddy_classify): Okubo-Weiss below ``threshold`` and vorticity
    positive / negative / anything else (NaN is class 0).  The arrays are ``velocity_gradient``'s
    [nCells, nVertLevels] tensors; returns an int32 CUDA tensor [nCells]."""
    import torch
    layer, _ = _census_args(mesh, layer, threshold=threshold)
    ow = _cell_tensor(mesh, okubo_weiss, "okubo_weiss", torch.float64, per_level=True)
    vo = _cell_tensor(mesh, vorticity, "vorticity", torch.float64, per_level=True)
    out = torch.empty((mesh.nCells,), dtype=torch.int32, device="cuda")
    L.check(L.load().mops_eddy_classify(mesh.handle, ow, vo, layer, float(threshold), _tensor_ptr(out),
                                        _stream_or_current(stream)), "mops_eddy_classify")
    return out


def label_components(mesh: DeviceMesh, classes, return_rounds: bool = False, stream=None):
    """Connected components of an int32 CUDA class array [nCells] over the cellsOnCell graph
    (mops_label_components): cells are joined across an edge when their classes are equal and not 0.  Returns an
    int32 CUDA tensor [nCells]: the smallest cell index of the cell's component, -1 for class 0.  The call
    synchronises the stream (the host decides convergence between rounds); ``return_rounds``: also the rounds
    used."""
    import torch
    cls = _cell_tensor(mesh, classes, "classes", torch.int32)
    out = torch.empty((mesh.nCells,), dtype=torch.int32, device="cuda")
    rounds = C.c_int32(0)
    L.check(L.load().mops_label_components(mesh.handle, cls, _tensor_ptr(out), C.byref(rounds),
                                           _stream_or_current(stream)), "mops_label_components")
    return (out, int(rounds.value)) if return_rounds else out


EDDY_COLUMNS = ("root", "n_cells", "polarity", "core_cell", "area", "circulation", "ow_min", "centre")


def eddy_table(mesh: DeviceMesh, labels, classes, area, vorticity, okubo_weiss, layer: int, min_cells: int = 1,
               stream=None):
    """Membership and the census table (mops_eddy_count, mops_eddy_table) from ``label_components``'s labels:
    components of fewer than ``min_cells`` cells are dropped, the rest numbered in ascending order of their root
    cell.  Returns (eddy_of_cell: int32 CUDA tensor [nCells], the eddy index or -1; table: a dict of numpy
    arrays [E] -- ``EDDY_COLUMNS``, ``centre`` being [E, 3]).  Every sum runs over an eddy's cells in ascending
    cell index.  Both entries synchronise the stream."""
    import torch
    layer, min_cells = _census_args(mesh, layer, min_cells)
    lab = _cell_tensor(mesh, labels, "labels", torch.int32)
    cls = _cell_tensor(mesh, classes, "classes", torch.int32)
    ar = _cell_tensor(mesh, area, "area", torch.float64)
    vo = _cell_tensor(mesh, vorticity, "vorticity", torch.float64, per_level=True)
    ow = _cell_tensor(mesh, okubo_weiss, "okubo_weiss", torch.float64, per_level=True)
    h = _stream_or_current(stream)
    lib = L.load()
    eoc = torch.empty((mesh.nCells,), dtype=torch.int32, device="cuda")
    n = C.c_int64(0)
    L.check(lib.mops_eddy_count(mesh.handle, lab, min_cells, _tensor_ptr(eoc), C.byref(n), h), "mops_eddy_count")
    E = int(n.value)
    t = {k: np.empty((E,), dtype=np.int32) for k in EDDY_COLUMNS[:4]}
    t.update({k: np.empty((E,), dtype=np.float64) for k in EDDY_COLUMNS[4:7]})
    t["centre"] = np.empty((E, 3), dtype=np.float64)
    L.check(lib.mops_eddy_table(mesh.handle, _tensor_ptr(eoc), E, cls, ar, vo, ow, layer,
                                *[_ptr(t[k]) for k in EDDY_COLUMNS], h), "mops_eddy_table")
    return eoc, t


def eddy_lat_lon_radius(centre, area):
    """(lat, lon) in degrees of the unit vectors ``centre`` [E, 3] and the radius of the circle of ``area``,
    with numpy on the host: lat = degrees(arcsin(z)), lon = degrees(arctan2(y, x)), radius = sqrt(area / pi)."""
    centre = np.asarray(centre, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        lat = np.degrees(np.arcsin(centre[:, 2]))
        lon = np.degrees(np.arctan2(centre[:, 1], centre[:, 0]))
        radius = np.sqrt(np.asarray(area, dtype=np.float64) / np.pi)
    return lat, lon, radius


class EddyCensus:
    """The result of ``eddy_census``: ``threshold`` (the Okubo-Weiss threshold used), ``labels`` (int32 CUDA
    tensor [nCells]: the eddy index of every cell or -1), ``table`` (numpy columns ``EDDY_COLUMNS`` plus ``lat``,
    ``lon`` in degrees and ``radius``, one row per eddy), ``classes`` and ``components`` (the int32 CUDA class and
    component-root arrays behind them), ``rounds`` (labelling rounds used) and ``n_eddies``."""

    def __init__(self, mesh, field, layer, threshold, classes, components, rounds, labels, table):
        self.mesh, self.field, self.layer = mesh, field, layer
        self.threshold, self.classes, self.components, self.rounds = threshold, classes, components, rounds
        self.labels, self.table = labels, table
        self.n_eddies = len(table["root"])

    def cells(self, e: int):
        """The member cells of eddy ``e`` in ascending order: an int64 CUDA tensor."""
        import torch
        e = int(e)
        if not 0 <= e < self.n_eddies:
            raise ValueError(f"eddy {e} outside the {self.n_eddies} eddies")
        return torch.nonzero(self.labels == e).reshape(-1)

    def image(self, width: int, height: int, lat_range, lon_range, return_cells: bool = False, stream=None):
        """The label image on a window: a float64 CUDA tensor [height, width, 4] = {eddy index, polarity, 0, 1}
        from the cell map of ``remap_fixed_layer`` at the census layer.  Channels 0 and 1 are NaN where the
        fixed-layer image is NaN or the pixel's cell is in no eddy, so it overlays every other image of the
        window.  ``return_cells``: also the int32 cell map and the fixed-layer image."""
        import torch
        layer_image, cells = remap_fixed_layer(self.mesh, self.field, width, height, lat_range, lon_range,
                                               float(self.layer), return_cells=True, stream=stream)
        with _on_stream(stream):
            inside = (cells >= 0) & (cells < self.mesh.nCells) & ~torch.isnan(layer_image[..., 0])
            c = torch.where(inside, cells, torch.zeros_like(cells)).long()
            e = self.labels[c]
            ok = inside & (e >= 0)
            nan = torch.full_like(layer_image[..., 0], float("nan"))
            out = torch.empty_like(layer_image)
            out[..., 0] = torch.where(ok, e.double(), nan)
            out[..., 1] = torch.where(ok, self.classes[c].double(), nan)
            out[..., 2] = 0.0
            out[..., 3] = 1.0
        return (out, cells, layer_image) if return_cells else out


def eddy_census(mesh: DeviceMesh, field: DeviceField, layer: int = 0, k_sigma: float = 0.2, threshold=None,
                min_cells: int = 4, gradient=None):
    """The eddies of one layer as objects: the cells whose Okubo-Weiss parameter lies below ``threshold``, split
    by the sign of their vorticity, grouped into connected components of the mesh (mops_eddy_classify,
    mops_label_components), and one table row per component of at least ``min_cells`` cells (mops_eddy_table).

    ``threshold``: as given, else ``-k_sigma * sigma`` with sigma the population standard deviation of the
    layer's finite Okubo-Weiss values (torch, FP64); the value used is ``.threshold``.  ``gradient``: a dict
    with ``velocity_gradient``'s "vorticity" and "okubo_weiss" tensors to reuse instead of computing them.
    ValueError before any launch for a layer outside the levels, ``min_cells < 1``, a non-finite threshold or a
    ``gradient`` of the wrong shape.  Returns an ``EddyCensus``; on torch's current stream, which it
    synchronises."""
    import math
    import torch
    layer, min_cells = _census_args(mesh, layer, min_cells, threshold)
    if threshold is None and not math.isfinite(float(k_sigma)):
        raise ValueError(f"k_sigma {k_sigma!r} is not finite")
    if gradient is not None:
        try:
            vort, ow = gradient["vorticity"], gradient["okubo_weiss"]
        except (KeyError, TypeError):
            raise ValueError("gradient: expected a dict with 'vorticity' and 'okubo_weiss'") from None
        for name, t in (("vorticity", vort), ("okubo_weiss", ow)):
            _cell_tensor(mesh, t, f"gradient[{name!r}]", torch.float64, per_level=True)
            if tuple(t.shape) != (mesh.nCells, mesh.nVertLevels):
                raise ValueError(f"gradient[{name!r}]: expected shape [nCells, nVertLevels], not {tuple(t.shape)}")
    else:
        g = velocity_gradient(mesh, field, which=("vorticity", "okubo_weiss"))
        vort, ow = g["vorticity"], g["okubo_weiss"]
    if threshold is None:
        col = ow[:, layer]
        fin = col[torch.isfinite(col)]
        sigma = float(torch.std(fin, unbiased=False)) if fin.numel() else float("nan")
        threshold = -float(k_sigma) * sigma
        if not math.isfinite(threshold):
            raise ValueError("no finite Okubo-Weiss value in the layer: no threshold")
    threshold = float(threshold)
    classes = eddy_classify(mesh, ow, vort, layer, threshold)
    components, rounds = label_components(mesh, classes, return_rounds=True)
    labels, table = eddy_table(mesh, components, classes, cell_area(mesh), vort, ow, layer, min_cells)
    table["lat"], table["lon"], table["radius"] = eddy_lat_lon_radius(table["centre"], table["area"])
    return EddyCensus(mesh, field, layer, threshold, classes, components, rounds, labels, table)


def _vertex_attr_ptr(mesh: DeviceMesh, t, name: str):
    if not (t.is_cuda and t.dtype.is_floating_point and t.element_size() == 8 and t.is_contiguous()
            and t.numel() == mesh.nVertices * mesh.nVertLevels):
        raise ValueError(f"{name}: expected a contiguous float64 CUDA tensor [nVertices, nVertLevels]")
    return C.c_void_p(t.data_ptr())


def remap_fixed_depth(mesh: DeviceMesh, field: DeviceField, width: int, height: int, lat_range, lon_range,
                      depth: float, n_attr: int = 0, vertex_attrs=(), layer_rule: str = "reference",
                      return_cells: bool = False, stage_ms: list | None = None, stream=None):
    """MOPSApp::runRemapping (mops_remap_fixed_depth): the fixed-depth images as one float64 CUDA tensor
    [n_images, height, width, 4], n_images = 1 + ceil(n_attr / 3) (1 without attributes).

    ``n_attr``: the solution's double-attribute count; with two or more, ``vertex_attrs`` holds the vertex
    arrays (``cell_to_vertex_attr``) of the first two in name order.  ``layer_rule``: "reference" (every wet
    pixel is layer 0, quirk Q13) or "bracket".  ``return_cells``: also the int32 [height, width] cell map.
    ``stage_ms``: a list that receives the positions / locate / evaluation times (HIP events, ms)."""
    import torch
    cfg = _remap_cfg(width, height, lat_range, lon_range, depth=depth, layer_rule=layer_rule)
    n_attr = int(n_attr)
    if n_attr < 0 or (n_attr > 1 and len(vertex_attrs) < 2):
        raise ValueError("n_attr > 1 needs the first two attributes' vertex arrays")
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    a = [_vertex_attr_ptr(mesh, vertex_attrs[k], f"vertex_attrs[{k}]") if n_attr > 1 else None for k in range(2)]
    images = torch.empty((int(lib.mops_remap_num_images(n_attr)), cfg.height, cfg.width, 4), dtype=torch.float64,
                         device=dev)
    cells = torch.empty((cfg.height, cfg.width), dtype=torch.int32, device=dev) if return_cells else None
    ms = (C.c_float * 3)() if stage_ms is not None else None
    L.check(lib.mops_remap_fixed_depth(mesh.handle, field.handle, C.byref(cfg), n_attr, a[0], a[1],
                                       _tensor_ptr(images), _tensor_ptr(cells), ms, _stream_or_current(stream, dev)),
            "mops_remap_fixed_depth")
    if stage_ms is not None:
        stage_ms[:] = [float(x) for x in ms]
    return (images, cells) if return_cells else images


def remap_fixed_latitude(mesh: DeviceMesh, field: DeviceField, width: int, height: int, lon_range,
                         latitude: float, depth_range, return_cells: bool = False, stream=None):
    """MOPSApp::runReGrid (mops_remap_fixed_latitude): one float64 CUDA tensor [height, width, 4]; rows are
    depths from depth_range[0] to depth_range[1] (the grid's refBottomDepth front / back), columns
    longitudes at ``latitude``.  ``return_cells``: also the int32 [width] cell of each column."""
    import torch
    cfg = _remap_cfg(width, height, lon_range=lon_range, latitude=latitude, depth_range=depth_range)
    dev = torch.device("cuda", torch.cuda.current_device())
    image = torch.empty((cfg.height, cfg.width, 4), dtype=torch.float64, device=dev)
    cells = torch.empty((cfg.width,), dtype=torch.int32, device=dev) if return_cells else None
    L.check(L.load().mops_remap_fixed_latitude(mesh.handle, field.handle, C.byref(cfg), _tensor_ptr(image),
                                               _tensor_ptr(cells), _stream_or_current(stream, dev)),
            "mops_remap_fixed_latitude")
    return (image, cells) if return_cells else image


def remap_fixed_layer(mesh: DeviceMesh, field: DeviceField, width: int, height: int, lat_range, lon_range,
                      layer: float, return_cells: bool = False, stream=None):
    """Kernel::VisualizeFixedLayer (mops_remap_fixed_layer): one float64 CUDA tensor [height, width, 4] =
    {zonal, meridional, 0, 1} at layer ClampLayer(int(layer), nVertLevels) -- ``layer`` is the settings'
    double FixedLayer, truncated toward zero and clamped into the levels; NaN outside the mesh.
    ``return_cells``: also the int32 [height, width] cell map."""
    import torch
    cfg = _remap_cfg(width, height, lat_range, lon_range, layer=layer)
    dev = torch.device("cuda", torch.cuda.current_device())
    image = torch.empty((cfg.height, cfg.width, 4), dtype=torch.float64, device=dev)
    cells = torch.empty((cfg.height, cfg.width), dtype=torch.int32, device=dev) if return_cells else None
    L.check(L.load().mops_remap_fixed_layer(mesh.handle, field.handle, C.byref(cfg), _tensor_ptr(image),
                                            _tensor_ptr(cells), _stream_or_current(stream, dev)),
            "mops_remap_fixed_layer")
    return (image, cells) if return_cells else image


def _waypoints(path) -> np.ndarray:
    try:
        way = np.ascontiguousarray([(float(lat), float(lon)) for lat, lon in path], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("path: expected a sequence of (lat, lon) waypoints in degrees") from None
    return way.reshape(-1, 2)


def section_points(path, width: int):
    """The columns of a section along great-circle legs through the (lat, lon) waypoints of ``path``
    (mops_section_points; host only): (points [width, 3] on the remapping's sphere, unit normals [width, 3] to
    the left of the direction of travel, distance [width] in metres from the first waypoint), numpy float64.
    ValueError where the entry refuses: fewer than two waypoints or columns, a non-finite waypoint, |lat| > 90,
    a leg of zero length or between antipodal waypoints."""
    way = _waypoints(path)
    width = int(width)
    if not -2**31 <= width < 2**31:
        raise ValueError(f"invalid column count {width}")
    n = max(width, 0)
    pts, nrm, dist = np.empty((n, 3)), np.empty((n, 3)), np.empty(n)
    st = L.load().mops_section_points(len(way), _ptr(way), width, _ptr(pts), _ptr(nrm), _ptr(dist))
    if st == L.MOPS_ERR_INVALID:
        raise ValueError(L.load().mops_last_error().decode(errors="replace"))
    L.check(st, "mops_section_points")
    return pts, nrm, dist


def section_transport(image, distance, depth_range):
    """Volume transport through a section (mops_section_transport; host only): ``image`` is image 0 of
    ``remap_section`` ([height, width, 4], a tensor or an array), ``distance`` its columns' [width] metres,
    ``depth_range`` its rows' (first, last) depth.  Returns (Sverdrups, valid area in m^2): the across channel
    times ds * dz over the non-NaN pixels, one fixed-order FP64 sum (include/mops_traj.h)."""
    if hasattr(image, "detach"):
        image = image.detach().cpu().numpy()
    img = np.ascontiguousarray(image, dtype=np.float64)
    dist = np.ascontiguousarray(distance, dtype=np.float64).reshape(-1)
    if img.ndim != 3 or img.shape[2] != 4 or img.shape[1] != dist.size:
        raise ValueError("section_transport: expected an image [height, width, 4] and distance [width]")
    sv, area = C.c_double(), C.c_double()
    st = L.load().mops_section_transport(img.shape[1], img.shape[0], _ptr(img), _ptr(dist), float(depth_range[0]),
                                         float(depth_range[1]), C.byref(sv), C.byref(area))
    if st == L.MOPS_ERR_INVALID:
        raise ValueError(L.load().mops_last_error().decode(errors="replace"))
    L.check(st, "mops_section_transport")
    return sv.value, area.value


def remap_section(mesh: DeviceMesh, field: DeviceField, path, width: int, height: int, depth_range=None,
                  vertex_attrs=(), return_cells: bool = False, columns=None, stream=None):
    """A vertical section (mops_remap_section): depth by distance along great-circle legs through the
    (lat, lon) waypoints of ``path``.  Returns (images, distance): a float64 CUDA tensor [1 + (1 if
    vertex_attrs else 0), height, width, 4] and the columns' distance [width] in metres (numpy).

    Image 0 is {zonal, meridional, across, 1}: the fixed-latitude curtain's pixel at each column's position and
    row's depth, and the velocity across the section, positive to the left of the direction of travel.  Image 1
    (with one or two ``vertex_attrs``, vertex arrays from ``cell_to_vertex_attr``) is {attr0, attr1 or 0, 0, 1},
    blended in depth as the velocity is.  Failed pixels are NaN.  ``depth_range`` None: the mesh's
    (refBottomDepth[0], refBottomDepth[-1]) (a ``DeviceMesh.from_mesh`` of a mesh that has them).
    ``return_cells``: also the int32 [width] cell of each column, as a third value.  ``columns`` = (points
    [width, 3], normals [width, 3] or None) replaces ``path`` (then None) by explicit column positions; the
    distance returned is None, and without normals the across channel is 0."""
    import torch
    width, height = _image_size(width, height)
    if columns is None:
        pts, nrm, dist = section_points(path, width)
    else:
        if path is not None:
            raise ValueError("remap_section: give either path or columns")
        pts = np.ascontiguousarray(columns[0], dtype=np.float64)
        nrm = None if columns[1] is None else np.ascontiguousarray(columns[1], dtype=np.float64)
        dist = None
        if pts.shape != (width, 3) or (nrm is not None and nrm.shape != (width, 3)):
            raise ValueError("remap_section: columns must be [width, 3] arrays")
    if depth_range is None:
        ref = getattr(mesh, "refBottomDepth", None)
        if ref is None or len(ref) == 0:
            raise ValueError("remap_section: depth_range is needed for a mesh without refBottomDepth")
        depth_range = (float(ref[0]), float(ref[-1]))
    d0, d1 = float(depth_range[0]), float(depth_range[1])
    if not (np.isfinite(d0) and np.isfinite(d1)):
        raise ValueError("remap_section: non-finite depth range")
    n_attr = len(vertex_attrs)
    if n_attr > 2:
        raise ValueError("remap_section: at most two vertex attributes")
    a = [_vertex_attr_ptr(mesh, vertex_attrs[k], f"vertex_attrs[{k}]") if k < n_attr else None for k in range(2)]
    dev = torch.device("cuda", torch.cuda.current_device())
    images = torch.empty((2 if n_attr else 1, height, width, 4), dtype=torch.float64, device=dev)
    cells = torch.empty((width,), dtype=torch.int32, device=dev) if return_cells else None
    L.check(L.load().mops_remap_section(mesh.handle, field.handle, width, height, d0, d1, _ptr(pts), _ptr(nrm), n_attr,
                                        a[0], a[1], _tensor_ptr(images[0]), _tensor_ptr(images[1] if n_attr else None),
                                        _tensor_ptr(cells), _stream_or_current(stream, dev)), "mops_remap_section")
    return (images, dist, cells) if return_cells else (images, dist)


def colormap_rgba(image_cuda, channels=(0, 1, 2), return_minmax: bool = False, stream=None):
    """MOPS::SaveToPNG's colouring on the device (mops_colormap_rgba8): a float64 CUDA image [H, W, 4] -> a
    uint8 CUDA tensor [len(channels), H, W, 4] (RGBA, Viridis; NaN pixels {0, 0, 0, 0}), one plane per entry of
    ``channels`` (each 0..3, strictly ascending).  ``return_minmax``: also a float32 numpy array
    [len(channels), 2], every selected channel's {min, max} as the map used them."""
    import torch
    t = image_cuda
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 3
            and t.shape[2] == 4 and t.is_contiguous() and t.numel() > 0):
        raise ValueError("colormap_rgba: expected a contiguous float64 CUDA tensor [H, W, 4]")
    channels = [int(c) for c in channels]
    if not channels or any(c < 0 or c > 3 for c in channels) or any(b <= a for a, b in zip(channels, channels[1:])):
        raise ValueError("colormap_rgba: channels must be strictly ascending values in 0..3")
    mask = sum(1 << c for c in channels)
    hgt, wid = int(t.shape[0]), int(t.shape[1])
    out = torch.empty((len(channels), hgt, wid, 4), dtype=torch.uint8, device=t.device)
    mm = np.empty((4, 2), dtype=np.float32) if return_minmax else None
    with torch.cuda.device(t.device):
        L.check(L.load().mops_colormap_rgba8(_tensor_ptr(t), wid, hgt, mask, _tensor_ptr(out), _ptr(mm),
                                             _stream_or_current(stream, t.device)), "mops_colormap_rgba8")
    return (out, mm[channels]) if return_minmax else out


DENSITY_KINDS = {None: L.MOPS_DENSITY_COUNT, "speed": L.MOPS_DENSITY_SPEED}


class DensityMap:
    """A particle density map (mops_density_accumulate, include/mops_traj.h): how many trajectory samples fell
    into each lat / lon pixel of a ``width`` x ``height`` window, and the fixed-point sum of a value over them.

    ``value``: None (count only), "speed" (the record's |velocity|) or an attribute name (the matching row of
    a ParticleSet's attribute slab; ``names`` of the sampled attributes are given to ``accumulate``).
    ``accum`` is the raw int64 CUDA tensor [height, width, 2] = {count, qsum}: integer sums, so the same bytes
    for every particle order and launch split.  ``image()`` turns it into an [height, width, 4] float64 image
    {count, mean, sum, 1} for ``colormap_rgba`` and the PNG / VTI writers."""

    def __init__(self, width: int, height: int, lat_range, lon_range, value: str | None = None, device=None):
        import torch
        if value is not None and not isinstance(value, str):
            raise ValueError("DensityMap: value must be None, 'speed' or an attribute name")
        lat, lon = (float(lat_range[0]), float(lat_range[1])), (float(lon_range[0]), float(lon_range[1]))
        width, height = _image_size(width, height)
        if not (np.isfinite(lat).all() and np.isfinite(lon).all() and lat[1] > lat[0] and lon[1] > lon[0]
                and lon[1] - lon[0] <= 360.0):
            raise ValueError(f"invalid latitude / longitude range {lat} / {lon}")
        self.torch = torch
        self.width, self.height, self.lat_range, self.lon_range, self.value = width, height, lat, lon, value
        self.kind = DENSITY_KINDS.get(value, L.MOPS_DENSITY_VALUES)
        self.cfg = _remap_cfg(width, height, lat, lon)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.accum = torch.zeros((height, width, 2), dtype=torch.int64, device=self.device)

    @property
    def attribute(self):
        """The attribute name this map averages, or None for a count or speed map."""
        return self.value if self.kind == L.MOPS_DENSITY_VALUES else None

    def reset(self):
        """Zero the accumulator: a torch fill on torch's *current* stream (there is no ``stream=``), without a
        host synchronisation.  A caller that accumulates on another stream orders the two itself."""
        self.accum.zero_()

    def _call(self, n, k0, k1, points_ptr, sk, si, sc, seeds_ptr, values_ptr, vk, vi, stream):
        with self.torch.cuda.device(self.device):
            L.check(L.load().mops_density_accumulate(
                C.byref(self.cfg), int(n), int(k0), int(k1), C.c_void_p(points_ptr), int(sk), int(si), int(sc),
                None if seeds_ptr is None else C.c_void_p(seeds_ptr), self.kind,
                None if values_ptr is None else C.c_void_p(values_ptr), int(vk), int(vi),
                _tensor_ptr(self.accum), _stream_or_current(stream, self.device)), "mops_density_accumulate")

    def accumulate(self, ps: "ParticleSet", n_records: int | None = None, seeds: bool = False, names=None,
                   record_range=None, stream=None):
        """Bin record slots [0, n_records) (default ``ps.K``; or ``record_range`` = (k_begin, k_end)) of every
        particle of ``ps`` from its record slab, on ``stream`` (default torch's current one), without a host
        synchronisation.  ``seeds``: also the particles' seeds (count maps only: a seed carries no value).
        A map of an attribute reads that attribute's row of ``ps.attr_records``: ``names`` lists the sampled
        attributes in slab order (PathlineChain passes its own; default salinity, temperature -- std::map
        order -- cut to ``ps.n_attr``)."""
        k0, k1 = (0, ps.K if n_records is None else int(n_records)) if record_range is None else map(int, record_range)
        if k0 < 0 or k1 > ps.records.shape[0]:
            raise ValueError(f"record range [{k0}, {k1}) outside the slab's {ps.records.shape[0]} slots")
        vptr, vk = None, 0
        if self.kind == L.MOPS_DENSITY_VALUES:
            names = list(names) if names is not None else ["salinity", "temperature"][:ps.n_attr]
            if ps.attr_records is None or self.value not in names or names.index(self.value) >= ps.n_attr:
                raise ValueError(f"DensityMap: the particle set samples no attribute {self.value!r}")
            vptr = ps.attr_records.data_ptr() + 8 * names.index(self.value) * ps.rec_stride
            vk = ps.n_attr * ps.rec_stride
        self._call(ps.n, k0, k1, ps.records.data_ptr(), 6 * ps.rec_stride, 1, ps.rec_stride,
                   ps.seeds.data_ptr() if seeds else None, vptr, vk, 1, stream)

    def accumulate_lines(self, points, values=None):
        """Bin every point of [n, P, 3] lines (CUDA tensor or host array) on torch's current stream; ``values``
        [n, P] for a map of an attribute, velocities [n, P, 3] for a speed map."""
        torch = self.torch
        pts = torch.as_tensor(points, dtype=torch.float64).to(self.device).contiguous()
        if pts.dim() != 3 or pts.shape[2] != 3:
            raise ValueError("accumulate_lines: points must be [n, P, 3]")
        n, P = int(pts.shape[0]), int(pts.shape[1])
        if self.kind == L.MOPS_DENSITY_COUNT:
            self._call(n, 0, P, pts.data_ptr(), 3, 3 * P, 1, None, None, 0, 0, None)
            return
        if values is None:
            raise ValueError("accumulate_lines: this map needs values")
        val = torch.as_tensor(values, dtype=torch.float64).to(self.device).contiguous()
        if self.kind == L.MOPS_DENSITY_SPEED:
            if tuple(val.shape) != (n, P, 3):
                raise ValueError("accumulate_lines: a speed map needs velocities [n, P, 3]")
            both = torch.cat([pts, val], dim=2).contiguous()  # [n][P][6]: the velocity at components 3..5
            self._call(n, 0, P, both.data_ptr(), 6, 6 * P, 1, None, None, 0, 0, None)
            return
        if tuple(val.shape) != (n, P):
            raise ValueError("accumulate_lines: values must be [n, P]")
        self._call(n, 0, P, pts.data_ptr(), 3, 3 * P, 1, None, val.data_ptr(), 1, P, None)

    def image(self, nan_empty: bool = True, stream=None):
        """The accumulator as a float64 CUDA image [height, width, 4] = {count, mean, sum, 1}
        (mops_density_image); ``nan_empty``: pixels without samples are NaN in channels 0-2 (transparent in
        ``colormap_rgba``), else count and sum are 0 there and only the mean is NaN."""
        torch = self.torch
        with torch.cuda.device(self.device):
            img = torch.empty((self.height, self.width, 4), dtype=torch.float64, device=self.device)
            L.check(L.load().mops_density_image(C.byref(self.cfg), _tensor_ptr(self.accum), 1 if nan_empty else 0,
                                                _tensor_ptr(img), _stream_or_current(stream, self.device)),
                    "mops_density_image")
        return img


class PathIntegral:
    """The integral of |a sampled attribute| along each particle's path (mops_path_integral_abs,
    include/mops_traj.h "path integrals and LAVD"): ``accum`` is a float64 CUDA tensor [n] indexed by particle
    id (seed order), whatever order the particle set keeps its slots in.

    The rule is a rectangle rule: slot j of a pair's attribute slab is sampled at the start of step
    (j+1)*ri - 1 (ri = recordT / deltaT steps) and stands for one record interval, so a pair adds
    sum_j |sample_j| * |recordT| seconds, in ascending j, onto what the accumulator holds: a chain that
    accumulates pair by pair equals one long ascending sum.  A particle's slots after its death hold the
    reference's zeros and add nothing; a consumer masks such a particle (``FlowMapLattice.lavd(death=)``).  A
    non-finite sample makes the sum non-finite."""

    def __init__(self, n: int, device=None):
        import torch
        n = int(n)
        if n < 1:
            raise ValueError(f"PathIntegral: n {n} < 1")
        self.torch = torch
        self.n = n
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.accum = torch.zeros((n,), dtype=torch.float64, device=self.device)

    def reset(self):
        """Zero the accumulator: a torch fill on torch's *current* stream (there is no ``stream=``), as
        ``DensityMap.reset``."""
        self.accum.zero_()

    @staticmethod
    def _weight(weight):
        weight = float(weight)
        if not (np.isfinite(weight) and weight >= 0.0):
            raise ValueError(f"PathIntegral: the weight must be finite and >= 0, not {weight!r}")
        return weight

    def _call(self, n, k0, k1, values_ptr, vk, vi, ids_ptr, weight, stream):
        with self.torch.cuda.device(self.device):
            L.check(L.load().mops_path_integral_abs(
                int(n), int(k0), int(k1), C.c_void_p(values_ptr), int(vk), int(vi),
                None if ids_ptr is None else C.c_void_p(ids_ptr), weight, _tensor_ptr(self.accum),
                _stream_or_current(stream, self.device)), "mops_path_integral_abs")

    def accumulate(self, ps: "ParticleSet", name: str, names=None, n_records: int | None = None, weight=None,
                   stream=None):
        """Add slots [0, n_records) (default ``ps.K``) of the attribute ``name`` from ``ps.attr_records``, each
        times ``weight`` (default |recordT| seconds of ``ps.cfg``: the rectangle rule above), onto ``accum`` at
        ``ps.ids``, on ``stream`` (default torch's current one), without a host synchronisation.  ``names`` lists
        the sampled attributes in slab order, exactly as ``DensityMap.accumulate`` finds its row.  ValueError
        where the set samples no such attribute."""
        if ps.n != self.n:
            raise ValueError("PathIntegral: the particle set has another particle count")
        k1 = ps.K if n_records is None else int(n_records)
        names = list(names) if names is not None else ["salinity", "temperature"][:ps.n_attr]
        if ps.attr_records is None or name not in names or names.index(name) >= ps.n_attr:
            raise ValueError(f"PathIntegral: the particle set samples no attribute {name!r}")
        if k1 < 0 or k1 > ps.attr_records.shape[0]:
            raise ValueError(f"record range [0, {k1}) outside the slab's {ps.attr_records.shape[0]} slots")
        weight = self._weight(abs(int(ps.cfg.recordT)) if weight is None else weight)
        self._call(ps.n, 0, k1, ps.attr_records.data_ptr() + 8 * names.index(name) * ps.rec_stride,
                   ps.n_attr * ps.rec_stride, 1, ps.ids.data_ptr(), weight, stream)

    def accumulate_lines(self, values, weight, skip_last: bool = True):
        """Add the samples of finished attribute lines ``values`` [n, P] (seed order; CUDA tensor or host array)
        of a SINGLE pair, each times ``weight``, on torch's current stream.  ``skip_last`` (the default) drops
        entry K = P - 1, the 0 the reference appends to an attribute line (mops_traj_finalize_attrs), so the
        sum runs over the pair's K slots as ``accumulate`` does.  Lines concatenated over a chain do not
        qualify: later pairs drop their slot 0 there (the reference's caller removes each later pair's first
        sample), so the concatenation no longer holds every slot; accumulate a chain pair by pair
        (``PathlineChain.run(integrals=)``)."""
        torch = self.torch
        val = torch.as_tensor(values, dtype=torch.float64).to(self.device).contiguous()
        if val.dim() != 2 or int(val.shape[0]) != self.n:
            raise ValueError(f"accumulate_lines: values must be [{self.n}, P]")
        P = int(val.shape[1])
        k1 = P - 1 if skip_last else P
        if k1 < 0:
            raise ValueError("accumulate_lines: no samples")
        self._call(self.n, 0, k1, val.data_ptr(), 1, P, None, self._weight(weight), None)


class FlowMapLattice:
    """One particle per pixel of a ``width`` x ``height`` lat / lon window, and the FTLE image of their flow map
    ("flow-map lattices and FTLE", include/mops_traj.h).

    ``seeds`` is the float64 CUDA tensor [height * width, 3] of the fixed-depth remapping's pixel positions, row
    major, row 0 at ``lat_range[1]`` (mops_flowmap_lattice: formed on the device, never on the host), so the image
    overlays a ``remap_fixed_depth`` image and a ``DensityMap`` image of the same window.  ``wrap_lon``: the window
    spans the whole circle (``lon_range[1] - lon_range[0] == 360.0``), so columns 0 and width - 1 are neighbours.
    ``ftle`` turns the particles' last points (seed order) into a float64 CUDA image [height, width, 4] =
    {ftle, lambda_max, lambda_min, 1}, NaN where a pixel has no valid stencil, for ``colormap_rgba`` and the PNG /
    VTI writers."""

    def __init__(self, width: int, height: int, lat_range, lon_range, device=None):
        import torch
        lat, lon = (float(lat_range[0]), float(lat_range[1])), (float(lon_range[0]), float(lon_range[1]))
        width, height = _image_size(width, height)
        if not (np.isfinite(lat).all() and np.isfinite(lon).all()):
            raise ValueError(f"invalid latitude / longitude range {lat} / {lon}")
        self.torch = torch
        self.width, self.height, self.lat_range, self.lon_range = width, height, lat, lon
        self.n = width * height
        self.wrap_lon = lon[1] - lon[0] == 360.0
        self.cfg = _remap_cfg(width, height, lat, lon)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(self.device):
            self.seeds = torch.empty((self.n, 3), dtype=torch.float64, device=self.device)
            L.check(L.load().mops_flowmap_lattice(C.byref(self.cfg), _tensor_ptr(self.seeds),
                                                  _stream_or_current(None, self.device)), "mops_flowmap_lattice")

    def ftle(self, last_points, death=None, horizon: float = 1.0, stream=None):
        """The FTLE image (mops_ftle_image) of ``last_points`` [height * width, 3] in seed order (CUDA tensor or
        host array); ``death`` [height * width] int32, >= 0 where the particle died (None: a particle counts as
        dead only through a zero or non-finite last point); ``horizon`` > 0, the integration time in the unit the
        exponent is wanted per (days throughout the Python layer).

        Everything runs on ``stream`` (None, a raw handle or a torch stream; default torch's current one): the
        kernel, and before it the torch copies that bring an input into the kernel's form (a non-contiguous
        tensor, a ``death`` of another integer type, a tensor of another device).  CUDA inputs must be ordered on
        that stream by the caller; with them the call does not synchronise the host.  A host array is uploaded
        with torch's blocking copy, which waits for the stream.  The copies are allocated under ``stream``, so
        dropping them here while the kernel may still read them is safe; the image is allocated under torch's
        current stream, as every entry's result is."""
        torch = self.torch
        horizon = float(horizon)
        if not (np.isfinite(horizon) and horizon > 0.0):
            raise ValueError("ftle: the horizon must be finite and positive")
        with _on_stream(stream):
            last = torch.as_tensor(last_points, dtype=torch.float64).to(self.device).contiguous()
            if death is not None:
                death = torch.as_tensor(death).to(device=self.device, dtype=torch.int32).contiguous()
        if last.numel() != 3 * self.n:
            raise ValueError(f"ftle: last_points must be [{self.n}, 3]")
        if death is not None and death.numel() != self.n:
            raise ValueError(f"ftle: death must be [{self.n}]")
        with torch.cuda.device(self.device):
            img = torch.empty((self.height, self.width, 4), dtype=torch.float64, device=self.device)
            L.check(L.load().mops_ftle_image(C.byref(self.cfg), _tensor_ptr(self.seeds), _tensor_ptr(last),
                                             _tensor_ptr(death), horizon, 1 if self.wrap_lon else 0, _tensor_ptr(img),
                                             _stream_or_current(stream, self.device)), "mops_ftle_image")
        return img

    def ftle_from(self, ps: "ParticleSet", horizon: float, stream=None):
        """The FTLE image of a ParticleSet seeded with ``seeds``: its ``last_points()`` and its death steps back
        in seed order.  All of it -- the last points, the reordering of the death steps (torch) and the kernel --
        runs on ``stream`` (default torch's current one) without a host synchronisation, so the call may follow
        the set's ``advance`` / ``compact`` on that stream directly."""
        if ps.n != self.n:
            raise ValueError("ftle_from: the particle set is not this lattice's")
        h = _current_or(stream, self.device)
        last = ps.last_points(stream=h)
        _release_on(last, stream)
        return self.ftle(last, ps.original(ps.death, stream=h), horizon, stream=h)

    def lavd(self, integral, death=None, horizon: float = 1.0, stream=None):
        """The LAVD image (mops_path_integral_image) of a ``PathIntegral`` of this lattice's particles (or its
        ``accum``-like float64 tensor [height * width] in seed order): a float64 CUDA image [height, width, 4] =
        {LAVD, LAVD / horizon, 0, 1}, NaN in channels 0-2 where ``death`` [height * width] is >= 0 or the sum is
        not finite.  ``horizon`` > 0 is in SECONDS here (``ftle`` takes days): with the integral of the
        vorticity deviation under ``PathIntegral``'s rectangle rule -- one record interval of |recordT| seconds
        per slot -- channel 1 is the mean |deviation| along the path in 1/s.  The stream contract is ``ftle``'s:
        the kernel and the torch copies that bring an input into its form run on ``stream`` (default torch's
        current one); CUDA inputs are ordered on that stream by the caller; the image is allocated under torch's
        current stream."""
        torch = self.torch
        horizon = float(horizon)
        if not (np.isfinite(horizon) and horizon > 0.0):
            raise ValueError("lavd: the horizon must be finite and positive")
        acc = integral.accum if isinstance(integral, PathIntegral) else integral
        with _on_stream(stream):
            acc = torch.as_tensor(acc, dtype=torch.float64).to(self.device).contiguous()
            if death is not None:
                death = torch.as_tensor(death).to(device=self.device, dtype=torch.int32).contiguous()
        if acc.numel() != self.n:
            raise ValueError(f"lavd: the integral must be [{self.n}]")
        if death is not None and death.numel() != self.n:
            raise ValueError(f"lavd: death must be [{self.n}]")
        with torch.cuda.device(self.device):
            img = torch.empty((self.height, self.width, 4), dtype=torch.float64, device=self.device)
            L.check(L.load().mops_path_integral_image(self.n, _tensor_ptr(acc), _tensor_ptr(death), horizon,
                                                      _tensor_ptr(img), _stream_or_current(stream, self.device)),
                    "mops_path_integral_image")
        return img
