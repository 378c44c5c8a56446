"""MOPSPathline: the reference's month-pair pathline caller on the device-resident chain.

Mirrors ``MOPSPathline`` of tutorial/pyMOPSAPI.py:1179-1531 -- the same methods, argument meaning,
state and result layout -- so a script written against the tutorial class runs unchanged:

    p = MOPSPathline("mpas.yaml").init("gpu")
    p.set_time(1, 1, 2, 1, direction="forward")          # month pairs (_month_pairs_forward)
    p.set_seed(depth=20.0, lat_range=(18, 31), lon_range=(-98, -80), grid=(40, 40))
    lines = p.run(method="rk4", delta_minutes=1, record_every_minutes=6)

The reference re-registers the grid and both solutions with MOPS and runs one PathLine per pair,
preprocessing every snapshot on the host each time.  Here the whole schedule is one
``chain.PathlineChain`` run: the grid is uploaded once, each snapshot read once (MPASOReader) and
derived on the device, continuation points, per-particle depths and lines stay in HBM, and each pair's
simulationDuration comes from the snapshots' xtime (``_time_gap_seconds``, :1444) -- read ahead with
``MPASOReader.readTimeStamp`` so that every pair's step and record counts are known up front.

State across run() calls is the reference's: after a run, the next run continues the same particles
from their last points (``_first_round`` / ``_last_pt``) until ``reset_segments``.
"""
from __future__ import annotations

import numpy as np

from . import chain as _chain
from . import _lib as L

EARTH_RADIUS_M = _chain.EARTH_RADIUS_M  # pyMOPSAPI.py:46


class MOPSPathline:
    def __init__(self, yaml_path: str):
        self.yaml_path = yaml_path
        self.pairs = None
        self.direction = "forward"
        self._seed_conf = None
        self._seed_points = None
        self._follow_last = True
        self._first_round = True
        self._depth = None
        self._particle_depths = None
        self._last_pt = None
        self._one_min = 60
        self._grid = None
        self._mesh = None   # DeviceMesh, built at the first run (its level count comes from a solution)
        self.device = None

    # ---- MOPSPathline static helpers (pyMOPSAPI.py:1235-1295)
    _month_pairs_forward = staticmethod(_chain.month_pairs_forward)
    _month_pairs_backward = staticmethod(_chain.month_pairs_backward)
    _time_gap_seconds = staticmethod(_chain.time_gap_seconds)

    @staticmethod
    def _to_int_ymd(s: str) -> int:  # "0018-01-01" -> 180101 (pyMOPSAPI.py:1281-1283)
        y, mo, d = s.split("-")
        return int(y) * 10000 + int(mo) * 100 + int(d)

    def reset_segments(self):
        """The next run() starts a new sequence from the configured seeds (pyMOPSAPI.py:1219-1233)."""
        self._first_round = True
        self._last_pt = None

    def init(self, device: str = "gpu"):
        """Load the static grid (pyMOPSAPI.py:1300-1305).  ``device`` is accepted for the reference's
        signature; the engine runs on the current HIP device."""
        import torch
        from .mpas import MPASOReader
        if device not in ("gpu", "cpu", "cuda"):
            raise ValueError(f"unknown device {device!r}")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self._grid = MPASOReader.readGridData(self.yaml_path)
        self._mesh = None
        return self

    def set_time(self, sy: int, sm: int, ey: int, em: int, direction: str = "forward"):
        """Month pairs and direction (pyMOPSAPI.py:1310-1327)."""
        self.direction = direction.lower()
        if self.direction == "forward":
            self.pairs = self._month_pairs_forward(sy, sm, ey, em)
        elif self.direction == "backward":
            self.pairs = self._month_pairs_backward(sy, sm, ey, em)
        else:
            raise ValueError("direction must be 'forward' or 'backward'")
        if not self.pairs:
            raise ValueError("no month pairs produced; check input range")
        return self

    def set_seed(self, depth: float = None, depths=None, lat_range: tuple = None, lon_range: tuple = None,
                 grid: tuple = (2, 2), points=None, follow_last: bool = True):
        """Seeds: explicit (N, 3) points with an optional per-particle depth each, or a lat/lon lattice
        at one depth (pyMOPSAPI.py:1332-1391)."""
        from . import pyMOPS
        self._follow_last = bool(follow_last)
        if depths is not None:
            self._particle_depths = np.asarray(depths, dtype=np.float32).flatten()
            self._depth = float(self._particle_depths[0])
        elif depth is not None:
            self._depth = float(depth)
            self._particle_depths = None
        else:
            raise ValueError("must provide either 'depth' (scalar) or 'depths' (array)")
        if points is not None:
            arr = np.asarray(points, dtype=float)
            if arr.ndim != 2 or arr.shape[1] != 3:
                raise ValueError("points must be a (N,3) array")
            self._seed_points = arr.copy()
            self._seed_conf = None
            if self._particle_depths is not None and len(self._particle_depths) != arr.shape[0]:
                raise ValueError(f"depths length ({len(self._particle_depths)}) must match points count "
                                 f"({arr.shape[0]})")
        else:
            if not (lat_range and lon_range):
                raise ValueError("when points is None, must provide lat_range & lon_range")
            if self._particle_depths is not None:
                raise ValueError("per-particle depths only supported when providing explicit points")
            nx, ny = grid
            conf = pyMOPS.SeedsSettings()
            conf.setSeedsRange((int(nx), int(ny)))
            conf.setGeoBox(tuple(map(float, lat_range)), tuple(map(float, lon_range)))
            conf.setDepth(self._depth)
            self._seed_conf = conf
            self._seed_points = None
        return self

    def _seeds(self):
        from . import pyMOPS
        if self._first_round or not self._follow_last:
            if self._seed_points is not None:
                return self._seed_points.copy()
            return pyMOPS.MOPS_GenerateSeedsPoints(self._seed_conf)
        if self._last_pt is None:
            raise RuntimeError("follow_last=True but last_pts is None")
        return self._last_pt.copy()

    def _make_chain(self, sample_attributes: bool = False, derived_attrs=None):
        """The PathlineChain over the month pairs' snapshots: timestamps read ahead, the mesh uploaded at the
        first call, each snapshot read from its file and derived on the device when its pair needs it.
        ``derived_attrs(mesh) -> make_attrs``: attributes derived from each snapshot's field instead of read from
        its file (chain.derived_attr_factory; the mesh exists only here)."""
        from .chain import PathlineChain
        from .engine import DeviceField, DeviceMesh, cell_to_vertex_attr
        from .mpas import MPASOReader, mesh_from_reader, snapshot_from_reader
        if self.pairs is None:
            raise RuntimeError("call set_time(...) before run()")
        if self._grid is None:
            raise RuntimeError("call init(...) before run()")
        dates = [a for a, _ in self.pairs] + [self.pairs[-1][1]]
        stamps = [MPASOReader.readTimeStamp(self.yaml_path, d, 0) for d in dates]
        if self._mesh is None:
            first = MPASOReader.readSolData(self.yaml_path, dates[0], 0)
            self._mesh = DeviceMesh.from_mesh(mesh_from_reader(self._grid, first.mVertLevels))

        cell_attrs = {}  # snapshot -> its file's cell attributes, from make_field's read to make_attrs

        def make_field(i, stream):  # snapshot i read from its file and derived on the device
            sol = MPASOReader.readSolData(self.yaml_path, dates[i], 0)
            if sample_attributes:
                cell_attrs[i] = {k: v for k, v in sol.attributes.items() if k in ("temperature", "salinity") and v.size}
            return DeviceField.from_snapshot(self._mesh, snapshot_from_reader(sol, timestep_id=i), stream=stream)

        def make_attrs(i, stream):  # (called right after make_field(i), on the same stream)
            return {k: cell_to_vertex_attr(self._mesh, v) for k, v in cell_attrs.pop(i).items()}

        if derived_attrs is not None:
            make_attrs = derived_attrs(self._mesh)
        return PathlineChain(self._mesh, make_field, len(dates), timestamps=stamps, device=self.device,
                             make_attrs=make_attrs if (sample_attributes or derived_attrs is not None) else None)

    def run(self, method: str = "rk4", delta_minutes: int = 1, record_every_minutes: int = 6,
            sample_attributes: bool = False, density=None, layer: int | None = None, diffusivity: float = 0.0,
            seed: int = 0) -> list:
        """All month pairs as one device-resident chain; the per-pair lines concatenated (later pairs
        without their first sample), pyMOPSAPI.py:1396-1531.  Returns list[dict] with lineID, points
        (M, 3), velocity (M, 3), temperature (M,), salinity (M,), lastPoint (3,).
        ``sample_attributes``: temperature / salinity are the snapshot files' fields of those names sampled
        along each line (PathlineChain.run(attrs=True)) instead of the reference's velocity x / y (quirk Q9);
        a name the files do not carry stays zeros.
        ``method``: "rk4" (the reference's, quirk Q1 included), "rk4_relocate" (this engine's RK4 that locates
        each stage in its own cell, MOPS_RK4_RELOCATE: particles survive cell crossings; not with
        ``sample_attributes``); any other string means Euler, as in the reference's caller.
        ``density``: an engine.DensityMap or a list of them, filled with every pair's samples on the device
        (PathlineChain.run(density=...)); a map of "temperature" / "salinity" needs ``sample_attributes``.
        ``layer``: advect within that model layer with w = 0 (PathlineChain.run(layer=...); the depth set by
        ``set_seed`` is still carried, because the records keep their radius); not with ``sample_attributes``.
        ``diffusivity`` (m^2/s), ``seed``: a horizontal random walk on top of the advection
        (PathlineChain.run(diffusivity=, seed=): reproducible to the bit for a given seed); not with
        ``sample_attributes``."""
        if float(diffusivity) > 0.0 and sample_attributes:
            raise ValueError("sample_attributes is not supported with diffusivity > 0")
        if layer is not None and sample_attributes:
            raise ValueError("sample_attributes is not supported with a layer")
        meth = {"rk4": L.MOPS_RK4, "rk4_relocate": L.MOPS_RK4_RELOCATE}.get(method.lower(), L.MOPS_EULER)
        if meth == L.MOPS_RK4_RELOCATE and sample_attributes:
            raise ValueError('sample_attributes is not supported with method="rk4_relocate"')
        if self.pairs is None:
            raise RuntimeError("call set_time(...) before run()")
        if self._depth is None:
            raise RuntimeError("call set_seed(...) before run()")
        if self._grid is None:
            raise RuntimeError("call init(...) before run()")
        seeds = self._seeds()
        pdep = None
        if self._particle_depths is not None:
            pdep = self._particle_depths
            if self._follow_last and not self._first_round:  # :1465-1469
                pdep = np.clip(EARTH_RADIUS_M - np.linalg.norm(seeds, axis=1), 0.0, None).astype(np.float32)
        chain = self._make_chain(bool(sample_attributes))
        res = chain.run(seeds, depth=self._depth, particle_depths=pdep,
                        method=meth,
                        delta_t=int(delta_minutes) * self._one_min,
                        record_t=int(record_every_minutes) * self._one_min,
                        direction=L.MOPS_FORWARD if self.direction == "forward" else L.MOPS_BACKWARD,
                        follow_last=self._follow_last, attrs=bool(sample_attributes), density=density, layer=layer,
                        diffusivity=diffusivity, seed=seed)
        out = {k: res[k].cpu().numpy() for k in ("points", "velocity", "temperature", "salinity", "lastPoint")}
        self._last_pt = out["lastPoint"].astype(float, copy=True)
        if self._particle_depths is not None:  # :1491-1495
            self._particle_depths = np.clip(EARTH_RADIUS_M - np.linalg.norm(self._last_pt, axis=1), 0.0,
                                            None).astype(np.float32)
        self._first_round = False
        return [dict(lineID=i, points=out["points"][i], velocity=out["velocity"][i],
                     temperature=out["temperature"][i], salinity=out["salinity"][i], lastPoint=out["lastPoint"][i])
                for i in range(out["points"].shape[0])]

    def ftle(self, width: int, height: int, lat_range, lon_range, depth: float, method: str = "rk4_relocate",
             delta_minutes: int = 1, record_every_minutes: int = 1440, horizon_days: float | None = None,
             layer: int | None = None, diffusivity: float = 0.0, seed: int = 0):
        """The FTLE image of the month pairs set by ``set_time``: one particle per pixel of the ``width`` x
        ``height`` window (engine.FlowMapLattice, seeded on the device: the pixel positions of a
        ``MOPS_RunRemapping`` image of the same window), integrated at ``depth`` through every pair as one
        device-resident chain that keeps no lines, and the finite-time Lyapunov exponent of the resulting flow
        map -- a float64 CUDA tensor [height, width, 4] = {ftle per day, lambda_max, lambda_min, 1}, NaN where a
        pixel has no valid stencil (land, a particle that died, fewer than two usable neighbours in a
        direction).  A forward run (``set_time(direction="forward")``) shows where the flow pulls neighbours
        apart, a backward run the attracting structures.  A particle that died in any pair is dropped
        (chain.EverDead): one that dies in an early pair is re-seeded from its last record and would otherwise
        pass for alive.  ``horizon_days``: the time the exponent is divided by (default: the sum of the pair
        gaps, in days).  ``method``: as ``run``; the default "rk4_relocate" keeps its particles, while the
        reference's "rk4" kills a particle at its first cell crossing (quirk Q1: two thirds of them within a
        day at config 3), so its map is mostly NaN -- use it only to reproduce the reference's lines.  Does not
        touch the state ``run`` keeps between calls (seeds, last points).  ``layer``: the flow map of that model
        layer (as ``run``), an image that overlays the ``MOPS_RunRemappingFixedLayer`` one.  ``diffusivity``,
        ``seed``: as ``run``."""
        from .chain import EverDead
        from .engine import FlowMapLattice
        meth = {"rk4": L.MOPS_RK4, "rk4_relocate": L.MOPS_RK4_RELOCATE}.get(method.lower(), L.MOPS_EULER)
        chain = self._make_chain(False)
        if horizon_days is None:
            horizon_days = sum(chain.gaps) / 86400.0
        lattice = FlowMapLattice(width, height, lat_range, lon_range, device=self.device)
        ever = EverDead()
        res = chain.run(lattice.seeds, depth=float(depth), method=meth,
                        delta_t=int(delta_minutes) * self._one_min,
                        record_t=int(record_every_minutes) * self._one_min,
                        direction=L.MOPS_FORWARD if self.direction == "forward" else L.MOPS_BACKWARD,
                        follow_last=True, keep_lines=False, on_pair=ever, layer=layer, diffusivity=diffusivity,
                        seed=seed)
        return lattice.ftle(res["lastPoint"], ever.death(), horizon=float(horizon_days))

    def lavd(self, width: int, height: int, lat_range, lon_range, depth: float, method: str = "euler",
             delta_minutes: int = 1, record_every_minutes: int = 60, horizon_days: float | None = None,
             mean_weight=None):
        """The LAVD image of the month pairs set by ``set_time``: the Lagrangian-averaged vorticity deviation, the
        integral of |vorticity - its horizontal mean| along the pathline of one particle per pixel of the
        ``width`` x ``height`` window (engine.FlowMapLattice: the pixel positions of a ``MOPS_RunRemapping`` image
        and of ``ftle`` of the same window), seeded at ``depth`` and integrated through every pair as one
        device-resident chain that keeps no lines.  FTLE shows the transport barriers, LAVD the coherent cores
        they enclose.  Every snapshot's vorticity deviation (engine.vorticity_deviation) is derived from its field
        on the device and sampled inside the trajectory launches; the integral is engine.PathIntegral's
        rectangle rule: slot j of a pair is sampled at the start of step (j+1)*ri - 1 (ri =
        record_every_minutes / delta_minutes) and stands for one record interval.  Returns a float64 CUDA
        tensor [height, width, 4] = {LAVD (dimensionless), mean |deviation| in 1/s, 0, 1}, NaN for a particle
        that died in any pair (chain.EverDead; land included): its later slots hold zeros and would dilute the
        integral.  ``horizon_days``: the time channel 1 is divided by (default: the sum of the pair gaps).
        ``mean_weight``: the float64 CUDA tensor [nCells] the horizontal mean is weighted with (default: the cell
        areas); zero weights confine the mean to a window or basin.  ``method``: "euler" (the default) or
        "rk4" -- the reference's RK4 kills a particle at its first cell crossing (quirk Q1), which leaves a
        mostly-NaN map; "rk4_relocate" is refused with the chain's own message, because the samplers refuse
        it.  Does not touch the state ``run`` keeps between calls (seeds, last points)."""
        from .chain import EverDead, vorticity_deviation_factory
        from .engine import FlowMapLattice, PathIntegral
        meth = {"rk4": L.MOPS_RK4, "rk4_relocate": L.MOPS_RK4_RELOCATE}.get(method.lower(), L.MOPS_EULER)
        name = "vorticity_deviation"
        chain = self._make_chain(False, derived_attrs=lambda mesh: vorticity_deviation_factory(mesh, mean_weight, name))
        if horizon_days is None:
            horizon_days = sum(chain.gaps) / 86400.0
        lattice = FlowMapLattice(width, height, lat_range, lon_range, device=self.device)
        integral = PathIntegral(lattice.n, device=self.device)
        ever = EverDead()
        chain.run(lattice.seeds, depth=float(depth), method=meth,
                  delta_t=int(delta_minutes) * self._one_min,
                  record_t=int(record_every_minutes) * self._one_min,
                  direction=L.MOPS_FORWARD if self.direction == "forward" else L.MOPS_BACKWARD,
                  follow_last=True, keep_lines=False, on_pair=ever, attrs=True, integrals={name: integral})
        return lattice.lavd(integral, ever.death(), horizon=float(horizon_days) * 86400.0)
