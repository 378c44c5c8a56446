"""pyMOPS-compatible Python API for the MI355X trajectory engine.

Mirrors the trajectory and image-remapping surface of the reference's pybind
module (tools/pyMOPS/bindings.cpp:23-455): the same enum, class and function
names, the same argument meaning and the same return layout, so a pyMOPS
script runs unchanged with ``from mops_amd import pyMOPS``:

    MOPS_Init / MOPS_Begin / MOPS_AddGridMesh / MOPS_AddAttribute / MOPS_End /
    MOPS_ActiveAttribute                       (bindings.cpp:281-286)
    MOPS_RunRemapping(VisualizationSettings)   -> [ (H, W, 4) float64 ]   (:287-299)
    MOPS_RunReGrid(VisualizationSettings)      -> (H, W, 4) float64       (:301-309)
    MOPS_GenerateSeedsPoints(SeedsSettings)    -> (N, 3) float64   (:311-327)
    MOPS_RunStreamLine(cfg, (N, 3))            -> [ {lineID, points, velocity} ]           (:328-381)
    MOPS_RunPathLine(cfg, (N, 3))              -> [ {lineID, points, velocity, temperature,
                                                     salinity, lastPoint, depth} ]          (:383-455)
    MOPS_ResetTiming / MOPS_PrintTimingSummary / MOPS_PrintTimingDetailed /
    MOPS_GetCategoryTime / MOPS_GetTotalTime   (:457-475)

and, beyond the pybind module, the image output of the reference's C++ side:

    SaveToPNG(image, filename, channel=3)      MOPS::SaveToPNG (src/Common/ImageBuffer.hpp:91-136)
    SaveVTI(images, config, names, outputName) VTKFileManager::SaveVTI (src/IO/VTKFileManager.hpp:25-138)
    MOPS_RunRemappingFixedLayer(config)        extension: Kernel::VisualizeFixedLayer, which MOPS_RunRemapping
                                               never reaches (MOPSApp.cpp:192)
    MOPS_RunDensity(lines, config, value=None) extension: the particle density map of returned lines,
                                               (H, W, 4) float64 {count, mean, sum, 1}
    MOPS_LatticeSeeds(config)                  extension: one seed per pixel of the window, (H*W, 3)
    MOPS_RunFTLE(lines, config, horizon)       extension: the FTLE image of lines seeded on that lattice,
                                               (H, W, 4) float64 {ftle, lambda_max, lambda_min, 1}
    MOPS_RunLAVD(config, traj)                 extension: the Lagrangian-averaged vorticity deviation over the active
                                               pair on that lattice, (H, W, 4) float64 {LAVD, mean, 0, 1}
    MOPS_RunRemappingSection(config)           extension: a vertical section along config.SectionPath,
                                               [ (H, W, 4) float64 ] {zonal, meridional, across, 1} and
                                               {attr0, attr1, 0, 1}
    MOPS_SectionTransport(image, config)       extension: its volume transport in Sverdrups
    MOPS_RunEddyMap(config)                    extension: relative vorticity and Okubo-Weiss at FixedDepth,
                                               (H, W, 4) float64 {vorticity, okubo_weiss, 0, 1}
    MOPS_RunEddyCensus(config)                 extension: the eddies of layer FixedLayer as a list of dicts and
                                               their label image (H, W, 4) float64 {eddy index, polarity, 0, 1}

Every trajectory and every image goes through the HIP engine
(``engine.run_trajectories`` / ``engine.remap_fixed_depth`` /
``engine.remap_fixed_latitude`` on the C ABI); there is no CPU path.
``MPASOReader`` / ``init_from_reader`` load MPAS netCDF classic files
(mops_amd/mpas.py).  ``VisualizationSettings.layerRule`` is the one extension:
"reference" (default) keeps the reference's layer override, "bracket" drops it
(DESIGN.md quirk Q13).
"""
from __future__ import annotations

import enum
import math
import sys
import time
import types

import numpy as np

from . import engine as _E
from . import _lib as _L
from .mpas import MPASOReader  # noqa: F401  (bindings.cpp:88-91: readGridData / readSolData)


class CalcDirection(enum.IntEnum):
    kForward = 0
    kBackward = 1


class CalcMethodType(enum.IntEnum):
    kRK4 = 0
    kEuler = 1


class CalcPositionType(enum.IntEnum):
    kCenter = 0
    kVertx = 1
    kPoint = 2


class CalcAttributeType(enum.IntEnum):
    kZonalMerimoal = 0
    kVelocity = 1
    kZTop = 2
    kTemperature = 3
    kSalinity = 4
    kAll = 5


class VisualizeType(enum.IntEnum):
    kFixedLayer = 0
    kFixedDepth = 1


class SaveType(enum.IntEnum):
    kVTI = 0
    kPNG = 1
    kNone = 2


class GridAttributeType(enum.IntEnum):
    kCellSize = 0
    kEdgeSize = 1
    kVertexSize = 2
    kMaxEdgesSize = 3
    kVertLevels = 4
    kVertLevelsP1 = 5
    kVertexCoord = 6
    kCellCoord = 7
    kEdgeCoord = 8
    kVertexLatLon = 9
    kVerticesOnCell = 10
    kVerticesOnEdge = 11
    kCellsOnVertex = 12
    kCellsOnCell = 13
    kNumberVertexOnCell = 14
    kCellsOnEdge = 15
    kEdgesOnCell = 16
    kCellWeight = 17


class AttributeType(enum.IntEnum):
    kZonalVelocity = 0
    kMeridionalVelocity = 1
    kVelocity = 2
    kNormalVelocity = 3
    kZTop = 4
    kLayerThickness = 5
    kBottomDepth = 6


def _error(msg: str):
    print(f"[Error]: {msg}", file=sys.stderr)


# ---- data model (MPASOGrid.cpp:82-188, MPASOSolution.cpp:1145-1210) -------

_GRID_SCALARS = {GridAttributeType.kCellSize: "mCellsSize", GridAttributeType.kEdgeSize: "mEdgesSize",
                 GridAttributeType.kVertexSize: "mVertexSize", GridAttributeType.kMaxEdgesSize: "mMaxEdgesSize",
                 GridAttributeType.kVertLevels: "mVertLevels", GridAttributeType.kVertLevelsP1: "mVertLevelsP1"}


class MPASOGrid:
    def __init__(self):
        self.mCellsSize = self.mEdgesSize = self.mMaxEdgesSize = self.mVertexSize = 0
        self.mVertLevels = self.mVertLevelsP1 = 0
        self.vec3 = {}
        self.ints = {}
        self.cellRefBottomDepth_vec = np.empty(0)   # [L] (MPASOGrid.h:79), the fixed-latitude image's rows

    def init_from_reader(self, reader):
        """MPASOGrid::initGrid(MPASOReader*) (MPASOGrid.cpp:190-230)."""
        G = GridAttributeType
        self.cellRefBottomDepth_vec = np.asarray(getattr(reader, "cellRefBottomDepth_vec", np.empty(0)), dtype=np.float64)
        self.mCellsSize, self.mEdgesSize = reader.mCellsSize, reader.mEdgesSize
        self.mMaxEdgesSize, self.mVertexSize = reader.mMaxEdgesSize, reader.mVertexSize
        self.mVertLevels, self.mVertLevelsP1 = reader.mVertLevels, reader.mVertLevelsP1
        self.vec3 = {G.kCellCoord: reader.cellCoord_vec, G.kVertexCoord: reader.vertexCoord_vec,
                     G.kEdgeCoord: reader.edgeCoord_vec}
        self.ints = {G.kVerticesOnCell: reader.verticesOnCell_vec, G.kVerticesOnEdge: reader.verticesOnEdge_vec,
                     G.kCellsOnVertex: reader.cellsOnVertex_vec, G.kCellsOnCell: reader.cellsOnCell_vec,
                     G.kNumberVertexOnCell: reader.numberVertexOnCell_vec, G.kCellsOnEdge: reader.cellsOnEdge_vec,
                     G.kEdgesOnCell: reader.edgesOnCell_vec}

    def init_from_yaml(self, yaml_path):
        """MPASOGrid::initGrid_DemoLoading (MPASOGrid.cpp:14-27)."""
        self.init_from_reader(MPASOReader.readGridData(yaml_path))

    def setGridAttribute(self, type, val: int):
        name = _GRID_SCALARS.get(GridAttributeType(type))
        if name is None:
            _error("[MPASOGrid]::Invalid GridAttributeType")
            return
        setattr(self, name, int(val))

    def setGridAttributesVec3(self, type, arr):
        type = GridAttributeType(type)
        if type not in (GridAttributeType.kVertexCoord, GridAttributeType.kCellCoord, GridAttributeType.kEdgeCoord):
            print("Error: Invalid GridAttributeType")
            return
        self.vec3[type] = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1, 3)

    def setGridAttributesVec2(self, type, arr):
        if GridAttributeType(type) != GridAttributeType.kVertexLatLon:
            print("Error: Invalid GridAttributeType")
            return
        self.vertexLatLon = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1, 2)

    def setGridAttributesInt(self, type, arr):
        self.ints[GridAttributeType(type)] = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1)

    def setGridAttributesFloat(self, type, arr):
        self.cellWeight = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)

    def checkAttribute(self) -> bool:
        need_i = (GridAttributeType.kVerticesOnCell, GridAttributeType.kCellsOnVertex, GridAttributeType.kCellsOnCell,
                  GridAttributeType.kNumberVertexOnCell)
        return (self.mCellsSize and self.mVertexSize and self.mMaxEdgesSize and self.mVertLevels
                and GridAttributeType.kCellCoord in self.vec3 and GridAttributeType.kVertexCoord in self.vec3
                and all(t in self.ints for t in need_i))


class MPASOSolution:
    def __init__(self):
        self.mCellsSize = self.mEdgesSize = self.mMaxEdgesSize = self.mVertexSize = 0
        self.mVertLevels = self.mVertLevelsP1 = 0
        self.mTimesteps = 0
        self.mID = ("", 0)                      # SolutionID {timeStamp, timestep} (MPASOSolution.h:12-16)
        self.mTimeStamp = ""
        self.doubles = {}
        self.cellCenterVelocity = None
        self.cellVertVelocity_vec = None        # [C*(L+1)] vertVelocityTop; None => zero
        self.cellSurfaceHeight = None
        self.mDoubleAttributes = {}

    def init_from_reader(self, reader):
        """MPASOSolution::initSolution(MPASOReader*): raw per-cell arrays, sizes and time stamp."""
        A = AttributeType
        self.mVertLevels, self.mVertLevelsP1 = reader.mVertLevels, reader.mVertLevelsP1
        self.mTimesteps = reader.mTimesteps
        self.mTimeStamp = reader.mTimeStamp
        self.mID = (self.mTimeStamp, self.mTimesteps)   # MPASOSolution.cpp:298-299
        self.doubles = {k: v for k, v in ((A.kLayerThickness, reader.cellLayerThickness_vec),
                                          (A.kBottomDepth, reader.cellBottomDepth_vec),
                                          (A.kZonalVelocity, reader.cellZonalVelocity_vec),
                                          (A.kMeridionalVelocity, reader.cellMeridionalVelocity_vec),
                                          (A.kZTop, reader.cellZTop_vec),
                                          (A.kNormalVelocity, reader.cellNormalVelocity_vec)) if v.size}
        self.cellSurfaceHeight = reader.cellSurfaceHeight_vec if reader.cellSurfaceHeight_vec.size else None
        self.cellVertVelocity_vec = reader.cellVertVelocity_vec if reader.cellVertVelocity_vec.size else None
        for k, v in getattr(reader, "attributes", {}).items():
            self.mDoubleAttributes[k] = v

    def init_from_yaml(self, yaml_path, data_name="", timestep=0):
        self.init_from_reader(MPASOReader.readSolData(yaml_path, data_name, timestep))

    def add_attribute(self, name: str, arr=None):
        """Explicit array, or (pyMOPSAPI: ``add_attribute("temperature", AttributeFormat.kFloat)``) a name the
        reader already loaded.  Trajectory outputs carry attributes only where
        ``TrajectorySettings.sampleAttributes`` asks for them (default: the reference's output, quirk Q9)."""
        if arr is not None and not isinstance(arr, (int, enum.Enum)):
            self.mDoubleAttributes[name] = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1)

    def setTimestep(self, t: int):
        self.mTimesteps = int(t)                # like the reference, mID is untouched

    def getID(self) -> int:
        """32-bit FNV-1a of "<timeStamp>_<timestep>" as a signed int (MPASOSolution.h:74-86)."""
        h = 2166136261
        for c in f"{self.mID[0]}_{self.mID[1]}".encode():
            h = ((h ^ c) * 16777619) & 0xFFFFFFFF
        return h - (1 << 32) if h >= (1 << 31) else h

    def getTimeStamp(self) -> str:
        return self.mTimeStamp

    def setAttribute(self, type, val: int):
        name = _GRID_SCALARS.get(GridAttributeType(type))
        if name is None:
            _error("Invalid GridAttributeType")
            return
        setattr(self, name, int(val))

    def setAttributesVec3(self, type, arr):
        if AttributeType(type) != AttributeType.kVelocity:
            _error("Invalid AttributeType")
            return
        self.cellCenterVelocity = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1, 3)

    def setAttributesDouble(self, type, arr):
        self.doubles[AttributeType(type)] = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1)

    def checkAttribute(self) -> bool:
        if AttributeType.kZTop not in self.doubles and AttributeType.kLayerThickness not in self.doubles:
            _error("[MPASOSolution]::Error: Invalid ZTop Attribute")
            return False
        return True


class TrajectorySettings:
    """TrajectorySettings (src/Core/MPASOVisualizer.h:90-103); default method Euler."""

    def __init__(self):
        self.deltaT = 0
        self.simulationDuration = 0
        self.recordT = 0
        self.depth = 0.0
        self.particle_depths = []
        self.fileName = ""
        self.directionType = CalcDirection.kForward
        self.methodType = CalcMethodType.kEuler
        # this engine's extension: MOPS_RunPathLine samples the first two attribute names, in sorted order, that
        # both active solutions carry, and returns them as temperature / salinity BY NAME (see MOPS_RunPathLine)
        self.sampleAttributes = False
        # this engine's extension, the opt-out of quirk Q1: with methodType kRK4, MOPS_RunPathLine locates each RK4
        # stage in its own cell (MOPS_RK4_RELOCATE, include/mops_traj.h) instead of evaluating it in the step's start
        # cell, where a stage across a cell edge kills the particle.  No effect with kEuler (no stages).
        # MOPS_RunStreamLine with it and kRK4, and MOPS_RunPathLine with it, kRK4 and sampleAttributes: Error() and
        # an empty list.
        self.relocateStages = False
        # this engine's extension, the layer mode (mops_traj_advance_layer, include/mops_traj.h): >= 0 makes
        # MOPS_RunStreamLine / MOPS_RunPathLine advect within that model layer with w = 0 (``depth`` is still
        # carried: the records keep their radius); there relocateStages applies to streamlines too.  A layer
        # outside [0, nVertLevels), or sampleAttributes with it: Error() and an empty list.  -1: the depth mode.
        self.fixedLayer = -1
        # a horizontal random walk on top of the advection (TrajectoryConfig.diffusivity; 0: none): Kh in m^2/s,
        # the generator's 64-bit key, and a counter word the caller owns
        self.diffusivity = 0.0
        self.randomSeed = 0
        self.randomEpoch = 0

    def hasPerParticleDepths(self) -> bool:
        return len(self.particle_depths) > 0


class VisualizationSettings:
    """VisualizationSettings as bound by pyMOPS (bindings.cpp:174-218; src/Core/MPASOVisualizer.h:20-42).
    ``layerRule`` ("reference" / "bracket") is this engine's extension."""

    def __init__(self):
        self.imageSize = (0.0, 0.0)         # (width, height)
        self.LatRange = (0.0, 0.0)
        self.LonRange = (0.0, 0.0)
        self.DepthRange = (0.0, 0.0)
        self.FixedLatitude = 0.0
        self.FixedDepth = 0.0
        self.TimeStep = 0.0
        self.tile_index = 0                 # uninitialised in the reference; its CLI prints it into the VTI name
        self.CalcType = CalcAttributeType.kZonalMerimoal
        self.VisType = VisualizeType.kFixedDepth
        self.PositionType = CalcPositionType.kPoint
        self.SaveType = SaveType.kNone
        self.layerRule = "reference"
        # the waypoints (lat, lon) in degrees of MOPS_RunRemappingSection's great-circle path (this engine's
        # extension); its rows span DepthRange, or the reference bottom depths while that is (0, 0)
        self.SectionPath = []
        # MOPS_RunEddyCensus (this engine's extension): the Okubo-Weiss threshold in standard deviations of the
        # layer (the census takes -EddyThreshold * sigma) and the fewest cells an eddy may have
        self.EddyThreshold = 0.2
        self.EddyMinCells = 4

    def __setattr__(self, name, value):
        if name in ("imageSize", "LatRange", "LonRange", "DepthRange"):
            if len(value) != 2:
                raise RuntimeError(f"{name} must be a tuple of size 2")
            value = (float(value[0]), float(value[1]))
        if name == "FixedLayer":  # `union { double FixedDepth; double FixedLayer; }` (MPASOVisualizer.h:31-35)
            name = "FixedDepth"
        object.__setattr__(self, name, value)

    @property
    def FixedLayer(self):
        return self.FixedDepth


class SeedsSettings:
    """SamplingSettings as bound by pyMOPS (bindings.cpp:225-241)."""

    def __init__(self):
        self._range = (0, 0)
        self._lat = (0.0, 0.0)
        self._lon = (0.0, 0.0)
        self._depth = 0.0

    def setSeedsRange(self, t):
        if len(t) != 2:
            raise RuntimeError("sampleRange must be a tuple of size 2")
        self._range = (int(t[0]), int(t[1]))

    def setGeoBox(self, lat, lon):
        if len(lat) != 2 or len(lon) != 2:
            raise RuntimeError("setGeoBox expects two tuples of size 2")
        self._lat = (float(lat[0]), float(lat[1]))
        self._lon = (float(lon[0]), float(lon[1]))

    def setDepth(self, d: float):
        self._depth = float(d)

    def getDepth(self) -> float:
        return self._depth


# ---- timing (src/Utils/Timer.hpp, categories only) ------------------------

_timing = {"by_category": {}, "records": []}


class _Timer:
    def __init__(self, name, cat):
        self.name, self.cat = name, cat

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        ms = (time.perf_counter() - self.t0) * 1e3
        _timing["by_category"][self.cat] = _timing["by_category"].get(self.cat, 0.0) + ms
        _timing["records"].append((self.name, ms))


def MOPS_ResetTiming():
    _timing["by_category"].clear()
    _timing["records"].clear()


def MOPS_PrintTimingSummary():
    print("==== MOPS timing summary (ms) ====")
    for k, v in _timing["by_category"].items():
        print(f"  {k}: {v:.3f}")


def MOPS_PrintTimingDetailed():
    print("==== MOPS timing detailed (ms) ====")
    for k, v in _timing["records"]:
        print(f"  {k}: {v:.3f}")


def MOPS_GetCategoryTime(category: str) -> float:
    return float(_timing["by_category"].get(category, 0.0))


def MOPS_GetTotalTime() -> float:
    return float(sum(_timing["by_category"].values()))


# ---- app state machine (src/Core/MOPS.cpp:10-71, MOPSApp.cpp:34-290) ------

class _App:
    def __init__(self):
        self.configuring = False
        self.grid: MPASOGrid | None = None
        self.sols: dict[int, MPASOSolution] = {}
        self.mesh = None
        self.fields: dict[int, _E.DeviceField] = {}
        self.front = None
        self.back = None
        self.front_id = None
        self.back_id = None
        self.vertex_attrs = {}  # solID -> {name: the attribute's vertex array (device)}, built on first use
        self.eddy_attrs = {}    # solID -> (vorticity, okubo_weiss) vertex arrays (device), built on first use
        self.lavd_attrs = {}    # solID -> the vorticity deviation's vertex array (device), built on first use


_app = _App()


def MOPS_Init(device: str = "gpu"):
    global _app
    _app = _App()
    _app.grid = MPASOGrid()
    _L.load()  # fail loudly here if the HIP engine is missing


def MOPS_Begin():
    _app.configuring = True


def MOPS_AddGridMesh(grid: MPASOGrid):
    with _Timer("Preprocessing::addGrid", "Preprocessing"):
        _app.grid = grid


def MOPS_AddAttribute(solID: int, sol: MPASOSolution):
    with _Timer("Preprocessing::addSol", "Preprocessing"):
        if solID in _app.sols:  # MOPSApp.cpp:82-87
            return
        g = _app.grid
        sol.mCellsSize, sol.mEdgesSize, sol.mMaxEdgesSize, sol.mVertexSize = \
            g.mCellsSize, g.mEdgesSize, g.mMaxEdgesSize, g.mVertexSize
        g.mVertLevels, g.mVertLevelsP1 = sol.mVertLevels, sol.mVertLevelsP1
        _app.sols[solID] = sol


def MOPS_End():
    if not _app.configuring:  # MOPS.cpp:31-46
        print(" [ MOPS is not configuring ]", file=sys.stderr)
        sys.exit(1)
    ok = _app.grid is not None and bool(_app.grid.checkAttribute())
    ok = ok and all(s.checkAttribute() for s in _app.sols.values())
    if not ok:
        print(" [ MOPS is not configured ]", file=sys.stderr)
        sys.exit(1)
    _app.configuring = False
    with _Timer("Preprocessing::upload", "Preprocessing"):
        g = _app.grid
        G = GridAttributeType
        _app.mesh = _E.DeviceMesh(nCells=g.mCellsSize, nVertices=g.mVertexSize, maxEdges=g.mMaxEdgesSize,
                                  nVertLevels=g.mVertLevels, nEdgesOnCell=g.ints[G.kNumberVertexOnCell],
                                  verticesOnCell=g.ints[G.kVerticesOnCell], cellsOnCell=g.ints[G.kCellsOnCell],
                                  cellsOnVertex=g.ints[G.kCellsOnVertex], cellCoord=g.vec3[G.kCellCoord],
                                  vertexCoord=g.vec3[G.kVertexCoord])
        A = AttributeType
        # a solution with the edge-normal velocity only (kNormalVelocity) takes the RBF reconstruction
        # (MPASOSolution::calcCellCenterVelocity), which needs the grid's edges on the device
        rbf = {sid: (s.doubles.get(A.kZonalVelocity) is None or s.doubles.get(A.kMeridionalVelocity) is None)
               and s.doubles.get(A.kNormalVelocity) is not None for sid, s in _app.sols.items()}
        if any(rbf.values()):
            _app.mesh.set_edges(len(g.vec3[G.kEdgeCoord]), g.ints[G.kEdgesOnCell], g.ints[G.kCellsOnEdge],
                                g.vec3[G.kEdgeCoord])
        for sid, s in sorted(_app.sols.items()):
            snap = types.SimpleNamespace(
                timestep=s.mTimesteps, layerThickness=s.doubles.get(A.kLayerThickness),
                bottomDepth=s.doubles.get(A.kBottomDepth), surfaceHeight=s.cellSurfaceHeight,
                zonalVelocity=s.doubles.get(A.kZonalVelocity),
                meridionalVelocity=s.doubles.get(A.kMeridionalVelocity), vertVelocityTop=s.cellVertVelocity_vec,
                normalVelocity=s.doubles.get(A.kNormalVelocity))
            _app.fields[sid] = _E.DeviceField.from_snapshot(_app.mesh, snap,
                                                            velocity="rbf" if rbf[sid] else "zonal")
        if _app.fields:
            _app.front_id = min(_app.fields)
            _app.front = _app.fields[_app.front_id]


def MOPS_ActiveAttribute(t1: int, t2: int | None = None):
    _app.front = _app.back = None
    if t1 not in _app.fields or (t2 is not None and t2 not in _app.fields):
        _error(f"[MOPSApp]::activeAttribute: solID {t1 if t1 not in _app.fields else t2} not found")
        return
    _app.front = _app.fields[t1]
    _app.front_id = t1
    _app.back = None if t2 is None else _app.fields[t2]
    _app.back_id = t2


def MOPS_GenerateSeedsPoints(setting: SeedsSettings) -> np.ndarray:
    """MPASOVisualizer::GenerateSamplePoint (MPASOVisualizer.cpp:120-149): exclusive upper bounds."""
    (min_lat, max_lat), (min_lon, max_lon) = setting._lat, setting._lon
    i_step = (max_lat - min_lat) / float(setting._range[0] - 1)
    j_step = (max_lon - min_lon) / float(setting._range[1] - 1)
    pts = []
    i = min_lat
    while i < max_lat:
        j = min_lon
        while j < max_lon:
            pts.append((j, i))
            j += j_step
        i += i_step
    r = float(np.float32(6371010.0))
    out = np.empty((len(pts), 3))
    for k, (lon_d, lat_d) in enumerate(pts):
        lat, lon = lat_d * (math.pi / 180.0), lon_d * (math.pi / 180.0)
        ct, cp, st, sp = math.cos(lat), math.cos(lon), math.sin(lat), math.sin(lon)
        out[k] = (r * ct * cp, r * ct * sp, r * st)
    return out


def _run(config: TrajectorySettings, sample_points_np, pathline: bool, stage: str):
    a = np.asarray(sample_points_np)
    if a.ndim != 2 or a.shape[1] != 3:
        raise RuntimeError("Input sample_points must be a (N, 3) numpy array.")
    seeds = np.ascontiguousarray(a, dtype=np.float64)
    if config is None or _app.front is None or (pathline and _app.back is None):
        _error(f"[{stage}] invalid inputs")
        return None, seeds, None
    if len(seeds) == 0:
        return None, seeds, None
    if config.deltaT == 0 or config.recordT == 0 or config.simulationDuration == 0:
        _error(f"[{stage}] invalid trajectory settings")
        return None, seeds, None
    depths = None
    if config.hasPerParticleDepths() and len(config.particle_depths) == len(seeds):
        depths = np.asarray(config.particle_depths, dtype=np.float32)
    eff = depths if depths is not None else np.full(len(seeds), np.float32(config.depth), dtype=np.float32)
    method = int(config.methodType)
    layer = int(getattr(config, "fixedLayer", -1))
    if layer >= 0:
        if layer >= _app.mesh.nVertLevels:
            _error(f"[{stage}] fixedLayer {layer} outside [0, {_app.mesh.nVertLevels})")
            return None, seeds, None
        if getattr(config, "sampleAttributes", False):
            _error(f"[{stage}] sampleAttributes is not supported with fixedLayer")
            return None, seeds, None
    if getattr(config, "relocateStages", False) and method == int(CalcMethodType.kRK4):
        if layer >= 0:
            pass  # (the layer mode locates the stages of streamlines and pathlines alike)
        elif not pathline:
            _error(f"[{stage}] relocateStages is for pathlines only")
            return None, seeds, None
        elif getattr(config, "sampleAttributes", False):
            _error(f"[{stage}] sampleAttributes is not supported with relocateStages")
            return None, seeds, None
        method = _L.MOPS_RK4_RELOCATE
    kh = float(getattr(config, "diffusivity", 0.0))
    if not (kh >= 0.0) or not np.isfinite(kh):
        _error(f"[{stage}] diffusivity must be finite and >= 0")
        return None, seeds, None
    if kh > 0.0 and layer < 0 and not pathline:
        _error(f"[{stage}] diffusivity needs fixedLayer for streamlines")
        return None, seeds, None
    if kh > 0.0 and getattr(config, "sampleAttributes", False):
        _error(f"[{stage}] sampleAttributes is not supported with diffusivity")
        return None, seeds, None
    cfg = _E.TrajectoryConfig(deltaT=int(config.deltaT), simulationDuration=int(config.simulationDuration),
                              recordT=int(config.recordT), depth=float(np.float32(config.depth)),
                              direction=int(config.directionType), method=method,
                              layer=layer if layer >= 0 else None, diffusivity=kh,
                              seed=int(getattr(config, "randomSeed", 0)), epoch=int(getattr(config, "randomEpoch", 0)))
    if cfg.n_records <= 0 or cfg.n_steps <= 0:
        _error(f"[{stage}] invalid integration steps")  # seed-only lines (:709-712)
        return "seed_only", seeds, eff
    attrs = None
    if pathline and getattr(config, "sampleAttributes", False):
        # the first two names, sorted (std::map order), that both solutions carry; one is enough (the
        # reference's size() > 1 gate, MPASOVisualizerKernels.cpp:1093, is not kept)
        fs, bs = _app.sols.get(_app.front_id), _app.sols.get(_app.back_id)
        names = sorted(set(fs.mDoubleAttributes) & set(bs.mDoubleAttributes))[:2] if fs and bs else []
        attrs = {k: (_vertex_attr(_app.front_id, k), _vertex_attr(_app.back_id, k)) for k in names}
    r = _E.run_trajectories(_app.mesh, _app.front, _app.back if pathline else None, cfg, seeds, depths=depths,
                            attrs=attrs or None)
    if attrs is not None and not attrs:  # the flag is set and no name is shared: nothing sampled, zeros
        r["temperature"] = np.zeros_like(r["temperature"])
        r["salinity"] = np.zeros_like(r["salinity"])
    return r, seeds, eff


def MOPS_RunStreamLine(config: TrajectorySettings, sample_points_np):
    with _Timer("GPUKernel::StreamLine", "GPUKernel"):
        r, seeds, _ = _run(config, sample_points_np, False, "MI355X::StreamLine")
        if r is None:
            return []
        if isinstance(r, str):  # velocity shorter than points -> NaN rows (bindings.cpp:356-360)
            return [{"lineID": i, "points": seeds[i:i + 1].copy(), "velocity": np.full((1, 3), np.nan)}
                    for i in range(len(seeds))]
        return [{"lineID": i, "points": r["points"][i], "velocity": r["velocity"][i]} for i in range(len(seeds))]


def MOPS_RunPathLine(config: TrajectorySettings, sample_points_np):
    with _Timer("GPUKernel::PathLine", "GPUKernel"):
        if _app.front is None or _app.back is None:  # MOPSApp.cpp:259-271
            _error("[MOPSApp]::Sol_Front or Sol_Back is nullptr, please activeAttribute first")
            sys.exit(-1)
        r, seeds, eff = _run(config, sample_points_np, True, "MI355X::PathLine")
        if r is None:
            return []
        if isinstance(r, str):
            return [{"lineID": i, "points": seeds[i:i + 1].copy(), "velocity": np.zeros((1, 3)),
                     "temperature": np.zeros(1), "salinity": np.zeros(1), "lastPoint": seeds[i].copy(),
                     "depth": float(eff[i])} for i in range(len(seeds))]
        return [{"lineID": i, "points": r["points"][i], "velocity": r["velocity"][i],
                 "temperature": r["temperature"][i], "salinity": r["salinity"][i], "lastPoint": r["lastPoint"][i],
                 "depth": float(eff[i])} for i in range(len(seeds))]


def _vertex_attr(sol_id, name: str):
    """One attribute of one solution as a vertex array on the device (CalcCellCenterToVertex,
    MOPSApp.cpp:121-127: mDoubleAttributes_CtoV), built once per solution id and name."""
    cache = _app.vertex_attrs.setdefault(sol_id, {})
    if name not in cache:
        cache[name] = _E.cell_to_vertex_attr(_app.mesh, _app.sols[sol_id].mDoubleAttributes[name])
    return cache[name]


def _front_vertex_attrs():
    """The active front solution's attribute count and, with two or more, the vertex arrays of the first two
    in name order (the reference's std::map order: mDoubleAttributes_CtoV)."""
    sol = _app.sols.get(_app.front_id)
    names = sorted(sol.mDoubleAttributes) if sol is not None else []
    if len(names) < 2:
        return len(names), ()
    return len(names), tuple(_vertex_attr(_app.front_id, k) for k in names[:2])


def MOPS_RunRemapping(config: VisualizationSettings):
    """MOPSApp::runRemapping (MOPSApp.cpp:171-196) -> a list of [H, W, 4] float64 arrays (bindings.cpp:287-299)."""
    images = _remap_device(config)
    if images is None:
        return []
    host = images.cpu().numpy()
    return [host[k] for k in range(host.shape[0])]


def _remap_device(config: VisualizationSettings):
    """MOPS_RunRemapping's images where the kernel wrote them: one float64 CUDA tensor [n, H, W, 4], or None
    for invalid inputs.  Fixed depth whatever ``VisType`` says, as the reference (MOPSApp.cpp:192).  The CLI
    colours these in place and never copies the doubles to the host."""
    with _Timer("GPUKernel::Remapping", "GPUKernel"):
        if config is None or _app.mesh is None or _app.front is None:  # MPASOVisualizerKernels.cpp:240-243
            _error("[MI355X::VisualizeFixedDepth] invalid inputs")
            return None
        w, h = int(config.imageSize[0]), int(config.imageSize[1])
        n_attr, vattrs = _front_vertex_attrs()
        return _E.remap_fixed_depth(_app.mesh, _app.front, w, h, config.LatRange, config.LonRange,
                                    float(config.FixedDepth), n_attr=n_attr, vertex_attrs=vattrs,
                                    layer_rule=getattr(config, "layerRule", "reference"))


def _eddy_vertex_attrs(sol_id):
    """(vorticity, okubo_weiss) of one solution as signed vertex arrays on the device
    (``engine.velocity_gradient(vertex=True)``), built once per solution id, like ``_vertex_attr``."""
    if sol_id not in _app.eddy_attrs:
        g = _E.velocity_gradient(_app.mesh, _app.fields[sol_id], which=("vorticity", "okubo_weiss"), vertex=True)
        _app.eddy_attrs[sol_id] = (g["vorticity"], g["okubo_weiss"])
    return _app.eddy_attrs[sol_id]


def MOPS_RunEddyMap(config: VisualizationSettings):
    """Extension (no reference counterpart): the relative vorticity and the Okubo-Weiss parameter of the active
    front solution at ``config.FixedDepth`` -> one [H, W, 4] float64 array {vorticity, okubo_weiss, 0, 1}.  It is
    image 1 of the fixed-depth remapping with the two signed vertex arrays as its attributes: the window,
    ``FixedDepth`` and ``layerRule`` of ``MOPS_RunRemapping``, so it overlays the velocity, density and FTLE
    images.  Invalid inputs answer Error() and return []."""
    image = _eddy_device(config)
    return [] if image is None else image.cpu().numpy()


def _eddy_device(config: VisualizationSettings):
    """MOPS_RunEddyMap's image where the kernel wrote it: a float64 CUDA tensor [H, W, 4], or None."""
    with _Timer("GPUKernel::EddyMap", "GPUKernel"):
        w, h = (int(config.imageSize[0]), int(config.imageSize[1])) if config is not None else (0, 0)
        if config is None or _app.mesh is None or _app.front is None or w <= 0 or h <= 0:
            _error("[MI355X::EddyMap] invalid inputs")
            return None
        images = _E.remap_fixed_depth(_app.mesh, _app.front, w, h, config.LatRange, config.LonRange,
                                      float(config.FixedDepth), n_attr=2,
                                      vertex_attrs=_eddy_vertex_attrs(_app.front_id),
                                      layer_rule=getattr(config, "layerRule", "reference"))
        return images[1]


EDDY_KEYS = ("index", "lat", "lon", "radius", "area", "polarity", "circulation", "n_cells", "root", "core_cell",
             "ow_min", "centre")


def _census_layer(config, n_levels: int) -> int:
    """``config.FixedLayer`` as MOPS_RunRemappingFixedLayer reads it: truncated toward zero and clamped into the
    levels (a NaN gives layer 0)."""
    fl = float(config.FixedLayer)
    return 0 if not fl >= 1.0 else (n_levels - 1 if fl >= n_levels else int(fl))


def _census_device(config: VisualizationSettings):
    """MOPS_RunEddyCensus where the kernels wrote it: (engine.EddyCensus, its label image as a float64 CUDA
    tensor [H, W, 4]), or None after Error() for invalid inputs."""
    with _Timer("GPUKernel::EddyCensus", "GPUKernel"):
        w, h = (int(config.imageSize[0]), int(config.imageSize[1])) if config is not None else (0, 0)
        if config is None or _app.mesh is None or _app.front is None or w <= 0 or h <= 0:
            _error("[MI355X::EddyCensus] invalid inputs")
            return None
        try:
            k_sigma, min_cells = float(config.EddyThreshold), int(config.EddyMinCells)
        except (TypeError, ValueError):
            k_sigma, min_cells = float("nan"), 0
        if not np.isfinite(k_sigma) or min_cells < 1:
            _error("[MI355X::EddyCensus] EddyThreshold must be finite and EddyMinCells at least 1")
            return None
        layer = _census_layer(config, _app.mesh.nVertLevels)
        try:
            census = _E.eddy_census(_app.mesh, _app.front, layer=layer, k_sigma=k_sigma, min_cells=min_cells)
        except ValueError as e:  # (a layer without a finite Okubo-Weiss value)
            _error(f"[MI355X::EddyCensus] {e}")
            return None
        return census, census.image(w, h, config.LatRange, config.LonRange)


def _census_rows(census):
    t = census.table
    return [{"index": e, "lat": float(t["lat"][e]), "lon": float(t["lon"][e]), "radius": float(t["radius"][e]),
             "area": float(t["area"][e]), "polarity": int(t["polarity"][e]),
             "circulation": float(t["circulation"][e]), "n_cells": int(t["n_cells"][e]), "root": int(t["root"][e]),
             "core_cell": int(t["core_cell"][e]), "ow_min": float(t["ow_min"][e]),
             "centre": tuple(float(x) for x in t["centre"][e])} for e in range(census.n_eddies)]


def MOPS_RunEddyCensus(config: VisualizationSettings):
    """Extension (no reference counterpart): the eddies of the active front solution at layer
    ``config.FixedLayer`` (clamped as ``MOPS_RunRemappingFixedLayer`` clamps it) -- the connected sets of at
    least ``config.EddyMinCells`` cells whose Okubo-Weiss parameter lies below ``-config.EddyThreshold`` standard
    deviations of the layer, split by the sign of their vorticity (``engine.eddy_census``).  Returns
    ``(eddies, image)``: a list of dicts (``EDDY_KEYS``: lat / lon in degrees, radius in metres, area in square
    metres, polarity +1 / -1 the sign of the vorticity, circulation in m^2/s) and the label image [H, W, 4] float64
    {eddy index, polarity, 0, 1} on the config's window, NaN in channels 0 and 1 outside every eddy.  Invalid
    inputs answer Error() and return ([], [])."""
    got = _census_device(config)
    if got is None:
        return [], []
    return _census_rows(got[0]), got[1].cpu().numpy()


def MOPS_RunRemappingFixedLayer(config: VisualizationSettings):
    """Extension (the reference's MOPSApp has no fixed-layer entry; its kernel is reached through
    MPASOVisualizer::VisualizeFixedLayer): Kernel::VisualizeFixedLayer (MPASOVisualizerKernels.cpp:141-236) of
    the active front solution at ``config.FixedLayer`` -> one [H, W, 4] float64 array {zonal, meridional, 0, 1}."""
    with _Timer("GPUKernel::FixedLayer", "GPUKernel"):
        w, h = (int(config.imageSize[0]), int(config.imageSize[1])) if config is not None else (0, 0)
        if config is None or _app.mesh is None or _app.front is None or w <= 0 or h <= 0:  # :143-161
            _error("[MI355X::VisualizeFixedLayer] invalid inputs")
            return np.zeros((max(h, 0), max(w, 0), 4))
        image = _E.remap_fixed_layer(_app.mesh, _app.front, w, h, config.LatRange, config.LonRange,
                                     float(config.FixedLayer))
        return image.cpu().numpy()


def _section_inputs(config, who: str):
    """(width, height, waypoints, depth range) of a section, or None after Error() for invalid inputs."""
    w, h = (int(config.imageSize[0]), int(config.imageSize[1])) if config is not None else (0, 0)
    if config is None or w <= 0 or h <= 0:
        _error(f"[MI355X::{who}] invalid inputs")
        return None
    try:
        path = [(float(lat), float(lon)) for lat, lon in getattr(config, "SectionPath", [])]
    except (TypeError, ValueError):
        _error(f"[MI355X::{who}] SectionPath must be a list of (lat, lon)")
        return None
    drange = tuple(config.DepthRange)
    if drange == (0.0, 0.0):
        ref = np.zeros(0) if _app.grid is None else \
            np.asarray(_app.grid.cellRefBottomDepth_vec, dtype=np.float64).reshape(-1)
        if ref.size == 0:
            _error(f"[MI355X::{who}] refBottomDepth is empty")
            return None
        drange = (float(ref[0]), float(ref[-1]))
    return w, h, path, drange


def MOPS_RunRemappingSection(config: VisualizationSettings):
    """Extension: a vertical section of the active front solution (engine.remap_section) along the great-circle
    legs through ``config.SectionPath``, ``imageSize`` = (columns, rows), rows over ``config.DepthRange`` (the
    reference bottom depths' first and last while it is (0, 0)).  Returns [image0] or, with double attributes,
    [image0, image1], [H, W, 4] float64 arrays: image0 = {zonal, meridional, across, 1}, image1 = the first two
    attributes in name order (as MOPS_RunRemapping chooses them), {attr0, attr1 or 0, 0, 1}.  Invalid inputs
    (no solution, a bad image size or path): Error() and an empty list."""
    images = _section_device(config)
    if images is None:
        return []
    host = images.cpu().numpy()
    return [host[k] for k in range(host.shape[0])]


def _section_device(config: VisualizationSettings):
    """MOPS_RunRemappingSection's images where the kernel wrote them: one float64 CUDA tensor [1 or 2, H, W, 4],
    or None after Error() for invalid inputs (the CLI colours these in place, as _remap_device's)."""
    with _Timer("GPUKernel::Section", "GPUKernel"):
        got = _section_inputs(config, "Section")
        if got is None:
            return None
        if _app.mesh is None or _app.front is None:
            _error("[MI355X::Section] invalid inputs")
            return None
        w, h, path, drange = got
        sol = _app.sols.get(_app.front_id)
        names = sorted(sol.mDoubleAttributes)[:2] if sol is not None else []
        try:
            images, _ = _E.remap_section(_app.mesh, _app.front, path, w, h, drange,
                                         vertex_attrs=tuple(_vertex_attr(_app.front_id, k) for k in names))
        except ValueError as e:
            _error(f"[MI355X::Section] {e}")
            return None
        return images


def MOPS_SectionTransport(image, config: VisualizationSettings):
    """Extension: the volume transport in Sverdrups (1e6 m^3/s) through a section image of
    MOPS_RunRemappingSection(config) -- its across channel times ds * dz over the non-NaN pixels, one fixed-order
    FP64 sum on the host (engine.section_transport), positive to the left of the direction of travel.  Invalid
    inputs: Error() and NaN."""
    with _Timer("Section::Transport", "GPUKernel"):
        got = _section_inputs(config, "SectionTransport")
        if got is None:
            return float("nan")
        w, h, path, drange = got
        try:
            _, _, dist = _E.section_points(path, w)
            sv, _ = _E.section_transport(image, dist, drange)
        except ValueError as e:
            _error(f"[MI355X::SectionTransport] {e}")
            return float("nan")
        return sv


def MOPS_RunDensity(lines, config: VisualizationSettings, value=None):
    """Extension (the reference's own plot helper, Vis_PathLines in tutorial/pyMOPSAPI.py:132-289, draws one
    matplotlib line per trajectory): the particle density map of ``lines`` -- the list[dict] MOPS_RunStreamLine /
    MOPS_RunPathLine return -- on the window ``config`` gives (imageSize, LatRange, LonRange), binned on the
    GPU (engine.DensityMap): one [H, W, 4] float64 array {count, mean, sum, 1} with NaN where no sample fell,
    usable with SaveToPNG and SaveVTI as MOPS_RunRemapping's images are.  Every point of every line is binned;
    ``value``: None (count only), "speed" (|velocity|), "temperature" or "salinity" (the lines' entries of
    that name).  Invalid inputs: Error() and an empty image, as MOPS_RunReGrid."""
    with _Timer("GPUKernel::Density", "GPUKernel"):
        w, h = (int(config.imageSize[0]), int(config.imageSize[1])) if config is not None else (0, 0)
        key = {None: None, "": None, "speed": "velocity", "temperature": "temperature", "salinity": "salinity"}
        lines = list(lines) if lines is not None else None
        if (config is None or lines is None or w <= 0 or h <= 0 or value not in key
                or any("points" not in ln or (key[value] is not None and key[value] not in ln) for ln in lines)):
            _error("[MI355X::Density] invalid inputs")
            return np.zeros((max(h, 0), max(w, 0), 4))
        try:
            dmap = _E.DensityMap(w, h, config.LatRange, config.LonRange, value=value or None)
        except ValueError as e:
            _error(f"[MI355X::Density] {e}")
            return np.zeros((h, w, 4))
        n = len(lines)
        P = max([np.asarray(ln["points"]).reshape(-1, 3).shape[0] for ln in lines], default=0)
        if n and P:
            # lines of unequal length are padded with NaN points, which the binning skips
            pts = np.full((n, P, 3), np.nan)
            val = None if key[value] is None else np.full((n, P, 3) if value == "speed" else (n, P), np.nan)
            for i, ln in enumerate(lines):
                q = np.asarray(ln["points"], dtype=np.float64).reshape(-1, 3)
                pts[i, :q.shape[0]] = q
                if val is not None:
                    v = np.asarray(ln[key[value]], dtype=np.float64).reshape((-1, 3) if value == "speed" else (-1,))
                    m = min(q.shape[0], v.shape[0])
                    val[i, :m] = v[:m]
            dmap.accumulate_lines(pts, val)
        return dmap.image(nan_empty=True).cpu().numpy()


def _lattice(config, who: str):
    """engine.FlowMapLattice of config's window, or None after Error() for invalid inputs."""
    w, h = (int(config.imageSize[0]), int(config.imageSize[1])) if config is not None else (0, 0)
    if config is None or w <= 0 or h <= 0:
        _error(f"[MI355X::{who}] invalid inputs")
        return None
    try:
        return _E.FlowMapLattice(w, h, config.LatRange, config.LonRange)
    except ValueError as e:
        _error(f"[MI355X::{who}] {e}")
        return None


def MOPS_LatticeSeeds(config: VisualizationSettings):
    """Extension ("flow-map lattices and FTLE", include/mops_traj.h): one seed per pixel of ``config``'s window
    (imageSize, LatRange, LonRange) as an (H*W, 3) float64 array, row major -- the positions MOPS_RunRemapping's
    image has its pixels at, formed on the GPU (engine.FlowMapLattice).  Run them with MOPS_RunPathLine /
    MOPS_RunStreamLine and give the lines, in this order, to MOPS_RunFTLE.  Invalid inputs: Error() and an empty
    (0, 3) array."""
    with _Timer("GPUKernel::LatticeSeeds", "GPUKernel"):
        lat = _lattice(config, "LatticeSeeds")
        return np.zeros((0, 3)) if lat is None else lat.seeds.cpu().numpy()


def MOPS_RunFTLE(lines, config: VisualizationSettings, horizon: float):
    """Extension: the finite-time Lyapunov exponent image of ``lines`` -- the list[dict] MOPS_RunPathLine /
    MOPS_RunStreamLine return for the seeds of MOPS_LatticeSeeds(config), in that order -- on the GPU
    (engine.FlowMapLattice.ftle): the flow map is ``points[0]`` -> ``lastPoint`` of each line.  No death array is
    passed: a dead line has a zero ``lastPoint``, which is not valid.  One [H, W, 4] float64 array {ftle,
    lambda_max, lambda_min, 1}, NaN where a pixel has no valid stencil, usable with SaveToPNG and SaveVTI.
    ``horizon`` > 0: the integration time in the unit the exponent is wanted per.  Invalid inputs (a line count
    other than H * W, a line without ``points`` / ``lastPoint``, a bad horizon): Error() and an empty image."""
    with _Timer("GPUKernel::FTLE", "GPUKernel"):
        lat = _lattice(config, "FTLE")
        if lat is None:
            return np.zeros((0, 0, 4))
        lines = list(lines) if lines is not None else None
        try:
            hz = float(horizon)
        except (TypeError, ValueError):
            hz = float("nan")
        if (lines is None or len(lines) != lat.n or not (np.isfinite(hz) and hz > 0.0)
                or any("points" not in ln or "lastPoint" not in ln for ln in lines)):
            _error("[MI355X::FTLE] invalid inputs")
            return np.zeros((0, 0, 4))
        seeds = np.zeros((lat.n, 3))
        last = np.zeros((lat.n, 3))
        for i, ln in enumerate(lines):
            q = np.asarray(ln["points"], dtype=np.float64).reshape(-1, 3)
            if q.shape[0]:  # (a line without points keeps zeros, which are not valid)
                seeds[i] = q[0]
                last[i] = np.asarray(ln["lastPoint"], dtype=np.float64).reshape(3)
        lat.seeds.copy_(lat.torch.as_tensor(seeds))  # points[0] of each line (the lattice seed itself, from a run)
        return lat.ftle(last, None, hz).cpu().numpy()


def _lavd_vertex_attr(sol_id):
    """The vorticity deviation of one solution as a signed vertex array on the device
    (``engine.vorticity_deviation``: area-weighted mean), built once per solution id, like ``_eddy_vertex_attrs``."""
    if sol_id not in _app.lavd_attrs:
        _app.lavd_attrs[sol_id] = _E.vorticity_deviation(_app.mesh, _app.fields[sol_id], vertex=True)[0]
    return _app.lavd_attrs[sol_id]


LAVD_ATTRIBUTE = "vorticity_deviation"


def MOPS_RunLAVD(config: VisualizationSettings, traj: TrajectorySettings):
    """Extension ("path integrals and LAVD", include/mops_traj.h): the Lagrangian-averaged vorticity deviation
    over the active front / back pair.  One particle per pixel of ``config``'s window (MOPS_LatticeSeeds) at
    ``config.FixedDepth`` runs one pathline with ``traj``'s deltaT, simulationDuration, recordT, direction and
    method; each solution's vorticity deviation (its vorticity minus the area-weighted mean of its level) is the
    single sampled attribute, and the sampled line is summed with the rectangle rule -- slot j, sampled at the
    start of step (j+1)*ri - 1, times recordT seconds (engine.PathIntegral.accumulate_lines).  One [H, W, 4]
    float64 array {LAVD, mean |deviation| in 1/s over K * recordT seconds, 0, 1}, NaN where the particle died
    (land included), usable with SaveToPNG and SaveVTI; it overlays the velocity, density, FTLE and eddy images
    of the same window.  kRK4 evaluates its stages in the step's start cell (quirk Q1) and leaves a mostly-NaN
    map.  Invalid inputs -- no back solution, ``fixedLayer`` >= 0, ``relocateStages``, ``diffusivity`` > 0, bad
    sizes or trajectory settings -- answer Error() and return an empty image."""
    with _Timer("GPUKernel::LAVD", "GPUKernel"):
        empty = np.zeros((0, 0, 4))
        if traj is None or _app.mesh is None or _app.front is None or _app.back is None:
            _error("[MI355X::LAVD] invalid inputs: it needs a TrajectorySettings and an active front / back pair")
            return empty
        if int(getattr(traj, "fixedLayer", -1)) >= 0:
            _error("[MI355X::LAVD] attributes are not sampled with fixedLayer")
            return empty
        if getattr(traj, "relocateStages", False):
            _error("[MI355X::LAVD] attributes are not sampled with relocateStages")
            return empty
        kh = float(getattr(traj, "diffusivity", 0.0))
        if not kh == 0.0:
            _error("[MI355X::LAVD] attributes are not sampled with diffusivity > 0")
            return empty
        cfg = _E.TrajectoryConfig(deltaT=int(traj.deltaT), simulationDuration=int(traj.simulationDuration),
                                  recordT=int(traj.recordT), depth=float(np.float32(config.FixedDepth))
                                  if config is not None else 0.0, direction=int(traj.directionType),
                                  method=int(traj.methodType))
        if cfg.n_records <= 0 or cfg.n_steps <= 0:
            _error("[MI355X::LAVD] invalid trajectory settings")
            return empty
        lat = _lattice(config, "LAVD")
        if lat is None:
            return empty
        attrs = {LAVD_ATTRIBUTE: (_lavd_vertex_attr(_app.front_id), _lavd_vertex_attr(_app.back_id))}
        r = _E.run_trajectories(_app.mesh, _app.front, _app.back, cfg, lat.seeds.cpu().numpy(), attrs=attrs)
        integral = _E.PathIntegral(lat.n)
        integral.accumulate_lines(r["attributes"][LAVD_ATTRIBUTE], float(abs(cfg.recordT)))
        return lat.lavd(integral, r["death_step"], horizon=float(cfg.n_records * abs(cfg.recordT))).cpu().numpy()


def SaveToPNG(image, filename: str, channel: int = 3) -> bool:
    """MOPS::SaveToPNG (ImageBuffer.hpp:91-136): one channel of an [H, W, 4] image (numpy or CUDA tensor)
    through the Viridis map into an RGBA PNG; the colouring runs on the GPU (io.save_image_png)."""
    from . import io as _io
    with _Timer("IO::SavePNG", "IO"):
        return _io.save_image_png(filename, image, channel)


def TypeToStr(vis_type) -> str:
    """VTKFileManager.hpp:12-20."""
    return {int(VisualizeType.kFixedLayer): "fixed_layer_", int(VisualizeType.kFixedDepth): "fixed_depth_"}.get(
        int(vis_type), "unknown_")


def vti_file_name(config: VisualizationSettings, outputName: str = "output") -> str:
    """outputName + "_" + TypeToStr(VisType) + std::to_string(k) + ".vti" (VTKFileManager.hpp:74, :133);
    std::to_string(double) prints "%f": fixed_depth_10.000000."""
    return f"{outputName}_{TypeToStr(config.VisType)}{float(config.FixedDepth):f}.vti"


def SaveVTI(images, config: VisualizationSettings, names=(), outputName: str = "output") -> str:
    """VTKFileManager::SaveVTI (VTKFileManager.hpp:25-138).  A list (or [n, H, W, 4] array) of images takes the
    multi-attribute overload: three one-component arrays per image, named from ``names`` then "attr_<i>",
    z spacing 1.  One [H, W, 4] image takes the single-image overload: one 3-component array "ImageScalars",
    z spacing k.  Origin (LonRange[0], LatRange[0], k), spacing range / (size - 1), k = FixedDepth / FixedLayer
    (one union).  Returns the file name written."""
    from . import io as _io
    with _Timer("IO::SaveVTI", "IO"):
        k = float(config.FixedDepth)
        w, h = config.imageSize
        with np.errstate(all="ignore"):
            lat_sp = float(np.float64(config.LatRange[1] - config.LatRange[0]) / np.float64(h - 1))
            lon_sp = float(np.float64(config.LonRange[1] - config.LonRange[0]) / np.float64(w - 1))
        origin = (config.LonRange[0], config.LatRange[0], k)
        name = vti_file_name(config, outputName)
        single = not isinstance(images, (list, tuple)) and getattr(images, "ndim", 0) == 3
        if single:
            _io.save_image_vti(name, images, origin, (lon_sp, lat_sp, k))
        else:
            _io.save_images_vti(name, images, origin, (lon_sp, lat_sp, 1.0), names)
        return name


def MOPS_RunReGrid(config: VisualizationSettings):
    """MOPSApp::runReGrid (MOPSApp.cpp:198-210) -> one [H, W, 4] float64 array (bindings.cpp:301-309)."""
    with _Timer("GPUKernel::ReGrid", "GPUKernel"):
        w, h = int(config.imageSize[0]), int(config.imageSize[1])
        if _app.mesh is None or _app.front is None or w <= 0 or h <= 0:  # MPASOVisualizerKernels.cpp:475-485
            _error("[MI355X::VisualizeFixedLatitude] invalid inputs")
            return np.zeros((max(h, 0), max(w, 0), 4))
        ref = np.asarray(_app.grid.cellRefBottomDepth_vec, dtype=np.float64).reshape(-1)
        if ref.size == 0:  # :491-494
            _error("[MI355X::VisualizeFixedLatitude] refBottomDepth is empty")
            return np.zeros((h, w, 4))
        image = _E.remap_fixed_latitude(_app.mesh, _app.front, w, h, config.LonRange, float(config.FixedLatitude),
                                        (float(ref[0]), float(ref[-1])))
        return image.cpu().numpy()
