"""GPU: pyMOPS.TrajectorySettings.sampleAttributes -- MOPS_RunPathLine's temperature / salinity become the
sampled attributes of those names (tests/pathline_attr_reference.py is the reference); off, nothing changes."""
import numpy as np
import pytest

import pathline_attr_reference as R

pytestmark = pytest.mark.gpu

K = R.DURATION // R.RECORD_T


def _setup(mesh, snaps, attr_names):
    """The app as the reference's Python tutorials configure it; snapshot t carries ``attr_names[t]``."""
    from mops_amd import pyMOPS as M
    G, A = M.GridAttributeType, M.AttributeType
    M.MOPS_Init("gpu")
    M.MOPS_Begin()
    g = M.MPASOGrid()
    g.setGridAttribute(G.kCellSize, mesh.nCells)
    g.setGridAttribute(G.kVertexSize, mesh.nVertices)
    g.setGridAttribute(G.kMaxEdgesSize, mesh.maxEdges)
    g.setGridAttributesVec3(G.kCellCoord, mesh.cellCoord)
    g.setGridAttributesVec3(G.kVertexCoord, mesh.vertexCoord)
    g.setGridAttributesInt(G.kNumberVertexOnCell, mesh.nEdgesOnCell)
    g.setGridAttributesInt(G.kVerticesOnCell, mesh.verticesOnCell)
    g.setGridAttributesInt(G.kCellsOnCell, mesh.cellsOnCell)
    g.setGridAttributesInt(G.kCellsOnVertex, mesh.cellsOnVertex)
    M.MOPS_AddGridMesh(g)
    for t, s in enumerate(snaps):
        sol = M.MPASOSolution()
        sol.setTimestep(t)
        sol.setAttribute(G.kVertLevels, mesh.nVertLevels)
        sol.setAttribute(G.kVertLevelsP1, mesh.nVertLevels + 1)
        sol.setAttributesDouble(A.kLayerThickness, s.layerThickness)
        sol.setAttributesDouble(A.kBottomDepth, s.bottomDepth)
        sol.setAttributesDouble(A.kZonalVelocity, s.zonalVelocity)
        sol.setAttributesDouble(A.kMeridionalVelocity, s.meridionalVelocity)
        sol.cellVertVelocity_vec = s.vertVelocityTop
        for name in attr_names[t]:
            sol.add_attribute(name, s.attributes[name])
        M.MOPS_AddAttribute(t, sol)
    M.MOPS_End()
    M.MOPS_ActiveAttribute(0, 1)
    return M


def _settings(M, ref, sample):
    cfg = M.TrajectorySettings()
    assert cfg.sampleAttributes is False
    cfg.deltaT, cfg.simulationDuration, cfg.recordT, cfg.depth = R.DELTA_T, R.DURATION, R.RECORD_T, 0.0
    cfg.methodType = M.CalcMethodType.kRK4
    cfg.particle_depths = list(ref["depths"])
    cfg.sampleAttributes = sample
    return cfg


@pytest.fixture(scope="module")
def ref(oracle_lib, small_case):
    mesh, s0, s1 = small_case
    return R.run_shared(oracle_lib, mesh, oracle_lib.preprocess(mesh, s0), oracle_lib.preprocess(mesh, s1), False, False)


def test_pymops_sampled_attributes(engine_lib, oracle_lib, gpu, small_case, ref):
    mesh, s0, s1 = small_case
    both = ("temperature", "salinity")
    M = _setup(mesh, (s0, s1), (both, both))
    want = R.attr_lines(oracle_lib, ref["seeds"], ref, K)        # names sorted: salinity, temperature
    assert ref["names"] == ["salinity", "temperature"]
    off = M.MOPS_RunPathLine(_settings(M, ref, False), ref["seeds"])
    on = M.MOPS_RunPathLine(_settings(M, ref, True), ref["seeds"])
    sl = M.MOPS_RunStreamLine(_settings(M, ref, True), ref["seeds"])   # the flag is ignored
    assert len(on) == len(off) == R.N_SEEDS and set(sl[0]) == {"lineID", "points", "velocity"}
    for i in range(R.N_SEEDS):
        assert np.array_equal(on[i]["temperature"], want[1, i])
        assert np.array_equal(on[i]["salinity"], want[0, i])
        for k in ("points", "velocity", "lastPoint"):
            assert on[i][k].tobytes() == off[i][k].tobytes(), k
        # flag off: today's output (quirk Q9)
        assert np.array_equal(off[i]["temperature"], off[i]["velocity"][:, 0])
        assert np.array_equal(off[i]["salinity"], off[i]["velocity"][:, 1])
    alive = ref["death"] < 0
    assert any(on[i]["temperature"][:K].all() for i in np.flatnonzero(alive))
    # the remapping still gets the first two attributes' vertex arrays from the generalised cache
    n_attr, va = M._front_vertex_attrs()
    assert n_attr == 2 and va[0] is M._vertex_attr(0, "salinity") and va[1] is M._vertex_attr(0, "temperature")


def test_pymops_one_shared_name(engine_lib, oracle_lib, gpu, small_case, ref):
    """The back solution carries only salinity: salinity is sampled, temperature is zeros."""
    mesh, s0, s1 = small_case
    M = _setup(mesh, (s0, s1), (("temperature", "salinity"), ("salinity",)))
    want = R.attr_lines(oracle_lib, ref["seeds"], ref, K)
    on = M.MOPS_RunPathLine(_settings(M, ref, True), ref["seeds"])
    for i in range(R.N_SEEDS):
        assert np.array_equal(on[i]["salinity"], want[0, i])
        assert not on[i]["temperature"].any()
