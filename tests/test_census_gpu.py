"""The eddy census on the GPU (mops_cell_area, mops_eddy_classify, mops_label_components, mops_eddy_count,
mops_eddy_table, engine.eddy_census) against the numpy restatement (tests/census_reference.py), bit for bit: the
labelling on synthetic class arrays over the small culled mesh, on the same mesh with its cells numbered
backwards and on the wheel meshes (neighbour slots up to 20); area, classes, membership and table at two
thresholds and three values of min_cells; the label image; the default threshold.

Every test asserts on the restatement first what makes its case worth running, so a mesh that stops exercising
the kernel fails loudly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_case as CC  # noqa: E402
import census_reference as CR  # noqa: E402
import eddy_case as EC  # noqa: E402
import eddy_reference as ER  # noqa: E402
import wide_case as WC  # noqa: E402

pytestmark = pytest.mark.gpu

SYNTHETIC = ("ones", "zeros", "single", "random", "band")


@pytest.fixture(scope="module")
def case(engine_lib, oracle_lib, gpu, small_case):
    from mops_amd import engine
    c = dict(CC.small(oracle_lib, small_case))
    c["O"] = oracle_lib
    c["dm"] = engine.DeviceMesh.from_mesh(c["mesh"])
    c["f0"] = engine.DeviceField.from_snapshot(c["dm"], c["s0"])
    c["classes"] = CC.synthetic_classes(c["mesh"])
    c["grad"] = engine.velocity_gradient(c["dm"], c["f0"], which=("vorticity", "okubo_weiss"))
    for k in c["grad"]:     # the census reads the arrays the restatement read
        assert c["grad"][k].cpu().numpy().tobytes() == np.ascontiguousarray(c["g0"][k]).tobytes(), k
    return c


def _label(dm, cls, rounds=False):
    import torch
    from mops_amd import engine
    got = engine.label_components(dm, torch.from_numpy(np.ascontiguousarray(cls)).cuda(), return_rounds=True)
    lab = got[0].cpu().numpy()
    assert lab.dtype == np.int32 and 1 <= got[1] <= 16
    return (lab, got[1]) if rounds else lab


def _check_synthetic(mesh, name, cls, want):
    """What each synthetic array is there for, asserted on the restatement."""
    sizes = CR.component_sizes(want)
    C = len(cls)
    if name == "ones":          # one component per basin, each crossing many 256-cell blocks
        assert (want >= 0).all() and 1 <= len(sizes) <= 20 and max(sizes.values()) > 1024
    elif name == "zeros":
        assert (want == -1).all()
    elif name == "single":
        assert sizes == {C // 3: 1}
    elif name == "random":      # many tiny components; adjacent cells of opposite class stay apart
        assert len(sizes) > 200 and max(sizes.values()) < 256
        nv, coc = CR.neighbours(mesh)
        assert any(cls[c] * cls[d] < 0 for c in range(C) for d in coc[c, :nv[c]] if d >= 0)
    elif name == "band":        # a ring: most members lie far from its smallest cell
        assert max(sizes.values()) > 100
        root = max(sizes, key=sizes.get)
        members = np.flatnonzero(want == root)
        assert np.median(members) - root > 256


# ---- labelling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SYNTHETIC)
def test_labelling_of_synthetic_classes(case, name):
    mesh, cls = case["mesh"], case["classes"][name]
    assert (np.asarray(mesh.cellsOnCell).astype(np.int64) == 0).any() and mesh.maxEdges == 7      # culled
    want = CR.label_components(mesh, cls)
    _check_synthetic(mesh, name, cls, want)
    got, rounds = _label(case["dm"], cls, rounds=True)
    print(f"{name}: {len(CR.component_sizes(want))} components, {rounds} round(s)")
    assert got.tobytes() == want.tobytes()
    assert _label(case["dm"], cls).tobytes() == got.tobytes()           # two calls, the same bytes


def permuted_mesh_arrays(mesh, perm):
    """The arrays of ``mesh`` with its cells renumbered -- new cell i is old cell perm[i] -- as the keyword
    arguments of engine.DeviceMesh.  Vertices keep their numbers."""
    C, V, maxE = int(mesh.nCells), int(mesh.nVertices), int(mesh.maxEdges)
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(C, dtype=np.int64)
    inv[perm] = np.arange(C)
    coc = np.asarray(mesh.cellsOnCell).astype(np.int64).reshape(C, maxE)
    valid = (coc >= 1) & (coc <= C)
    coc_new = np.where(valid, inv[np.where(valid, coc - 1, 0)] + 1, 0)[perm]
    cov = np.asarray(mesh.cellsOnVertex).astype(np.int64).reshape(V, 3)
    vvalid = (cov >= 1) & (cov <= C)
    cov_new = np.where(vvalid, inv[np.where(vvalid, cov - 1, 0)] + 1, 0)
    return dict(nCells=C, nVertices=V, maxEdges=maxE, nVertLevels=int(mesh.nVertLevels),
                nEdgesOnCell=np.asarray(mesh.nEdgesOnCell).reshape(C)[perm],
                verticesOnCell=np.asarray(mesh.verticesOnCell).reshape(C, maxE)[perm],
                cellsOnCell=coc_new.astype(np.uint64), cellsOnVertex=cov_new.astype(np.uint64),
                cellCoord=np.asarray(mesh.cellCoord, dtype=np.float64).reshape(C, 3)[perm],
                vertexCoord=np.asarray(mesh.vertexCoord, dtype=np.float64))


class _Arrays:
    def __init__(self, kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module")
def reversed_mesh(case):
    from mops_amd import engine
    mesh = case["mesh"]
    perm = np.arange(mesh.nCells)[::-1].copy()
    kw = permuted_mesh_arrays(mesh, perm)
    return perm, _Arrays(kw), engine.DeviceMesh(**kw)


@pytest.mark.parametrize("name", SYNTHETIC)
def test_labelling_with_the_cell_order_reversed(case, reversed_mesh, name):
    """The same classes on the same graph numbered backwards: the parent chains run against the launch order.
    The components are the same sets of cells, each labelled by its largest old index now."""
    perm, rmesh, rdm = reversed_mesh
    cls = case["classes"][name]
    rcls = np.ascontiguousarray(cls[perm])
    want = CR.label_components(rmesh, rcls)
    old = CR.label_components(case["mesh"], cls)
    live = old >= 0
    assert np.array_equal(want >= 0, live[perm])
    # the same partition: old cells c and d share a component iff their new numbers do
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    pairs = {}
    for c in np.flatnonzero(live):
        assert pairs.setdefault(old[c], want[inv[c]]) == want[inv[c]]
    assert len(set(pairs.values())) == len(pairs)
    got = _label(rdm, rcls)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("key", WC.KEYS)
def test_labelling_on_the_wheel_meshes(engine_lib, oracle_lib, gpu, key):
    """maxEdges 7, 12 and 20: the neighbour slots beyond the seventh carry edges of the graph."""
    import torch
    from mops_amd import engine
    mesh, s0, _ = WC.world(key)
    d = WC.derived(key)[0]
    g = ER.velocity_gradient(mesh, d.vertex_vel)
    thr = -0.2 * CC.sigma(g["okubo_weiss"], 0)
    ref = CR.census(mesh, g["vorticity"], g["okubo_weiss"], 0, thr, 1)
    sizes = CR.component_sizes(ref["components"])
    assert mesh.maxEdges == WC.MAX_EDGES[key] and len(sizes) >= 3 and max(sizes.values()) >= 30
    nv, coc = CR.neighbours(mesh)
    if key != "me7":        # valid neighbours sit in slots past the seventh, up to the last one
        assert any(coc[c, nv[c] - 1] >= 0 for c in np.flatnonzero(nv == WC.MAX_EDGES[key]))
    dm = engine.DeviceMesh.from_mesh(mesh)
    assert _label(dm, ref["classes"]).tobytes() == ref["components"].tobytes()
    ones = np.ones(mesh.nCells, dtype=np.int32)      # every slot of every wide cell is an edge of the graph
    assert _label(dm, ones).tobytes() == CR.label_components(mesh, ones).tobytes()
    f = engine.DeviceField.from_snapshot(dm, s0)
    cen = engine.eddy_census(dm, f, layer=0, threshold=thr, min_cells=1)
    assert cen.classes.cpu().numpy().tobytes() == ref["classes"].tobytes()
    assert cen.labels.cpu().numpy().tobytes() == ref["labels"].tobytes()
    assert engine.cell_area(dm).cpu().numpy().tobytes() == CR.cell_area(mesh).tobytes()
    for k in ref["table"]:
        assert cen.table[k].tobytes() == ref["table"][k].tobytes(), (key, k)
    assert isinstance(cen.labels, torch.Tensor) and cen.labels.dtype == torch.int32


# ---- area, classes, membership, table ---------------------------------------------------------------------------
def test_cell_area(case):
    from mops_amd import engine
    want = case["area"]
    assert np.isfinite(want).all() and (want > 0).all()
    got = engine.cell_area(case["dm"]).cpu().numpy()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_cell_area_of_degenerate_cells_is_nan(case):
    """The refusal of mops_cell_area on the device: cells whose vertices all coincide have A2 == 0 exactly and get
    NaN, their neighbours keep their areas.  (n < 3 and a non-finite A2 take the same branch of the same
    condition; the restatement's own refusals of them are held in tests/test_eddy_cpu.py.)"""
    from mops_amd import engine
    mesh = case["mesh"]
    kw = permuted_mesh_arrays(mesh, np.arange(mesh.nCells))
    voc = np.array(kw["verticesOnCell"]).reshape(mesh.nCells, mesh.maxEdges).copy()
    flat = [5, 300, mesh.nCells - 1]            # the first and the last block, and the very last cell
    for c in flat:
        voc[c, :] = voc[c, 0]
    kw["verticesOnCell"] = voc
    want = CR.cell_area(_Arrays(kw))
    assert np.isnan(want[flat]).all() and np.isnan(want).sum() == len(flat)
    keep = np.ones(mesh.nCells, dtype=bool)
    keep[flat] = False
    assert want[keep].tobytes() == case["area"][keep].tobytes()
    got = engine.cell_area(engine.DeviceMesh(**kw)).cpu().numpy()
    assert np.isnan(got[flat]).all() and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("min_cells", CC.MIN_CELLS)
@pytest.mark.parametrize("k_sigma", CC.K_SIGMAS)
def test_census_of_the_small_mesh(case, small_case, k_sigma, min_cells):
    from mops_amd import engine
    ref = CC.census(case["O"], small_case, k_sigma, min_cells)
    all_ = CC.census(case["O"], small_case, k_sigma, 1)
    sizes = CR.component_sizes(all_["components"])
    assert (all_["table"]["polarity"] == 1).any() and (all_["table"]["polarity"] == -1).any()
    if k_sigma == 0.2:
        assert min(sizes.values()) == 1                      # a singleton
    else:
        assert max(sizes.values()) > 256                     # a component that spans workgroups
    if min_cells == 10_000:
        assert ref["E"] == 0
    elif min_cells == 4:
        assert 0 < ref["E"] < all_["E"]
    thr = case["thresholds"][k_sigma]
    cen = engine.eddy_census(case["dm"], case["f0"], layer=CC.LAYER, threshold=thr, min_cells=min_cells)
    assert cen.threshold == thr and cen.n_eddies == ref["E"] and 1 <= cen.rounds <= 16
    print(f"k_sigma {k_sigma}, min_cells {min_cells}: {ref['E']} eddies of {len(sizes)} components, "
          f"largest {max(sizes.values())}, {cen.rounds} round(s)")
    assert cen.classes.cpu().numpy().tobytes() == ref["classes"].tobytes()
    assert cen.components.cpu().numpy().tobytes() == ref["components"].tobytes()
    assert cen.labels.cpu().numpy().tobytes() == ref["labels"].tobytes()
    assert sorted(cen.table) == sorted(ref["table"])
    for k in ref["table"]:
        assert cen.table[k].dtype == ref["table"][k].dtype and cen.table[k].shape == ref["table"][k].shape, k
        assert cen.table[k].tobytes() == ref["table"][k].tobytes(), k
    for e in range(min(ref["E"], 3)):
        assert np.array_equal(cen.cells(e).cpu().numpy(), np.flatnonzero(ref["labels"] == e))
    # a gradient handed in gives the same census without computing it again
    again = engine.eddy_census(case["dm"], case["f0"], layer=CC.LAYER, threshold=thr, min_cells=min_cells,
                               gradient=case["grad"])
    assert again.labels.cpu().numpy().tobytes() == ref["labels"].tobytes()
    for k in ref["table"]:
        assert again.table[k].tobytes() == ref["table"][k].tobytes(), k


def test_a_nan_cell_is_class_zero(case, small_case):
    from mops_amd import engine
    thr = case["thresholds"][0.2]
    ref = CC.census(case["O"], small_case, 0.2, 1)
    victim = int(ref["table"]["core_cell"][np.argmax(ref["table"]["n_cells"])])   # inside the largest eddy
    assert ref["classes"][victim] != 0
    ow = case["g0"]["okubo_weiss"].copy()
    ow[victim, CC.LAYER] = np.nan
    want = CR.census(case["mesh"], case["g0"]["vorticity"], ow, CC.LAYER, thr, 1, area=case["area"])
    assert want["classes"][victim] == 0 and want["labels"][victim] == -1
    import torch
    grad = {"vorticity": case["grad"]["vorticity"], "okubo_weiss": torch.from_numpy(ow).cuda()}
    cen = engine.eddy_census(case["dm"], case["f0"], layer=CC.LAYER, threshold=thr, min_cells=1, gradient=grad)
    assert cen.classes.cpu().numpy().tobytes() == want["classes"].tobytes()
    assert cen.labels.cpu().numpy().tobytes() == want["labels"].tobytes()
    for k in want["table"]:
        assert cen.table[k].tobytes() == want["table"][k].tobytes(), k


def test_label_image(case, small_case):
    from mops_amd import engine
    ref = CC.census(case["O"], small_case, 0.05, 4)
    cen = engine.eddy_census(case["dm"], case["f0"], layer=CC.LAYER, threshold=case["thresholds"][0.05], min_cells=4)
    img, cells, layer_image = cen.image(EC.WIDTH, EC.HEIGHT, EC.LAT, EC.LON, return_cells=True)
    cells, layer_image = cells.cpu().numpy(), layer_image.cpu().numpy()
    assert cells.shape == (EC.HEIGHT, EC.WIDTH)
    assert np.array_equal(cells.reshape(-1), EC.depth_cells(case["O"], small_case))     # the window's own cell map
    nan = np.isnan(layer_image[..., 0])
    want = CR.label_image(cells, nan, ref["labels"], ref["classes"])
    inside = ~np.isnan(want[..., 0])
    assert nan.any() and inside.sum() >= 10 and (~inside & ~nan).any()
    assert len(np.unique(want[..., 0][inside])) >= 2 and {-1.0, 1.0} <= set(np.unique(want[..., 1][inside]))
    got = img.cpu().numpy()
    assert got.shape == (EC.HEIGHT, EC.WIDTH, 4) and got.tobytes() == want.tobytes()
    assert cen.image(EC.WIDTH, EC.HEIGHT, EC.LAT, EC.LON).cpu().numpy().tobytes() == want.tobytes()


def test_default_threshold_is_k_sigma_of_the_layer(case, small_case):
    from mops_amd import engine
    for k in CC.K_SIGMAS:
        cen = engine.eddy_census(case["dm"], case["f0"], layer=CC.LAYER, k_sigma=k, min_cells=1)
        want = case["thresholds"][k]
        assert want < 0 and abs(cen.threshold - want) <= 1e-12 * abs(want)
        ref = CC.census(case["O"], small_case, k, 1, threshold=cen.threshold)       # the value used, handed on
        assert cen.labels.cpu().numpy().tobytes() == ref["labels"].tobytes()
        for name in ref["table"]:
            assert cen.table[name].tobytes() == ref["table"][name].tobytes(), name
    dflt = engine.eddy_census(case["dm"], case["f0"])
    assert abs(dflt.threshold - case["thresholds"][0.2]) <= 1e-12 * abs(dflt.threshold)
    assert dflt.n_eddies == CC.census(case["O"], small_case, 0.2, 4, threshold=dflt.threshold)["E"]
