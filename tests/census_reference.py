"""Restatement of the eddy census (mops_cell_area, mops_eddy_classify, mops_label_components, mops_eddy_count,
mops_eddy_table and engine.EddyCensus.image) in numpy, with no device.

TEST INFRASTRUCTURE ONLY: the product never imports this module.  Every expression is include/mops_traj.h's ("eddy
census"), as written there, left to right; every sum starts from 0.0 and runs over an eddy's cells in ascending
cell index; only + - * / and sqrt, each of which numpy rounds as IEEE 754 asks.  The labelling is a sequential
union-find over the graph the header defines; the cell area comes from eddy_reference's own A2.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eddy_reference as ER  # noqa: E402

F = np.float64
COLUMNS = ("root", "n_cells", "polarity", "core_cell", "area", "circulation", "ow_min", "centre")


def neighbours(mesh):
    """(nEdgesOnCell [C], cellsOnCell [C, maxEdges] 0-based with -1 for an entry outside 1 .. nCells)."""
    C = int(mesh.nCells)
    nv = np.asarray(mesh.nEdgesOnCell).astype(np.int64).reshape(-1)
    coc = np.asarray(mesh.cellsOnCell).astype(np.int64).reshape(C, -1)
    valid = (coc >= 1) & (coc <= C)
    return nv, np.where(valid, coc - 1, -1)


def edges(mesh, cls):
    """The joined pairs (c, d): d in c's list within nEdgesOnCell[c], a valid cell, equal non-zero classes."""
    nv, coc = neighbours(mesh)
    cls = np.asarray(cls)
    for c in range(len(nv)):
        if cls[c] == 0:
            continue
        for j in range(int(nv[c])):
            d = int(coc[c, j])
            if d >= 0 and cls[d] == cls[c]:
                yield c, d


def label_components(mesh, cls):
    """mops_label_components: int32 [C], the smallest cell index of the cell's component, -1 for class 0."""
    cls = np.asarray(cls)
    parent = list(range(len(cls)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for c, d in edges(mesh, cls):
        a, b = find(c), find(d)
        if a != b:
            parent[max(a, b)] = min(a, b)       # the smaller index stays the root: the root is the minimum
    out = np.full(len(cls), -1, dtype=np.int32)
    for c in range(len(cls)):
        if cls[c] != 0:
            out[c] = find(c)
    return out


def classify(ow, vort, layer, threshold):
    """mops_eddy_classify on [C, L] arrays: int32 [C]."""
    w = np.asarray(ow, dtype=np.float64)[:, layer]
    z = np.asarray(vort, dtype=np.float64)[:, layer]
    with np.errstate(invalid="ignore"):
        below = w < F(threshold)
        return np.where(below & (z > 0), 1, np.where(below & (z < 0), -1, 0)).astype(np.int32)


def cell_area(mesh):
    """mops_cell_area: 0.5 * |A2| with eddy_reference.geometry's A2; NaN where the operator refuses the cell."""
    cc, vc, nv, voc = ER.mesh_tables(mesh)
    out = np.full(len(cc), np.nan)
    for c in range(len(cc)):
        n = int(nv[c])
        if n < 3:
            continue
        A2 = ER.geometry(cc[c], vc[voc[c, :n]])[6]
        if A2 == 0.0 or not np.isfinite(A2):
            continue
        out[c] = F(0.5) * abs(A2)
    return out


def membership(labels, min_cells):
    """mops_eddy_count: (eddy_of_cell int32 [C], E)."""
    labels = np.asarray(labels)
    C = len(labels)
    count = np.zeros(C, dtype=np.int64)
    for c in range(C):
        if labels[c] >= 0:
            count[labels[c]] += 1
    index = np.full(C, -1, dtype=np.int32)
    E = 0
    for c in range(C):
        if labels[c] == c and count[c] >= min_cells:
            index[c] = E
            E += 1
    out = np.array([index[r] if r >= 0 else -1 for r in labels], dtype=np.int32).reshape(C)
    return out, E


def table(mesh, eddy_of_cell, E, cls, area, vort, ow, layer):
    """mops_eddy_table: a dict of the columns, one row per eddy."""
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    vort, ow = np.asarray(vort, dtype=np.float64), np.asarray(ow, dtype=np.float64)
    t = {k: np.empty(E, dtype=np.int32) for k in COLUMNS[:4]}
    t.update({k: np.empty(E, dtype=np.float64) for k in COLUMNS[4:7]})
    t["centre"] = np.empty((E, 3), dtype=np.float64)
    members = [[] for _ in range(E)]
    for c, e in enumerate(eddy_of_cell):
        if e >= 0:
            members[e].append(c)
    with np.errstate(all="ignore"):
        for e in range(E):
            A, G, Sx, Sy, Sz, wmin, core = F(0.0), F(0.0), F(0.0), F(0.0), F(0.0), F(np.inf), -1
            for c in members[e]:
                ar = F(area[c])
                A = A + ar
                G = G + F(vort[c, layer]) * ar
                Sx = Sx + ar * F(cc[c, 0])
                Sy = Sy + ar * F(cc[c, 1])
                Sz = Sz + ar * F(cc[c, 2])
                if ow[c, layer] < wmin:
                    wmin, core = F(ow[c, layer]), c
            nrm = np.sqrt((Sx * Sx + Sy * Sy) + Sz * Sz)
            first = members[e][0]
            t["root"][e], t["n_cells"][e], t["polarity"][e], t["core_cell"][e] = first, len(members[e]), cls[first], core
            t["area"][e], t["circulation"][e], t["ow_min"][e] = A, G, wmin
            t["centre"][e] = (Sx / nrm, Sy / nrm, Sz / nrm)
    return t


def lat_lon_radius(centre, area):
    """The host columns of engine.eddy_census: the same numpy expressions."""
    centre = np.asarray(centre, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return (np.degrees(np.arcsin(centre[:, 2])), np.degrees(np.arctan2(centre[:, 1], centre[:, 0])),
                np.sqrt(np.asarray(area, dtype=np.float64) / np.pi))


def census(mesh, vort, ow, layer, threshold, min_cells, area=None):
    """The whole census at a given threshold: dict(classes, components, labels, E, table)."""
    cls = classify(ow, vort, layer, threshold)
    comp = label_components(mesh, cls)
    eoc, E = membership(comp, min_cells)
    t = table(mesh, eoc, E, cls, cell_area(mesh) if area is None else area, vort, ow, layer)
    t["lat"], t["lon"], t["radius"] = lat_lon_radius(t["centre"], t["area"])
    return dict(classes=cls, components=comp, labels=eoc, E=E, table=t)


def label_image(cells, layer_nan, eddy_of_cell, cls):
    """EddyCensus.image from a cell map [H, W] and the NaN mask of the fixed-layer image: [H, W, 4]."""
    cells = np.asarray(cells).astype(np.int64)
    H, W = cells.shape
    out = np.empty((H, W, 4))
    out[..., 2], out[..., 3] = 0.0, 1.0
    for i in range(H):
        for j in range(W):
            c = cells[i, j]
            ok = 0 <= c < len(eddy_of_cell) and not layer_nan[i, j] and eddy_of_cell[c] >= 0
            out[i, j, 0] = float(eddy_of_cell[c]) if ok else np.nan
            out[i, j, 1] = float(cls[c]) if ok else np.nan
    return out


def component_sizes(labels):
    """{root: size} of a label array."""
    labels = np.asarray(labels)
    roots, counts = np.unique(labels[labels >= 0], return_counts=True)
    return dict(zip(roots.tolist(), counts.tolist()))
