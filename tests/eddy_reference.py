"""Restatement of the velocity-gradient operator (mops_velocity_gradient) and of the unclamped barycentric
cell-to-vertex interpolation (mops_cell_to_vertex_signed) in numpy float64.

TEST INFRASTRUCTURE ONLY: the product never imports this module.  Every expression is include/mops_traj.h's
("velocity gradient"), as written there, left to right; every sum starts from 0.0 and runs over k = 0 .. n-1 in
order; only + - * / and sqrt, each of which numpy rounds as IEEE 754 asks.  The loops over cells and vertices
are Python loops; the levels of one cell are carried as one float64 vector, whose element-wise operations are
the scalar ones.
"""
import numpy as np

F = np.float64
NAMES = ("vorticity", "divergence", "strain", "okubo_weiss")


def frame(c):
    """(e, nn): the east and north unit vectors at the cell centre c, convertXYZVelocityToENU's expressions."""
    cx, cy, cz = F(c[0]), F(c[1]), F(c[2])
    with np.errstate(all="ignore"):
        Rxy = np.sqrt(cx * cx + cy * cy)
        if Rxy == 0.0:
            return (F(1.0), F(0.0), F(0.0)), (F(0.0), F(1.0) if cz > 0.0 else F(-1.0), F(0.0))
        Rxyz = np.sqrt((cx * cx + cy * cy) + cz * cz)
        clon, slon, slat, clat = cx / Rxy, cy / Rxy, cz / Rxyz, Rxy / Rxyz
        return (-slon, clon, F(0.0)), (-slat * clon, -slat * slon, clat)


def geometry(c, poly):
    """(e, nn, xi, eta, gx, gy, A2) of a cell with centre c and vertices poly [n, 3] in verticesOnCell order."""
    e, nn = frame(c)
    n = len(poly)
    xi, eta = [], []
    with np.errstate(all="ignore"):
        for k in range(n):
            dx, dy, dz = F(poly[k][0]) - F(c[0]), F(poly[k][1]) - F(c[1]), F(poly[k][2]) - F(c[2])
            xi.append((dx * e[0] + dy * e[1]) + dz * e[2])
            eta.append((dx * nn[0] + dy * nn[1]) + dz * nn[2])
        A2 = F(0.0)
        gx, gy = [], []
        for k in range(n):
            kp, km = (k + 1) % n, (k - 1) % n
            A2 = A2 + (xi[k] * eta[kp] - xi[kp] * eta[k])
            gx.append(eta[kp] - eta[km])
            gy.append(xi[km] - xi[kp])
    return e, nn, xi, eta, gx, gy, A2


def cell_gradient(c, poly, U):
    """The four outputs of one cell: U [n, L, 3] are its vertices' velocities; four float64 vectors [L]."""
    U = np.asarray(U, dtype=np.float64)
    n, L = len(poly), U.shape[1]
    nan = np.full(L, np.nan)
    if n < 3:
        return nan, nan.copy(), nan.copy(), nan.copy()
    e, nn, _, _, gx, gy, A2 = geometry(c, poly)
    if A2 == 0.0 or not np.isfinite(A2):
        return nan, nan.copy(), nan.copy(), nan.copy()
    sux, suy, svx, svy = np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L)
    with np.errstate(all="ignore"):
        for k in range(n):
            Ux, Uy, Uz = U[k, :, 0], U[k, :, 1], U[k, :, 2]
            u = (Ux * e[0] + Uy * e[1]) + Uz * e[2]
            v = (Ux * nn[0] + Uy * nn[1]) + Uz * nn[2]
            sux = sux + u * gx[k]
            suy = suy + u * gy[k]
            svx = svx + v * gx[k]
            svy = svy + v * gy[k]
        ux, uy, vx, vy = sux / A2, suy / A2, svx / A2, svy / A2
        vorticity = vx - uy
        divergence = ux + vy
        sn = ux - vy
        ss = vx + uy
        s2 = sn * sn + ss * ss
        strain = np.sqrt(s2)
        okubo_weiss = s2 - vorticity * vorticity
    return vorticity, divergence, strain, okubo_weiss


def mesh_tables(mesh):
    """(cellCoord [C, 3], vertexCoord [V, 3], nEdgesOnCell [C], verticesOnCell [C, maxEdges] 0-based)."""
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    vc = np.asarray(mesh.vertexCoord, dtype=np.float64).reshape(-1, 3)
    nv = np.asarray(mesh.nEdgesOnCell).astype(np.int64).reshape(-1)
    voc = np.asarray(mesh.verticesOnCell).astype(np.int64).reshape(len(cc), -1) - 1
    return cc, vc, nv, voc


def velocity_gradient(mesh, vertex_vel, reverse=False):
    """mops_velocity_gradient: ``vertex_vel`` is cellVertexVelocity [V * L * 3] (DeviceField.export()'s);
    returns {name: [C, L]}.  ``reverse`` walks every cell's vertices in the opposite order."""
    cc, vc, nv, voc = mesh_tables(mesh)
    U = np.asarray(vertex_vel, dtype=np.float64).reshape(len(vc), -1, 3)
    L = U.shape[1]
    out = {k: np.empty((len(cc), L)) for k in NAMES}
    for c in range(len(cc)):
        ids = voc[c, :nv[c]]
        if reverse:
            ids = ids[::-1]
        res = cell_gradient(cc[c], vc[ids], U[ids])
        for k, r in zip(NAMES, res):
            out[k][c] = r
    return out


def cell_to_vertex_signed(mesh, cell_attr):
    """mops_cell_to_vertex_signed: [C * L] -> [V, L], the barycentric weights of the three cellsOnVertex centres
    (CalcCellCenterToVertex's expressions, MPASOSolutionTBB.cpp:57-106), no clamp; a vertex with a missing cell
    (quirk Q10: the 1-based entry is 0 or above nCells + 2) gets 0."""
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    vc = np.asarray(mesh.vertexCoord, dtype=np.float64).reshape(-1, 3)
    C, V = len(cc), len(vc)
    a = np.asarray(cell_attr, dtype=np.float64).reshape(C, -1)
    cov = np.asarray(mesh.cellsOnVertex).astype(np.int64).reshape(V, 3)
    out = np.zeros((V, a.shape[1]))
    with np.errstate(all="ignore"):
        for v in range(V):
            x = cov[v]
            if any(t == 0 or t - 1 > C + 1 for t in x):
                continue
            c0, c1, c2 = (int(t) - 1 for t in x)
            p, A, B, Cc = vc[v], cc[c0], cc[c1], cc[c2]
            v0 = [F(B[d]) - F(A[d]) for d in range(3)]
            v1 = [F(Cc[d]) - F(A[d]) for d in range(3)]
            v2 = [F(p[d]) - F(A[d]) for d in range(3)]
            d00 = v0[0] * v0[0] + v0[1] * v0[1] + v0[2] * v0[2]
            d01 = v0[0] * v1[0] + v0[1] * v1[1] + v0[2] * v1[2]
            d11 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]
            d20 = v2[0] * v0[0] + v2[1] * v0[1] + v2[2] * v0[2]
            d21 = v2[0] * v1[0] + v2[1] * v1[1] + v2[2] * v1[2]
            den = d00 * d11 - d01 * d01
            bv = (d11 * d20 - d01 * d21) / den
            bw = (d00 * d21 - d01 * d20) / den
            bu = F(1.0) - bv - bw
            out[v] = bu * a[c0] + bv * a[c1] + bw * a[c2]
    return out
