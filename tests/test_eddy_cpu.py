"""The velocity-gradient operator's restatement (tests/eddy_reference.py) against what the operator must give
analytically -- a solid-body rotation, a uniform field, a reversed polygon, the Okubo-Weiss identity -- its
cell-to-vertex interpolation against the oracle's where the clamp is idle, and the argument refusals of the two
C entries, which need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eddy_reference as ER  # noqa: E402

EPS = float(np.finfo(np.float64).eps)
OMEGA = 1.0e-5   # rad/s
AXES = {"z": (0.0, 0.0, 1.0), "tilted": (0.48, -0.36, 0.8)}   # unit vectors


@pytest.fixture(scope="module")
def tables(small_case):
    mesh = small_case[0]
    return (mesh,) + ER.mesh_tables(mesh)


def _cell_scales(cc, vc, nv, voc, c):
    """(geometry, max |rho_k|, projected perimeter P, largest |p_k|) of cell c."""
    ids = voc[c, :nv[c]]
    poly = vc[ids]
    g = ER.geometry(cc[c], poly)
    rhat = cc[c] / np.linalg.norm(cc[c])
    rho = np.abs((poly - cc[c]) @ rhat).max()
    xi, eta = np.array(g[2]), np.array(g[3])
    P = float(np.hypot(np.roll(xi, -1) - xi, np.roll(eta, -1) - eta).sum())
    return g, float(rho), P, float(np.linalg.norm(poly, axis=1).max())


@pytest.mark.parametrize("axis", sorted(AXES))
def test_solid_body_rotation(tables, axis):
    """U = Omega x p at every vertex, boundary vertices included.  The part of U that is linear in the plane
    coordinates has the gradient of a solid-body rotation exactly (vorticity 2 Omega . r_hat, no divergence, no
    strain), because the Green-Gauss sum is exact for a linear field; the out-of-plane offsets rho_k = d_k . r_hat
    add to u_k and v_k at most |Omega| max|rho_k|, which the sum turns into at most |Omega| max|rho_k| P / |A2 / 2|
    per derivative (sum_k |gx_k| <= 2 P).  Rounding slack per derivative: n + 8 operations' worth of eps on terms of
    size |Omega| |p| |g_k|."""
    mesh, cc, vc, nv, voc = tables
    om = OMEGA * np.array(AXES[axis])
    U = np.cross(om, vc)                       # [V, 3]
    L = 2
    vel = np.repeat(U[:, None, :], L, axis=1).reshape(-1)
    out = ER.velocity_gradient(mesh, vel)
    want = np.empty(len(cc)); bound = np.empty(len(cc)); slack = np.empty(len(cc))
    for c in range(len(cc)):
        g, rho, P, pmax = _cell_scales(cc, vc, nv, voc, c)
        half_area = abs(float(g[6])) / 2.0
        want[c] = 2.0 * float(om @ (cc[c] / np.linalg.norm(cc[c])))
        bound[c] = OMEGA * rho * P / half_area
        slack[c] = (nv[c] + 8) * EPS * OMEGA * pmax * P / half_area
    for name in ER.NAMES:
        assert np.isfinite(out[name]).all(), name
        assert np.array_equal(out[name][:, 0], out[name][:, 1]), name     # the levels hold the same velocities
    tol = 2.0 * bound + 2.0 * slack
    vort, dvg, strain = out["vorticity"][:, 0], out["divergence"][:, 0], out["strain"][:, 0]
    print(f"{axis}: max |vorticity error| / tol {np.max(np.abs(vort - want) / tol):.3g}, "
          f"|divergence| / tol {np.max(np.abs(dvg) / tol):.3g}, strain / tol {np.max(strain / tol):.3g}, "
          f"max bound / |2 Omega| {bound.max() / (2 * OMEGA):.3g}")
    assert np.all(np.abs(vort - want) <= tol)
    assert np.all(np.abs(dvg) <= tol)
    assert np.all(strain <= tol)
    # the sign: wherever the bound is under a quarter of |2 Omega . r_hat|
    sure = bound < 0.25 * np.abs(want)
    assert sure.sum() >= len(cc) / 2
    assert (want[sure] > 0).any() and (want[sure] < 0).any()       # both hemispheres of the rotation
    assert np.array_equal(np.sign(vort[sure]), np.sign(want[sure]))
    lat = np.degrees(np.arcsin(np.abs(want) / (2 * OMEGA)))
    print(f"{axis}: {int(sure.sum())} of {len(cc)} cells qualify; the unsure ones lie within "
          f"{lat[~sure].max() if (~sure).any() else 0.0:.2f} degrees of the rotation's equator")


def _velocities(tables, seed=7, L=3):
    mesh, cc, vc, nv, voc = tables
    rng = np.random.default_rng(seed)
    return rng.normal(scale=0.3, size=(len(vc), L, 3))


def _term_scale(cc, vc, nv, voc, U, c):
    """sum_k (|u_k| + |v_k|) (|gx_k| + |gy_k|) / |A2| per level: the size of a derivative's terms."""
    ids = voc[c, :nv[c]]
    e, nn, _, _, gx, gy, A2 = ER.geometry(cc[c], vc[ids])
    u = np.abs(U[ids] @ np.array(e, dtype=float)) + np.abs(U[ids] @ np.array(nn, dtype=float))   # [n, L]
    g = np.abs(np.array(gx, dtype=float)) + np.abs(np.array(gy, dtype=float))
    return (u * g[:, None]).sum(0) / abs(float(A2))


def test_reversed_vertex_order_gives_the_same_outputs(tables):
    """Reversing a cell's vertices negates gx, gy and A2: the quotients are the same sums in another order.  Two
    sums of n terms differ by at most 2 n eps of their terms' sizes, A2's terms are of one sign (the cells are
    star-shaped about their centres) so its own relative error is n eps in each order; with the four
    operations behind each term: (4 n + 8) eps S for the first-order outputs, S the size of a derivative's
    terms, and twice that times 2 S for the Okubo-Weiss parameter, which is quadratic."""
    mesh, cc, vc, nv, voc = tables
    U = _velocities(tables)
    a = ER.velocity_gradient(mesh, U.reshape(-1))
    b = ER.velocity_gradient(mesh, U.reshape(-1), reverse=True)
    worst = 0.0
    for c in range(len(cc)):
        S = _term_scale(cc, vc, nv, voc, U, c)
        tol = (4 * nv[c] + 8) * EPS * S
        for name in ("vorticity", "divergence", "strain"):
            d = np.abs(a[name][c] - b[name][c])
            worst = max(worst, float((d / tol).max()))
            assert np.all(d <= tol), (c, name)
        assert np.all(np.abs(a["okubo_weiss"][c] - b["okubo_weiss"][c]) <= 2 * tol * 2 * S), c
    print(f"reversed order: worst difference / tolerance {worst:.3g}")


def test_uniform_tangent_plane_field_has_no_gradient(tables):
    """U_k = a e + b nn at every vertex of a cell: sum_k gx_k and sum_k gy_k are zero but for rounding, (n + 8)
    eps of the terms' sizes."""
    mesh, cc, vc, nv, voc = tables
    a, b = 0.7, -0.4
    worst = 0.0
    for c in range(0, len(cc), 7):
        ids = voc[c, :nv[c]]
        e, nn = ER.frame(cc[c])
        Uc = a * np.array(e, dtype=float) + b * np.array(nn, dtype=float)
        U = np.repeat(Uc[None, None, :], len(ids), axis=0)        # [n, 1, 3]
        _, _, _, _, gx, gy, A2 = ER.geometry(cc[c], vc[ids])
        g = (np.abs(np.array(gx, dtype=float)) + np.abs(np.array(gy, dtype=float))).sum() / abs(float(A2))
        tol = 2 * (nv[c] + 8) * EPS * (abs(a) + abs(b)) * g
        vort, dvg, strain, ow = ER.cell_gradient(cc[c], vc[ids], U)
        for x in (vort, dvg, strain):
            worst = max(worst, float(abs(x[0]) / tol))
            assert abs(x[0]) <= 2 * tol, c      # strain: sqrt(sn^2 + ss^2) <= sqrt(2) of a first-order output
        assert abs(ow[0]) <= 8 * tol * tol, c
    print(f"uniform field: worst |output| / tolerance {worst:.3g}")


def test_okubo_weiss_is_strain_squared_minus_vorticity_squared(tables):
    mesh = tables[0]
    out = ER.velocity_gradient(mesh, _velocities(tables, seed=11).reshape(-1))
    s, w, ow = out["strain"], out["vorticity"], out["okubo_weiss"]
    assert np.isfinite(ow).all() and (ow > 0).any() and (ow < 0).any()
    # sqrt then square returns s2 within 2 eps of it; the subtraction adds one more of the larger operand
    assert np.all(np.abs(ow - (s * s - w * w)) <= 4 * EPS * (s * s + w * w))


def test_invalid_cells_are_nan():
    """n < 3, a zero area and a non-finite area give NaN at every level; NaN in, NaN out otherwise."""
    c = np.array([6.0e6, 1.0e6, 2.0e6])
    sq = c + np.array([[1e4, 0, 0], [0, 1e4, 0], [-1e4, 0, 0], [0, -1e4, 0]], dtype=float)
    U = np.ones((4, 2, 3))
    assert all(np.isfinite(x).all() for x in ER.cell_gradient(c, sq, U))
    assert all(np.isnan(x).all() for x in ER.cell_gradient(c, sq[:2], U[:2]))
    flat = np.repeat(sq[:1], 4, axis=0)
    assert all(np.isnan(x).all() for x in ER.cell_gradient(c, flat, U))                 # A2 == 0
    far = sq.copy(); far[1, 0] = np.inf
    assert all(np.isnan(x).all() for x in ER.cell_gradient(c, far, U))                  # A2 not finite
    Un = U.copy(); Un[2, 1, 0] = np.nan
    res = ER.cell_gradient(c, sq, Un)
    assert all(np.isfinite(x[0]) and np.isnan(x[1]) for x in res)
    # a centre on the axis takes the fixed frame
    assert ER.frame((0.0, 0.0, 5.0)) == ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    assert ER.frame((0.0, 0.0, -5.0)) == ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0))


def test_signed_interpolation_is_the_oracles_where_the_clamp_is_idle(oracle_lib, small_case):
    """On a non-negative array the clamp never acts: the restatement equals the oracle's CalcCellCenterToVertex
    (the arrays of preprocess) bit for bit; on a signed one it keeps negative values and boundary zeros."""
    mesh, s0, _ = small_case
    derived = oracle_lib.preprocess(mesh, s0)
    name = sorted(s0.attributes)[0]
    cell = np.asarray(s0.attributes[name], dtype=np.float64)
    assert (cell >= 0).all()
    got = ER.cell_to_vertex_signed(mesh, cell)
    assert got.reshape(-1).tobytes() == derived.attrs[name].tobytes()
    signed = ER.cell_to_vertex_signed(mesh, cell - cell.mean())
    assert (signed < 0).any() and (signed > 0).any()
    cov = np.asarray(mesh.cellsOnVertex).reshape(-1, 3)
    boundary = (cov == 0).any(axis=1)
    assert boundary.any() and np.all(signed[boundary] == 0.0)


def test_cli_eddy_option():
    from mops_amd.cli import parse_command_line
    assert parse_command_line(["-i", "x.yaml"]).eddy is False
    a = parse_command_line(["-i", "x.yaml", "--eddy", "--vti"])
    assert a.eddy and a.vti


def test_entry_refusals_need_no_device(engine_lib):
    """The argument checks of both entries come before any device work and touch no output."""
    from mops_amd import _lib, engine
    fake = C.c_void_p(0x1000)   # never dereferenced
    out = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    for mesh, field, outs in ((None, fake, (out, out, out, out)), (fake, None, (out, None, None, None)),
                              (fake, fake, (None, None, None, None))):
        assert engine_lib.mops_velocity_gradient(mesh, field, *outs, None) == _lib.MOPS_ERR_INVALID
        assert b"mops_velocity_gradient" in engine_lib.mops_last_error()
    for mesh, src, dst in ((None, out, out), (fake, None, out), (fake, out, None)):
        assert engine_lib.mops_cell_to_vertex_signed(mesh, src, dst, None) == _lib.MOPS_ERR_INVALID
        assert b"mops_cell_to_vertex_signed" in engine_lib.mops_last_error()
    assert list(out) == [7.0] * 4
    for bad in (("curl",), (), ("vorticity", "Okubo")):
        with pytest.raises(ValueError, match="which"):
            engine.velocity_gradient(None, None, which=bad)
