"""Restatement of the path-integral and LAVD entries (include/mops_traj.h, "path integrals and LAVD") in numpy,
expression by expression, with the header's order of every sum.

TEST INFRASTRUCTURE ONLY: the product never imports this module.  numpy float64 scalars and arrays round every
operation on its own (no contraction), so the bytes are the device's.
"""
import numpy as np

F = np.float64
GROUP = 64  # MOPS_MEAN_GROUP


def level_mean(field, weight, group=GROUP):
    """mops_level_mean: (mean [L], wsum [L]).  Explicit ascending loops over the cells of a group and then over
    the groups; vectorised over the levels only (every level runs the same sequence of operations)."""
    field = np.asarray(field, dtype=F)
    weight = np.asarray(weight, dtype=F).reshape(-1)
    C, L = field.shape
    assert weight.shape == (C,)
    num, den = np.zeros(L), np.zeros(L)
    with np.errstate(all="ignore"):
        for c0 in range(0, C, group):
            gnum, gden = np.zeros(L), np.zeros(L)
            for c in range(c0, min(c0 + group, C)):
                w = weight[c]
                if not (np.isfinite(w) and w > 0.0):
                    continue
                x = field[c]
                counts = np.isfinite(x)
                gnum = np.where(counts, gnum + (w * x), gnum)
                gden = np.where(counts, gden + w, gden)
            num = num + gnum
            den = den + gden
        mean = np.where(den == 0.0, np.nan, num / den)
    return mean, den


def deviation(field, mean):
    """field [C, L] - mean[l]: one IEEE subtraction per element."""
    with np.errstate(all="ignore"):
        return np.asarray(field, dtype=F) - np.asarray(mean, dtype=F)[None, :]


def path_integral(values, weight, start=None):
    """mops_path_integral_abs for values [K, n] (slot-major): s = start; for k ascending: s = s + (|v_k| * weight)."""
    values = np.asarray(values, dtype=F)
    s = np.zeros(values.shape[1]) if start is None else np.array(start, dtype=F, copy=True)
    w = F(weight)
    with np.errstate(all="ignore"):
        for k in range(values.shape[0]):
            s = s + (np.abs(values[k]) * w)
    return s


def image(accum, death, horizon):
    """mops_path_integral_image: [n, 4] = {s, s / horizon, 0, 1}; {NaN, NaN, NaN, 1} where death >= 0 or s is not
    finite."""
    s = np.asarray(accum, dtype=F).reshape(-1)
    bad = ~np.isfinite(s)
    if death is not None:
        bad = bad | (np.asarray(death).reshape(-1) >= 0)
    out = np.empty((s.size, 4))
    with np.errstate(all="ignore"):
        out[:, 0] = s
        out[:, 1] = s / F(horizon)
    out[:, 2] = 0.0
    out[bad, :3] = np.nan
    out[:, 3] = 1.0
    return out


def same(a, b):
    """Bit-exact up to the NaN payload: equal shapes, NaNs at equal places, equal bytes elsewhere."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes())
