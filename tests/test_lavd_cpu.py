"""The LAVD restatement (tests/lavd_reference.py) against independent arithmetic, the agreement of header, ctypes
stubs and exports on the three new entries, and the refusals of the C entries, of the engine layer and of
PathlineChain.run(integrals=...), none of which needs a device."""
import ctypes as C
import math
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lavd_reference as LR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mops_level_mean": 7, "mops_path_integral_abs": 10, "mops_path_integral_image": 6}


def _case(C_=300, L_=5, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((C_, L_)) * 1e-5, rng.uniform(0.5, 2.0, C_) * 1e9


def test_mean_agrees_with_fsum():
    x, w = _case()
    x[:, 0] = np.abs(x[:, 0]) + 1e-6   # one level without cancellation, the others signed
    mean, wsum = LR.level_mean(x, w)
    for l in range(x.shape[1]):
        # (the products are rounded once in both; fsum then adds them without error)
        num = math.fsum(float(a) * float(b) for a, b in zip(w, x[:, l]))
        den = math.fsum(float(b) for b in w)
        scale = math.fsum(abs(float(a) * float(b)) for a, b in zip(w, x[:, l])) / den
        # 300 terms: the sums' error is below 300 * 2^-53 = 3.4e-14 of the terms' size -- of the mean itself
        # where nothing cancels (level 0), of the mean absolute term on the signed levels
        assert abs(mean[l] - num / den) <= 1e-12 * (abs(num / den) if l == 0 else scale), l
        assert wsum[l] == pytest.approx(den, rel=1e-12)
    # the group size is part of the order: another grouping rounds differently somewhere, the same value loosely
    other, _ = LR.level_mean(x, w, group=7)
    assert np.allclose(other, mean, rtol=1e-9, atol=0.0)
    one, _ = LR.level_mean(x[:64], w[:64], group=64)
    seq = np.zeros(x.shape[1]); den = 0.0
    for c in range(64):
        seq = seq + (w[c] * x[c]); den = den + w[c]
    assert (seq / den).tobytes() == one.tobytes()           # one group: the plain ascending sum


def test_zero_weights_exclude_cells_and_nan_levels():
    x, w = _case()
    keep = np.arange(len(w)) % 3 == 0
    masked = np.where(keep, w, 0.0)
    mean, wsum = LR.level_mean(x, masked)
    for l in range(x.shape[1]):
        assert mean[l] == pytest.approx(np.sum(w[keep] * x[keep, l]) / np.sum(w[keep]), rel=1e-10)
    assert np.allclose(wsum, w[keep].sum(), rtol=1e-12)
    # negative, NaN and infinite weights and NaN values do not count either
    w2 = w.copy(); w2[1] = -1.0; w2[2] = np.nan; w2[3] = np.inf
    x2 = x.copy(); x2[4, 0] = np.nan; x2[5, 1] = np.inf
    m2, s2 = LR.level_mean(x2, w2)
    cnt = np.ones_like(x, dtype=bool); cnt[[1, 2, 3]] = False; cnt[4, 0] = False; cnt[5, 1] = False
    for l in range(x.shape[1]):
        assert s2[l] == pytest.approx(w[cnt[:, l]].sum(), rel=1e-12)
        assert np.isfinite(m2[l])
    # an all-NaN level: NaN mean, wsum 0; the other levels untouched
    x3 = x.copy(); x3[:, 2] = np.nan
    m3, s3 = LR.level_mean(x3, w)
    assert np.isnan(m3[2]) and s3[2] == 0.0
    m0, _ = LR.level_mean(x, w)
    assert np.array_equal(np.delete(m3, 2), np.delete(m0, 2))
    assert LR.same(LR.deviation(x3, m3)[:, 2], np.full(len(w), np.nan))


def test_path_integral_of_a_constant_power_of_two_is_exact():
    K, n, v, w = 7, 5, 2.0 ** -17, 3600.0
    vals = np.full((K, n), -v)
    s = LR.path_integral(vals, w)
    assert np.all(s == K * v * w)
    # it starts from the accumulator: two pieces equal the whole
    rng = np.random.default_rng(1)
    vals = rng.standard_normal((K, n))
    whole = LR.path_integral(vals, w, start=np.arange(n, dtype=float))
    parts = LR.path_integral(vals[3:], w, start=LR.path_integral(vals[:3], w, start=np.arange(n, dtype=float)))
    assert whole.tobytes() == parts.tobytes()
    vals[2, 1] = np.nan
    assert np.isnan(LR.path_integral(vals, w)[1]) and np.isfinite(LR.path_integral(vals, w)[0])
    img = LR.image([1.0, 2.0, np.inf, 4.0], [-1, 3, -1, -1], 2.0)
    assert LR.same(img, [[1.0, 0.5, 0.0, 1.0], [np.nan] * 3 + [1.0], [np.nan] * 3 + [1.0], [4.0, 2.0, 0.0, 1.0]])


def test_header_stubs_and_exports_agree(engine_lib):
    from mops_amd import _lib
    text = open(os.path.join(ROOT, "include", "mops_traj.h")).read()
    assert "path integrals and LAVD" in text
    assert re.search(r"#define\s+MOPS_MEAN_GROUP\s+64\b", text) and _lib.MOPS_MEAN_GROUP == LR.GROUP == 64
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in ENTRIES.items():
        assert name in _lib.EXPORTED and hasattr(engine_lib, name), name
        m = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        stub = getattr(engine_lib, name).argtypes
        assert len(params) == len(stub) == n_args, name
        for p, t in zip(params, stub):
            if "*" in p:
                assert t is C.c_void_p, (name, p)
            elif p.startswith("int32_t"):
                assert t is C.c_int32, (name, p)
            elif p.startswith("int64_t"):
                assert t is C.c_int64, (name, p)
            elif p.startswith("double"):
                assert t is C.c_double, (name, p)
            else:
                raise AssertionError((name, p))
    assert engine_lib.mops_abi_version() == 4  # names were added, no struct changed


def test_c_entry_refusals_need_no_device(engine_lib):
    from mops_amd import _lib
    fake = C.c_void_p(0x1000)   # never dereferenced
    nan, inf = float("nan"), float("inf")
    calls = [
        ("mops_level_mean", (4, 2, None, fake, fake, fake, None)),
        ("mops_level_mean", (4, 2, fake, None, fake, fake, None)),
        ("mops_level_mean", (4, 2, fake, fake, None, fake, None)),
        ("mops_level_mean", (4, 2, fake, fake, fake, None, None)),
        ("mops_level_mean", (0, 2, fake, fake, fake, fake, None)),
        ("mops_level_mean", (-3, 2, fake, fake, fake, fake, None)),
        ("mops_level_mean", (4, 0, fake, fake, fake, fake, None)),
        ("mops_path_integral_abs", (4, 0, 2, None, 4, 1, None, 1.0, fake, None)),
        ("mops_path_integral_abs", (4, 0, 2, fake, 4, 1, None, 1.0, None, None)),
        ("mops_path_integral_abs", (0, 0, 2, fake, 4, 1, None, 1.0, fake, None)),
        ("mops_path_integral_abs", (4, -1, 2, fake, 4, 1, None, 1.0, fake, None)),
        ("mops_path_integral_abs", (4, 3, 2, fake, 4, 1, None, 1.0, fake, None)),
        ("mops_path_integral_abs", (4, 0, 2, fake, 4, 1, None, nan, fake, None)),
        ("mops_path_integral_abs", (4, 0, 2, fake, 4, 1, None, inf, fake, None)),
        ("mops_path_integral_abs", (4, 0, 2, fake, 4, 1, None, -1.0, fake, None)),
        ("mops_path_integral_abs", (4, 2, 2, fake, 4, 1, None, -1.0, fake, None)),   # (checked before the empty range)
        ("mops_path_integral_image", (4, None, None, 1.0, fake, None)),
        ("mops_path_integral_image", (4, fake, None, 1.0, None, None)),
        ("mops_path_integral_image", (0, fake, None, 1.0, fake, None)),
        ("mops_path_integral_image", (4, fake, fake, 0.0, fake, None)),
        ("mops_path_integral_image", (4, fake, fake, -2.0, fake, None)),
        ("mops_path_integral_image", (4, fake, fake, nan, fake, None)),
        ("mops_path_integral_image", (4, fake, fake, inf, fake, None)),
    ]
    for name, args in calls:
        assert getattr(engine_lib, name)(*args) == _lib.MOPS_ERR_INVALID, (name, args)
        assert name.encode() in engine_lib.mops_last_error()
    # an empty range succeeds and touches nothing: the pointers are the stand-ins
    assert engine_lib.mops_path_integral_abs(4, 2, 2, fake, 4, 1, None, 1.0, fake, None) == _lib.MOPS_OK
    assert engine_lib.mops_path_integral_abs(4, 0, 0, fake, 4, 1, fake, 0.0, fake, None) == _lib.MOPS_OK


def test_engine_refusals_come_before_any_launch():
    import torch
    from mops_amd import engine
    with pytest.raises(ValueError, match="level_mean"):
        engine.level_mean(torch.zeros(4, 2, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))  # not on the device
    with pytest.raises(ValueError, match="level_mean"):
        engine.level_mean(np.zeros((4, 2)), np.zeros(4))
    with pytest.raises(ValueError, match="PathIntegral"):
        engine.PathIntegral(0)
    for w in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="weight"):
            engine.PathIntegral._weight(w)
    assert engine.PathIntegral._weight(3600) == 3600.0
    lat = types.SimpleNamespace(n=8, torch=torch)
    for h in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="horizon"):
            engine.FlowMapLattice.lavd(lat, None, horizon=h)


def test_chain_integrals_need_attrs_before_any_launch():
    """run(integrals=...) without attrs, with a name the chain does not sample, or with something that is no
    PathIntegral raises before a field is built: make_field here would fail the test."""
    from mops_amd import chain, engine

    def make_field(i, stream):
        raise AssertionError("a field was built")
    integral = object.__new__(engine.PathIntegral)   # (no device: never used)
    integral.n = 5
    mesh = types.SimpleNamespace(nVertLevels=3)
    c = chain.PathlineChain(mesh, make_field, 3, gap_seconds=3600)
    seeds = np.zeros((5, 3))
    with pytest.raises(ValueError, match="integrals.*attrs=True"):
        c.run(seeds, depth=10.0, integrals={"vorticity_deviation": integral})
    with pytest.raises(ValueError, match="integrals"):
        c.run(seeds, depth=10.0, attrs=True, integrals={"vorticity_deviation": 3.0})
    with pytest.raises(ValueError, match="integrals"):
        c.run(seeds, depth=10.0, attrs=True, integrals=[integral])

    def make_attrs(i, stream, field=None):
        raise AssertionError("attributes were built")
    make_attrs.names = ["salinity"]
    make_attrs.wants_field = True
    c = chain.PathlineChain(mesh, make_field, 3, gap_seconds=3600, make_attrs=make_attrs)
    with pytest.raises(ValueError, match="samples no attribute 'vorticity_deviation'"):
        c.run(seeds, depth=10.0, attrs=True, integrals={"vorticity_deviation": integral})
    # the factories carry what the chain looks for
    f = chain.vorticity_deviation_factory(mesh)
    assert f.wants_field is True and f.names == ["vorticity_deviation"] and f.seen == [] and f.means == {}
    assert chain.vorticity_deviation_factory(mesh, name="lavd").names == ["lavd"]
    with pytest.raises(ValueError, match="field"):
        f(0, 0)
