"""CPU: the host side of the capture path (mops_traj_capture_plan / mops_traj_capture_bytes and the argument
checks of mops_traj_advance_captured that need no device) against a brute-force enumeration of the sample
steps (include/mops_traj.h: step 0, and every step j with (j + 1) % ri == 0 whose slot is below K)."""
import ctypes as C

import pytest

DELTA_T = 60


def _cfg(ri, K):
    from mops_amd import _lib
    return _lib.TrajCfg(DELTA_T, DELTA_T * ri * K, DELTA_T * ri, 0, 1)


def _sample_steps(ri, K):
    n_steps = ri * K
    return [j for j in range(n_steps) if j == 0 or ((j + 1) % ri == 0 and (j + 1) // ri - 1 < K)]


def _plan(lib, cfg, sb, se, W):
    n = lib.mops_traj_capture_plan(C.byref(cfg), sb, se, W, None, 0)
    assert n >= 0
    out = (C.c_int64 * max(n, 1))()
    assert lib.mops_traj_capture_plan(C.byref(cfg), sb, se, W, out, n) == n
    return [int(out[i]) for i in range(n)]


def _ranges(ri, K):
    n = ri * K
    on = 2 * ri - 1  # a sample step past step 0
    cand = {(0, n), (0, on), (on, n), (on, on + 1), (0, on + 1), (1, n - 1), (on + 1, n), (ri, 4 * ri + 1),
            (on, 5 * ri - 1), (n - 1, n), (3, 3), (0, 1)}
    return sorted((a, b) for a, b in cand if 0 <= a <= b <= n)


@pytest.mark.parametrize("K", [6, 12])
@pytest.mark.parametrize("ri", [1, 3, 30])
def test_plan_against_brute_force(engine_lib, ri, K):
    cfg = _cfg(ri, K)
    samples = _sample_steps(ri, K)
    for sb, se in _ranges(ri, K):
        in_range = [j for j in samples if sb <= j < se]
        split = _plan(engine_lib, cfg, sb, se, 0)
        # W = 0: a boundary at every sample step after the first step, then the end (mops_traj_advance_sampled)
        want_split = [j for j in in_range if j > sb] + ([se] if se > sb else [])
        assert split == want_split, (sb, se)
        for W in (0, 1, 2, 5, K):
            ends = _plan(engine_lib, cfg, sb, se, W)
            if sb == se:
                assert ends == []
                continue
            assert ends[-1] == se and all(a < b for a, b in zip([sb] + ends, ends)), (sb, se, W, ends)
            starts = [sb] + ends[:-1]
            for j in in_range:
                first = sum(1 for s in starts if s == j)
                interior = sum(1 for s, e in zip(starts, ends) if s < j < e)
                assert first + interior == 1, (sb, se, W, j, ends)
            for s, e in zip(starts, ends):
                inside = [j for j in in_range if s < j < e]
                assert len(inside) <= W, (sb, se, W, ends)
                if e != se:  # greedy: a launch ends early only on a sample step, with its window full
                    assert e in in_range and len(inside) == W
            if W >= K:
                assert ends == [se]


def test_plan_clamps_and_counts(engine_lib):
    cfg = _cfg(3, 12)
    assert _plan(engine_lib, cfg, -5, 1000, 12) == [36]
    assert _plan(engine_lib, cfg, 0, 36, 5) == [17, 35, 36]
    out = (C.c_int64 * 2)(-1, -1)  # a short buffer: the count is returned, only `cap` ends are stored
    assert engine_lib.mops_traj_capture_plan(C.byref(cfg), 0, 36, 0, out, 1) == 13 and out[0] == 2 and out[1] == -1


def test_plan_refuses_invalid_settings(engine_lib):
    from mops_amd import _lib
    plan = engine_lib.mops_traj_capture_plan
    good = _cfg(3, 12)
    out = (C.c_int64 * 4)()
    assert plan(None, 0, 36, 1, out, 4) == -1 and engine_lib.mops_last_error().decode()
    assert plan(C.byref(good), 0, 36, -1, out, 4) == -1
    assert plan(C.byref(good), 0, 36, 1, out, -1) == -1
    assert plan(C.byref(good), 0, 36, 1, None, 4) == -1
    for bad in (_lib.TrajCfg(0, 3600, 600, 0, 1), _lib.TrajCfg(60, 3600, 0, 0, 1), _lib.TrajCfg(60, 0, 600, 0, 1),
                _lib.TrajCfg(60, 300, 600, 0, 1)):  # the last: no record fits the run
        assert plan(C.byref(bad), 0, 36, 1, out, 4) == -1


def test_capture_bytes(engine_lib):
    b = engine_lib.mops_traj_capture_bytes
    assert b(96, 12) == 32 * 96 * 12 and b(1, 1) == 32
    assert b(0, 5) == 0 and b(5, 0) == 0
    assert b(-1, 5) == -1 and b(5, -1) == -1
    assert b(2 ** 40, 2 ** 30) == -1  # overflow


def test_advance_captured_null_handles(engine_lib):
    from mops_amd import _lib
    assert hasattr(engine_lib, "mops_traj_advance_captured")
    cfg = _cfg(3, 12)
    st = engine_lib.mops_traj_advance_captured(None, None, None, C.byref(cfg), None, 0, 36, None, 0, 2, None, None, None,
                                               0, None, 4, None)
    assert st == _lib.MOPS_ERR_INVALID and engine_lib.mops_last_error().decode()
