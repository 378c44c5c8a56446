#!/usr/bin/env python3
"""Run bench.py with the given arguments on a -DMOPS_PROF experiment build (MOPS_TRAJ_LIB) and print both
counter arrays with the shares the stay-ball / regroup work is judged by:

    MOPS_TRAJ_LIB=$PWD/build/variants/libmops_prof.so python3 tools/prof_ext.py --no-cpu-baseline --steps 1 --warmup 0

bench.py prints the first array (mops_debug_prof, 16 words) itself, to stderr; this script captures that line
and reads the second array (mops_debug_prof_ext) once the run has ended.  Counts are sums over the whole run."""
import contextlib
import ctypes
import io
import os
import re
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = ("wave-steps running nbr_stay", "regroups that filled a tile", "tile pieces loaded (sum)",
       "groups at those regroups (sum)", "groups holding a lane that did not move (sum)")


def main():
    os.environ["MOPS_PROF_SECTIONS"] = "1"
    sys.path.insert(0, ROOT)
    sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        try:
            runpy.run_path(sys.argv[0], run_name="__main__")
        except SystemExit as e:
            if e.code not in (None, 0):
                sys.stderr = sys.__stderr__
                print(err.getvalue(), file=sys.stderr)
                raise
    from mops_amd import _lib
    lib = _lib.load()
    if not hasattr(lib, "mops_debug_prof_ext"):
        sys.exit("the engine library is not a -DMOPS_PROF build")
    buf = (ctypes.c_uint64 * 8)()
    if lib.mops_debug_prof_ext(buf, 8) != 0:
        sys.exit("mops_debug_prof_ext failed")
    ext = list(buf)[:len(EXT)]
    base = None
    for line in err.getvalue().splitlines():
        if line.startswith("prof counters"):
            base = [int(v) for v in re.findall(r"\d+", line.rsplit("[", 1)[1])]
            print(line)
    print("prof ext counters " + ", ".join(EXT) + ":", ext)
    if base:
        coop_ws = base[6]
        print(f"lane-steps {base[0]:.4e}, walks {base[1]:.4e}, cell loads {base[2]:.4e}, kept by the neighbour table "
              f"{base[13]:.4e}; wave-steps {base[3]:.4e}, cooperative {coop_ws:.4e}")
        if coop_ws:
            print(f"share of cooperative wave-steps running nbr_stay: {ext[0] / coop_ws:.4f}")
            print(f"share of cooperative wave-steps that fill a tile: {ext[1] / coop_ws:.4f}")
    if ext[1]:
        print(f"per tile fill: pieces {ext[2] / ext[1]:.1f}, groups {ext[3] / ext[1]:.2f}, groups with a lane that did "
              f"not move {ext[4] / ext[1]:.2f}")


if __name__ == "__main__":
    main()
