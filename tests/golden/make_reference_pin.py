"""Regenerates tests/golden/reference_pin.npz from the compiled reference (oracle/_ref/mops_ref_driver, built by
__graft_entry__.build_reference() where the reference's sources are present).

The file holds, per case of tests/ref_case.py's golden catalogue (16 trajectory combinations on the small mesh,
two z-level and two heptagon-mesh cases, one with seeds exactly on edge planes, one fixed-latitude and one
fixed-layer image; per wheel mesh of tests/wide_case.py four trajectory modes, a fixed-latitude row and a fixed-layer
window, with one stored line each) and per output array:
the SHA-256 of the array's bytes, its shape and dtype, its first 4 lines (image rows) raw, and the outcome
counts (dead / alive particles, finite / NaN pixels).  Case inputs are regenerated from mops_amd.synth with
fixed seeds and are not stored.  Run:  python tests/golden/make_reference_pin.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__ as g  # noqa: E402
import ref_case as RC  # noqa: E402


def main():
    driver = g.build_reference()
    if driver is None:
        sys.exit("the reference's sources are not present: nothing to record")
    entries = RC.reference_golden(driver)
    np.savez_compressed(RC.GOLDEN, **entries)
    print(f"wrote {RC.GOLDEN}: {len(entries)} entries, {os.path.getsize(RC.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
