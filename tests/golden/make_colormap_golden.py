"""Writes tests/golden/colormap_reference.npz: channels and the RGBA the reference's own SaveToPNG wrote.

    python tests/golden/make_colormap_golden.py --driver /path/to/driver

The driver is not part of this repository: a small program built once against the reference's
``Common/ImageBuffer.hpp`` (its own SaveToPNG, tinycolormap and stb writer; -ffp-contract=off as its x86-64
build) with this contract:

    driver <inputs.bin> <out_dir>
    inputs.bin : int32 n_cases, then per case int32 width, int32 height, width*height float64 (row-major)
    out_dir    : case_<k>.png = SaveToPNG(image whose channel 0 is the case, "...", 0)

This script writes inputs.bin, runs the driver, decodes its PNGs (tests/image_reference.py: stb compresses
and filters, so the decoder's inflate and filter paths run) and stores, per case ``<name>_in`` [H, W] float64
and ``<name>_rgba`` [H, W, 4] uint8.  The cases:

    normal_nan  37 x 23 standard-normal values, about 10 % NaN
    constant    9 x 5, every value 3.25            (min >= max: max = min + 1e-5f)
    all_nan     9 x 5, every value NaN             (min = FLT_MAX, max = -FLT_MAX; all transparent)
    subfloat    9 x 5, 1 + k * 1e-12               (doubles that differ only below float precision)
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_reference as IR  # noqa: E402


def cases():
    rng = np.random.default_rng(20240607)
    normal = rng.standard_normal((23, 37))
    normal[rng.random((23, 37)) < 0.10] = np.nan
    return {
        "normal_nan": normal,
        "constant": np.full((5, 9), 3.25),
        "all_nan": np.full((5, 9), np.nan),
        "subfloat": 1.0 + np.arange(45, dtype=np.float64).reshape(5, 9) * 1e-12,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--driver", required=True)
    args = ap.parse_args()
    cs = cases()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "inputs.bin"), "wb") as f:
            f.write(struct.pack("<i", len(cs)))
            for a in cs.values():
                f.write(struct.pack("<ii", a.shape[1], a.shape[0]))
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
        subprocess.run([args.driver, os.path.join(d, "inputs.bin"), d], check=True)
        for k, (name, a) in enumerate(cs.items()):
            rgba = IR.decode_png(os.path.join(d, f"case_{k}.png"))
            assert rgba.shape == a.shape + (4,)
            out[name + "_in"] = a
            out[name + "_rgba"] = rgba
    np.savez_compressed(os.path.join(HERE, "colormap_reference.npz"), **out)
    print("wrote colormap_reference.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
