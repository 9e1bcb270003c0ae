#!/usr/bin/env python3
"""How the reference GL (llvmpipe) lowers `mix(startUv, endUv, t)` in motion_blur.frag: the numpy restatement (tests/motion_blur_ref.py)
with candidate lowerings, each against the llvmpipe fixture of option cases (tests/golden/motion_blur_cases_128x72.npz); prints the
bit-identical share per case.  CPU only; reads committed files.

    python tools/probe_motion_blur_gl.py
"""
import inspect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))

import motion_blur_ref as R  # noqa: E402
from rfx_amd.context import load_blue_noise_table  # noqa: E402

MIX = "linear_fetch(source, su + t * du, sv + t * dv)"
VARIANTS = {
    "a + t (b - a), two roundings (the kernel's)": MIX,
    "fma(t, b - a, a)": "linear_fetch(source, fma(t, du, su), fma(t, dv, sv))",
    "a (1 - t) + b t": "linear_fetch(source, (su * (f32(1) - t) + eu * t).astype(f32), (sv * (f32(1) - t) + ev * t).astype(f32))",
    "fma(t, b, a - a t)": "linear_fetch(source, fma(t, eu, su - su * t), fma(t, ev, sv - sv * t))",
}


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "motion_blur_cases_128x72.npz"))
    bn = load_blue_noise_table()
    vel = np.concatenate([g["velocity"], np.zeros(g["velocity"].shape[:2] + (2,), np.float32)], -1)
    src = inspect.getsource(R.motion_blur)
    assert MIX in src
    for name, form in VARIANTS.items():
        ns = dict(R.__dict__)
        exec(src.replace(MIX, form), ns)
        share = []
        for c, ref in zip(g["cases"], g["outputs_rgb"]):
            s, i, j, rx, ry, f, dt = c
            got = ns["motion_blur"](vel, g["source"], blue_noise=bn, samples=int(s), intensity=i, jitter=j, resolution=(rx, ry), frame=int(f),
                                    deltaTime=dt)[..., :3]
            share.append((got == ref).mean())
        print("%-46s %s" % (name, " ".join("%.4f" % x for x in share)))


if __name__ == "__main__":
    main()
