#!/usr/bin/env python3
"""In-frame time of K6 (rfx_motion_blur) at 4K: samples 16 and 32 over three velocity fields, timed with rfx_profile (per-draw events
inside a loop of draws, as bench.py times the other kernels).  Not part of bench.py.

    python tools/time_motion_blur.py [--out profiles/motion_blur/timings.json] [--iters 50]

Fields: a uniform pan of ~8 px and of ~64 px at 60 fps (uv velocity * frameSpeed * width), and per-object random motion (64 x 64 blocks,
each with its own velocity up to ~48 px, 30 % of them static).  The counters come from a separate run of this script under
`rocprofv3 --pmc ...` (tools/collect_profiles.sh style), never combined with tracing.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))

from rfx_amd import abi  # noqa: E402
from rfx_amd.context import Context  # noqa: E402

W, H = 3840, 2160
DT = 1 / 60
FRAME_SPEED = 0.01 / DT  # uv per velocity unit


def field(kind, rng):
    v = np.zeros((H, W, 4), np.float32)
    if kind == "pan8":
        v[..., 0] = 8.0 / W / FRAME_SPEED
    elif kind == "pan64":
        v[..., 0] = 64.0 / W / FRAME_SPEED
    else:  # per-object
        by, bx = (H + 63) // 64, (W + 63) // 64
        blk = rng.uniform(-48, 48, (by, bx, 2)).astype(np.float32) / np.float32(W) / np.float32(FRAME_SPEED)
        blk[rng.random((by, bx)) < 0.3] = 0
        v[..., :2] = np.repeat(np.repeat(blk, 64, 0), 64, 1)[:H, :W]
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/motion_blur/timings.json for the full table; nothing is written for --only unless given")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default=None, help="one case, e.g. pan8:16 (for a counter run)")
    a = ap.parse_args()
    rng = np.random.default_rng(4096)
    ctx = Context(W, H)
    ctx.upload(abi.TEX_EFFECT_INPUT, rng.uniform(0, 3, (H, W, 4)).astype(np.float32))
    rows = []
    for kind in ("pan8", "pan64", "objects"):
        ctx.upload(abi.TEX_VELOCITY, field(kind, rng))
        for samples in (16, 32):
            if a.only and a.only != "%s:%d" % (kind, samples):
                continue
            p = abi.MotionBlurParams()
            p.source, p.center, p.samples, p.intensity, p.jitter, p.deltaTime, p.frame = abi.TEX_EFFECT_INPUT, -1, samples, 1.0, 1.0, DT, 1
            p.resolution[:] = [W, H]
            for _ in range(5):
                ctx.motion_blur(p)
            ctx.sync()
            ctx.profile(True)
            for _ in range(a.iters):
                ctx.motion_blur(p)
            prof = ctx.profile_read()["k6_motion_blur"]
            ctx.profile(False)
            ms = prof[0] / prof[1]
            rows.append(dict(field=kind, samples=samples, ms=round(ms, 4), mpix_per_s=round(W * H / ms / 1e3, 1), launches=prof[1]))
            print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    out = a.out or (None if a.only else os.path.join(ROOT, "profiles", "motion_blur", "timings.json"))
    if out is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(width=W, height=H, deltaTime=DT, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
