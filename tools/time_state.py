#!/usr/bin/env python3
"""Size of a checkpoint of the temporal state and wall time of one save and one load (rfx_amd/state.py) — default chain, 3840x2160 unless
--size says otherwise.  Median of --repeats after one warm-up of each; wall clock of the host calls (device sync, downloads, file writes
with fsync, checksums / reads, uploads).  Not part of bench.py; no threshold hangs on it.

    python tools/time_state.py [--size 3840x2160] [--repeats 5] [--dir DIR] [--out profiles/state_resume/timings.json]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))

from rfx_amd import effect, state  # noqa: E402
from rfx_amd.context import Context  # noqa: E402
from rfx_amd.scene import synthetic_frame  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2, help="frames drawn before the first save")
    ap.add_argument("--dir", default=None, help="where the checkpoint goes (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    where = a.dir or tempfile.mkdtemp(prefix="rfx-state-")
    ck = os.path.join(where, "checkpoint")
    ctx = Context(W, H)
    scene = types.SimpleNamespace(frame=None)
    frames = [synthetic_frame(W, H, i) for i in range(a.frames)]
    cam = types.SimpleNamespace(**vars(frames[0].camera))
    fx = effect.SSGIEffect(None, scene, cam, dict(width=W, height=H), seeds=dict(ssgi=11, denoise=22))
    for f in frames:
        scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        fx.update(ctx, None)
    ctx.sync()
    save, load = [], []
    for i in range(a.repeats + 1):  # (the first pair is the warm-up)
        t0 = time.perf_counter()
        header = state.save_state(ck, ctx, [fx])
        t1 = time.perf_counter()
        state.load_state(ck, ctx, [fx])
        t2 = time.perf_counter()
        if i:
            save.append(t1 - t0)
            load.append(t2 - t1)
    size = sum(os.path.getsize(os.path.join(ck, n)) for n in os.listdir(ck))
    ctx.close()
    res = dict(width=W, height=H, planes=[p["slot"] for p in header["planes"]], checkpoint_bytes=size, repeats=a.repeats,
               save_s_median=round(statistics.median(save), 4), save_s=[round(x, 4) for x in save],
               load_s_median=round(statistics.median(load), 4), load_s=[round(x, 4) for x in load])
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not a.dir:
        shutil.rmtree(where, ignore_errors=True)


if __name__ == "__main__":
    main()
