#!/usr/bin/env python3
"""The row-tiled form of K6 at 4K next to the whole-frame draw (tools/time_motion_blur.py's fields and samples): the reach reduction
(k6_motion_blur_reach, timed with rfx_profile on a whole-frame context next to k6_motion_blur itself), the tiled draw of one 270-row tile
(rank 4 of 8), and the bytes that tile's reach mask names outside its own rows.  Not part of bench.py.

    python tools/time_motion_blur_tiled.py [--out tiled.json] [--iters 50]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rfx_amd import abi  # noqa: E402
from rfx_amd.context import Context  # noqa: E402
from time_motion_blur import DT, H, W, field  # noqa: E402

RANKS, RANK = 8, 4


def timed(ctx, kind, call, iters):
    for _ in range(3):
        call()
    ctx.sync()
    ctx.profile(True)
    for _ in range(iters):
        call()
    ms, n = ctx.profile_read()[kind]
    ctx.profile(False)
    return ms / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    rng = np.random.default_rng(4096)
    src = rng.uniform(0, 3, (H, W, 4)).astype(np.float32)
    y0, rows = Context.split_rows(H, RANKS, RANK)
    whole = Context(W, H)
    tile = Context(W, H, tile_y0=y0, tile_rows=rows, halo_rows=0)
    whole.upload(abi.TEX_EFFECT_INPUT, src)
    tile.upload(abi.TEX_EFFECT_INPUT, src[y0:y0 + rows], y0, rows)
    blocks = (np.arange(W) * 32) // W
    block_texels = np.bincount(blocks, minlength=32)
    out = []
    for kind in ("pan8", "pan64", "objects"):
        vel = field(kind, rng)
        whole.upload(abi.TEX_VELOCITY, vel)
        tile.upload(abi.TEX_VELOCITY, vel[y0:y0 + rows], y0, rows)
        for samples in (16, 32):
            p = abi.MotionBlurParams()
            p.source, p.center, p.samples, p.intensity, p.jitter, p.deltaTime, p.frame = abi.TEX_EFFECT_INPUT, -1, samples, 1.0, 1.0, DT, 1
            p.resolution[:] = [W, H]
            k6 = timed(whole, "k6_motion_blur", lambda: whole.motion_blur(p), a.iters)
            reach = timed(whole, "k6_motion_blur_reach", lambda: whole.motion_blur_reach_mask(p), a.iters)
            ref = whole.download(abi.TEX_MOTION_BLUR, y0, rows)
            tile.motion_blur_stage(p)
            mask = tile.motion_blur_reach_mask(p)
            foreign = mask.copy()
            foreign[y0:y0 + rows] = 0
            texels = int(sum(int(block_texels[[b for b in range(32) if (int(m) >> b) & 1]].sum()) for m in foreign if m))
            named_rows = np.nonzero(foreign)[0]
            for y in named_rows:  # the transport: whole rows here (a superset of the named blocks)
                tile.upload(abi.TEX_BLUR_SOURCE, src[y:y + 1], int(y), 1)
            tiled = timed(tile, "k6_motion_blur", lambda: tile.motion_blur(p), a.iters)
            reach_tile = timed(tile, "k6_motion_blur_reach", lambda: tile.motion_blur_reach_mask(p), a.iters)
            same = tile.download(abi.TEX_MOTION_BLUR, y0, rows).tobytes() == ref.tobytes()
            row = dict(field=kind, samples=samples, k6_ms=round(k6, 4), reach_ms=round(reach, 4), tile_rows=rows, tiled_draw_ms=round(tiled, 4),
                       tile_reach_ms=round(reach_tile, 4), foreign_rows=int(named_rows.size), foreign_bytes=texels * 16,
                       other_tiles_bytes=(H - rows) * W * 16, tile_equals_whole_frame=bool(same))
            out.append(row)
            print(json.dumps(row), flush=True)
    whole.close()
    tile.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(width=W, height=H, deltaTime=DT, ranks=RANKS, rank=RANK, rows=out), f, indent=1)


if __name__ == "__main__":
    main()
