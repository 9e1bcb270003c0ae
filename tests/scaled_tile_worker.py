"""One tile of a row-tiled SSGIEffect run at resolutionScale < 1 with the exchanges behind the C ABI (test_resolution_scale_tiled_hostsim.py:
one process per tile on the host simulator's library; world 1 is the reference run).  No torch here: a torch process maps the real
librccl.so.1, which rfx_comm.hip would rightly reuse."""
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "realism-effects_amd"))

from rfx_amd import abi, tiling  # noqa: E402
from rfx_amd.context import Context  # noqa: E402
from rfx_amd.effect import SSGIEffect  # noqa: E402
from rfx_amd.scene import synthetic_frame  # noqa: E402

rank, world, outdir, W, H, FRAMES = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
MODE, SCALE = sys.argv[7], float(sys.argv[8])  # CommTiledRenderer history_gather; SSGIEffect resolutionScale
frames = [synthetic_frame(W, H, i) for i in range(FRAMES)]
vmax = max(float(np.abs(f.velocity[..., 1].view(np.float32)).max()) for f in frames)
y0, rows = tiling.split_rows(H, world)[rank]
ctx = Context(W, H, tile_y0=y0, tile_rows=rows, halo_rows=tiling.required_halo(3.0, vmax, H, W, resolution_scale=SCALE) if world > 1 else 0)
idf = os.path.join(outdir, "nccl_id")
if rank == 0:
    with open(idf + ".tmp", "wb") as f:
        f.write(Context.comm_unique_id())
    os.rename(idf + ".tmp", idf)
deadline = time.monotonic() + 60
while not os.path.exists(idf):
    if time.monotonic() > deadline:
        sys.exit("rank %d: rank 0 never wrote the communicator id" % rank)
    time.sleep(0.01)
with open(idf, "rb") as f:
    uid = f.read()
r = tiling.CommTiledRenderer(ctx, rank, world, uid, history_gather=MODE)
scene, cam = types.SimpleNamespace(frame=None), frames[0].camera
fx = SSGIEffect(None, scene, cam, dict(width=W, height=H, denoiseIterations=1, steps=12, refineSteps=3, resolutionScale=SCALE), seeds=dict(ssgi=5, denoise=9))
for f in frames:
    scene.frame = f
    for k, v in vars(f.camera).items():
        setattr(cam, k, v)
    fx.update(r, None)
r.finish_pending()
r.finish_halo()
if world > 1:
    assert r.history_gather == MODE and (MODE != "bounded" or len(r.history_bytes_received) == FRAMES)
j0, target = ctx.download_ssgi_target(SCALE)
np.savez(os.path.join(outdir, "s%d.npz" % rank), y0=y0, rows=rows, j0=j0, target=target, halo_violations=ctx.halo_violations(),
         history_bytes=np.array(r.history_bytes_received, np.int64),
         **{abi.TEX_NAMES[t]: ctx.download(t, y0, rows) for t in (abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1, abi.TEX_DENOISE_B0, abi.TEX_DENOISE_B1, abi.TEX_COMPOSE)})
ctx.comm_destroy()
ctx.close()
assert "torch" not in sys.modules
