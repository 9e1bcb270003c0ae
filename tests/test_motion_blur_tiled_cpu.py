"""CPU (-m "not gpu"): the row-tiled MotionBlurEffect without a device.  ABI 21 in include/rfx.h against rfx_amd/abi.py (compile and print);
the Python and the Node tiled renderers issue the same call sequence for a blurred frame (recording doubles); and
rfx_amd.tiling.TiledRenderer.motion_blur over gloo, on a tile double built on the numpy restatement (tests/motion_blur_ref.py) whose reach
mask is the restatement's own set of loaded texels."""
import json
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

import motion_blur_ref as R
from rfx_amd import abi, effect, tiling
from rfx_amd.context import load_blue_noise_table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")


def test_abi_21_matches_header(tmp_path):
    c = tmp_path / "abi21.c"
    c.write_text('#include <stdio.h>\n#include "rfx.h"\nint main(){printf("%d %d %d %d %d %d %d\\n",RFX_ABI_VERSION,(int)RFX_TEX_MOTION_BLUR,'
                 "(int)RFX_TEX_BLUR_SOURCE,(int)RFX_TEX_COUNT,(int)RFX_PROF_K6,(int)RFX_PROF_K6_REACH,(int)RFX_PROF_COUNT);return 0;}\n")
    exe = tmp_path / "abi21"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    # the three prototypes, as the hosts call them (compiled, not linked)
    proto = tmp_path / "proto.c"
    proto.write_text('#include "rfx.h"\n'
                     "int (*a)(rfx_ctx *, const rfx_motion_blur_params *, unsigned int *, int) = rfx_motion_blur_reach_mask;\n"
                     "int (*b)(rfx_ctx *, const rfx_motion_blur_params *) = rfx_motion_blur_stage;\n"
                     "int (*d)(rfx_ctx *, const rfx_motion_blur_params *, void *, size_t *) = rfx_motion_blur_gather;\n")
    subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.RFX_ABI_VERSION, abi.TEX_MOTION_BLUR, abi.TEX_BLUR_SOURCE, abi.TEX_COUNT, abi.PROF_KINDS.index("k6_motion_blur"),
                   abi.PROF_KINDS.index("k6_motion_blur_reach"), len(abi.PROF_KINDS)]
    assert got[0] == 21 and got[2] == got[1] + 1 and got[5] == got[4] + 1  # appended after RFX_TEX_MOTION_BLUR / RFX_PROF_K6
    assert abi.TEX_FORMAT[abi.TEX_BLUR_SOURCE] == (np.float32, 4) and abi.TEX_NAMES[abi.TEX_BLUR_SOURCE] == "blur_source" and len(abi.TEX_NAMES) == abi.TEX_COUNT
    lib = abi.load_library()
    for name in ("rfx_motion_blur_reach_mask", "rfx_motion_blur_stage", "rfx_motion_blur_gather"):
        assert name in abi.EXPORTS and hasattr(lib, name)
    assert lib.rfx_tex_texel_bytes(abi.TEX_BLUR_SOURCE) == 16


@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_slot_table_has_the_blur_source():
    js = "const r=require(%r);console.log(JSON.stringify([r.TEX.BLUR_SOURCE,r.TEX.MOTION_BLUR,r.FORMAT[r.TEX.BLUR_SOURCE][1],r.abiVersion()]))" % os.path.join(JS, "Renderer")
    assert json.loads(subprocess.check_output([node, "-e", js], text=True)) == [abi.TEX_BLUR_SOURCE, abi.TEX_MOTION_BLUR, 4, abi.RFX_ABI_VERSION]


# ---------------------------------------------------------------- the two hosts' call sequences for a blurred frame
BLUR_RECORDER = r"""
const fx = require(process.argv[1] + "/effects")
const { TiledRenderer } = require(process.argv[1] + "/tiling")
const { TEX } = require(process.argv[1] + "/Renderer")
const cam = JSON.parse(process.argv[2])
const calls = []
const inner = {
  uploadPlane() {}, heldRows() { return [0, 0] },
  setRowWindow(a, b) { calls.push(["window", a, b]) },
  ssgiMarch(u) { calls.push(["ssgi"]) }, ssgiTrace(u) { calls.push(["trace"]) }, ssgiShade(u) { calls.push(["shade"]) },
  temporalReproject(u) { calls.push(["temporal"]) }, poissonDenoise(u) { calls.push(["denoise", u.writeToB]) },
  compose(u) { calls.push(["compose"]) }, finalCompose(u) { calls.push(["final"]) },
  motionBlur(u) { calls.push(["blur", u.source, u.center, u.samples, u.frame]) }, sync() { calls.push(["sync"]) }
}
const comm = { haloExchange(tex, up, down) { calls.push(["halo", tex, up, down]) }, allgatherHistory(tex) { calls.push(["gather", tex]) },
  gatherHistoryRows(tex) { calls.push(["gather_rows", tex]); return 0 }, commWait() { calls.push(["wait"]) },
  motionBlurGather(u) { calls.push(["blur_gather", u.source, u.center, u.samples, u.frame]); return 7 } }
const out = {}
for (const rn of [[0, 3], [1, 3], [2, 3], [0, 1]]) {
  calls.length = 0
  const r = new TiledRenderer(96, 66, rn[0], rn[1], 6, null, { inner, comm, historyGather: "bounded" })
  const e = new fx.SSGIEffect(null, { frame: {} }, cam, { width: 96, height: 66 }, { ssgi: 10, denoise: 20 })
  const mb = new fx.MotionBlurEffect(null, { samples: 5 })
  for (let i = 0; i < 2; i++) {
    e.update(r, null)
    mb.update(r, e.mainImage(r), 1 / 60)
    mb.mainImage(r)
  }
  r.sync()
  out[rn.join("/")] = { calls: calls.slice(), bytes: r.blurBytesReceived }
}
console.log(JSON.stringify(out))
"""


class _RecCtx:
    """a recording stand-in for the tile's Context"""

    def __init__(self, rank, world, W=96, H=66, halo=6):
        self.W, self.H, self.rank = W, H, rank
        self.tile_y0, self.tile_rows = tiling.split_rows(H, world)[rank]
        self.halo = halo if world > 1 else 0
        self.calls = []

    def held_rows(self, tex):
        return (0, 0)

    def upload(self, *a, **k):
        pass

    def comm_init(self, *a):
        pass

    def set_row_window(self, a=0, b=0):
        self.calls.append(["window", a, b])

    def ssgi_march(self, p):
        self.calls.append(["ssgi"])

    def ssgi_trace(self, p):
        self.calls.append(["trace"])

    def ssgi_shade(self, p):
        self.calls.append(["shade"])

    def temporal_reproject(self, p):
        self.calls.append(["temporal"])

    def poisson_denoise(self, p):
        self.calls.append(["denoise", p.writeToB])

    def compose(self, p):
        self.calls.append(["compose"])

    def final_compose(self, p):
        self.calls.append(["final"])

    def motion_blur(self, p):
        self.calls.append(["blur", p.source, p.center, p.samples, p.frame])

    def motion_blur_gather(self, p):
        self.calls.append(["blur_gather", p.source, p.center, p.samples, p.frame])
        return 7

    def halo_exchange(self, tex, up, down):
        self.calls.append(["halo", tex, up, down])

    def allgather_history(self, tex):
        self.calls.append(["gather", tex])

    def gather_history_rows(self, tex):
        self.calls.append(["gather_rows", tex])
        return 0

    def comm_wait(self):
        self.calls.append(["wait"])

    def sync(self):
        self.calls.append(["sync"])


@pytest.mark.skipif(node is None, reason="node not installed")
def test_tiled_renderers_issue_the_same_calls_for_a_blurred_frame():
    """js/tiling.js TiledRenderer.motionBlur against rfx_amd.tiling.CommTiledRenderer.motion_blur on recording stand-ins: after the effect's
    final image, the gather (stage + reach mask + exchange, one C call), the wait, the draw — for a bottom, a middle and a top rank of
    three and for a single rank."""
    from rfx_amd.scene import synthetic_frame
    f = synthetic_frame(32, 16, 0)
    cam_json = json.dumps({k: [float(x) for x in np.asarray(getattr(f.camera, k)).ravel()] for k in
                           ("projectionMatrix", "projectionMatrixInverse", "matrixWorld", "matrixWorldInverse", "position", "quaternion")} |
                          dict(near=f.camera.near, far=f.camera.far))
    js = json.loads(subprocess.check_output([node, "-e", BLUR_RECORDER, JS, cam_json], text=True, timeout=120).strip().splitlines()[-1])
    import types
    for rank, world in ((0, 3), (1, 3), (2, 3), (0, 1)):
        ctx = _RecCtx(rank, world)
        r = tiling.CommTiledRenderer(ctx, rank, world, b"\0" * 128, history_gather="bounded")
        fx = effect.SSGIEffect(None, types.SimpleNamespace(frame=f), f.camera, dict(width=96, height=66), seeds=dict(ssgi=10, denoise=20))
        mb = effect.MotionBlurEffect(None, {"samples": 5})
        for _ in range(2):
            fx.update(r, None)
            mb.update(r, fx.mainImage(r), 1 / 60)
            mb.mainImage(r)
        r.sync()
        got = js["%d/%d" % (rank, world)]
        assert got["calls"] == json.loads(json.dumps(ctx.calls)), (rank, world)
        assert got["bytes"] == r.blur_bytes_received == [7, 7]
        seq = [c[0] for c in ctx.calls]
        k = seq.index("blur_gather")
        assert seq[k - 1] == "final" and seq[k + 1:k + 3] == ["wait", "blur"] and ctx.calls[k][1:] == ctx.calls[k + 2][1:] == [abi.TEX_FINAL, -1, 5, 0]


# ---------------------------------------------------------------- TiledRenderer.motion_blur over gloo, on a numpy tile
class RefTile:
    """A tile whose draws are the numpy restatement: it holds the velocity, its own rows of the source, and a whole-frame blur-source plane
    that starts as NaN.  motion_blur_reach_mask is the set of texels the restatement's own fetches of the source load for the tile rows."""

    def __init__(self, W, H, y0, rows, velocity, source, blue, options):
        self.W, self.H, self.tile_y0, self.tile_rows, self.halo = W, H, y0, rows, 0
        self.velocity, self.blue, self.options = velocity, blue, options
        self.source_rows = np.ascontiguousarray(source[y0:y0 + rows], np.float32)  # all this tile owns of the source
        self.blur_source = np.full((H, W, 4), np.nan, np.float32)
        self.out = None
        self.calls = []

    def _draw(self, p, plane, record=None):
        plane = np.ascontiguousarray(plane, np.float32)
        moved = None
        if record is not None:
            with np.errstate(all="ignore"):
                vx, vy = self.velocity[..., 0], self.velocity[..., 1]
                moved = (vx * vx + vy * vy) > np.float32(1e-9)
        orig, n = R.linear_fetch, [0]

        def fetch(tex, u, v):
            if record is not None and tex is plane:
                record(u, v, np.ones_like(moved) if n[0] == 0 else moved)  # the first fetch is inputColor's: every fragment makes it
                n[0] += 1
            return orig(tex, u, v)
        R.linear_fetch = fetch
        try:
            return R.motion_blur(self.velocity, plane, blue_noise=self.blue, samples=p.samples, intensity=p.intensity, jitter=p.jitter,
                                 deltaTime=p.deltaTime, frame=p.frame, resolution=tuple(p.resolution), target_half=bool(p.targetHalf),
                                 half_rtz=bool(p.halfStoreRTZ))
        finally:
            R.linear_fetch = orig

    def motion_blur_stage(self, p):
        self.calls.append("stage")
        assert p.source == abi.TEX_EFFECT_INPUT and p.center == -1
        self.blur_source[self.tile_y0:self.tile_y0 + self.tile_rows] = self.source_rows

    def motion_blur_reach_mask(self, p):
        self.calls.append("reach_mask")
        W, H, a, b = self.W, self.H, self.tile_y0, self.tile_y0 + self.tile_rows
        mask = np.zeros(H, np.uint32)

        def coord(t, n):  # motion_blur_ref.linear_fetch's texel pair
            c = (np.asarray(t, np.float32) * np.float32(n)).astype(np.float32) - np.float32(0.5)
            c = np.where(np.isnan(c), np.float32(0), np.clip(c, np.float32(0), np.float32(n) - np.float32(0.5))).astype(np.float32)
            i0 = c.astype(np.int64)
            return i0, np.minimum(i0 + 1, n - 1)

        def record(u, v, live):
            with np.errstate(all="ignore"):
                xs, ys = coord(u, W), coord(v, H)
            live = live[a:b]
            for yy in ys:
                for xx in xs:
                    np.bitwise_or.at(mask, yy[a:b][live], (np.uint32(1) << ((xx[a:b][live] * 32) // W).astype(np.uint32)))
        self._draw(p, np.zeros((H, W, 4), np.float32), record)
        return mask

    def upload(self, tex, array, row0, rows):
        self.calls.append("upload")
        assert tex == abi.TEX_BLUR_SOURCE and not (self.tile_y0 <= row0 < self.tile_y0 + self.tile_rows)
        self.blur_source[row0:row0 + rows] = np.asarray(array, np.float32).reshape(rows, self.W, 4)

    def download(self, tex, row0, rows):
        assert tex == abi.TEX_BLUR_SOURCE
        return self.blur_source[row0:row0 + rows].copy()

    def motion_blur(self, p):
        self.calls.append("motion_blur")
        self.out = self._draw(p, self.blur_source)[self.tile_y0:self.tile_y0 + self.tile_rows]

    def sync(self):
        pass


GW, GH = 33, 20


def _gloo_case():
    rng = np.random.default_rng(2133)
    vel = np.zeros((GH, GW, 4), np.float32)
    vel[..., :2] = rng.uniform(-0.6, 0.6, (GH, GW, 2))  # streaks of up to 0.6 * 0.6 of the frame: across the 6-row tiles of three ranks
    kind = rng.integers(0, 6, (GH, GW))
    vel[kind == 0, :2] = 0
    vel[kind == 1, 0] = np.nan
    vel[kind == 2, :2] = 1e-6
    src = rng.uniform(0, 4, (GH, GW, 4)).astype(np.float32)
    p = abi.MotionBlurParams()
    p.source, p.center, p.samples, p.intensity, p.jitter, p.deltaTime, p.frame = abi.TEX_EFFECT_INPUT, -1, 5, 1.0, 1.0, 1 / 60, 3
    p.resolution[:] = [GW, GH]
    p.halfStoreRTZ = 1
    return vel, src, p


def _gloo_worker(rank, world, port, outdir):
    import torch.distributed as dist
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    vel, src, p = _gloo_case()
    y0, rows = tiling.split_rows(GH, world)[rank]
    tile = RefTile(GW, GH, y0, rows, vel, src, load_blue_noise_table(), None)
    r = tiling.TiledRenderer(tile, {}, rank, world)
    r.motion_blur(p)
    uploads = tile.calls.count("upload")
    assert tile.calls == ["stage", "reach_mask"] + ["upload"] * uploads + ["motion_blur"], tile.calls
    np.savez(os.path.join(outdir, "g%d.npz" % rank), y0=y0, rows=rows, out=tile.out, bytes=np.array(r.blur_bytes_received, np.int64), uploads=uploads)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_tiled_renderer_motion_blur_over_gloo(tmp_path, world):
    """stage, reach mask, all-gather of the masks, Send/Recv of the rows that carry any bit, upload, draw — the three calls the C ABI gives a
    host with its own transport — on numpy tiles: every rank's rows equal the whole-frame restatement's.  A row the mask or the transport
    missed stays NaN in the tile's plane and shows in the result."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_gloo_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    vel, src, p = _gloo_case()
    ref = R.motion_blur(vel, src, blue_noise=load_blue_noise_table(), samples=p.samples, intensity=p.intensity, jitter=p.jitter, deltaTime=p.deltaTime,
                        frame=p.frame, resolution=(GW, GH))
    assert np.isfinite(ref).all()
    received = 0
    for rank in range(world):
        z = np.load(os.path.join(str(tmp_path), "g%d.npz" % rank))
        y0, rows = int(z["y0"]), int(z["rows"])
        assert z["out"].tobytes() == ref[y0:y0 + rows].tobytes(), "rank %d of %d" % (rank, world)
        assert len(z["bytes"]) == 1 and 0 < int(z["bytes"][0]) <= (GH - rows) * GW * 16 and int(z["uploads"]) >= 1
        received += int(z["bytes"][0])
    assert received > 0
