"""GPU (-m gpu; also under --hostsim): the device-encoded PNG through the Node host.  The Node FrameExporter with encode: "device" writes files
byte-identical to the Python host's for the same uploads, and `run_dump.js --framesOut DIR --framesEncode '"device"'` writes PNGs that decode to
the pixels of the host-encoded run's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import png_device_ref as R
from rfx_amd import abi, frames, imageio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason="node not installed")]

NODE_FRAMES = r"""
const fs = require("fs")
const { Renderer, TEX } = require(process.argv[1] + "/Renderer")
const { FrameExporter } = require(process.argv[1] + "/frames")
const [W, H, N] = [Number(process.argv[2]), Number(process.argv[3]), Number(process.argv[5])]
const dir = process.argv[4]
const r = new Renderer(W, H)
const fx = new FrameExporter(r, dir + "/node", { format: "png", tonemap: "linear", exposure: 1, encode: "device" })
for (let i = 0; i < N; i++) {
  const b = fs.readFileSync(dir + "/in" + i + ".bin")
  r.upload(TEX.EFFECT_INPUT, new Float32Array(b.buffer, b.byteOffset, b.length / 4))
  fx.submit(TEX.EFFECT_INPUT)
}
fx.finish()
const out = r.png({ source: TEX.EFFECT_INPUT, channels: 4 }, "paeth")
fs.writeFileSync(dir + "/node_rgba_paeth.bin", Buffer.from(out.buffer, out.byteOffset, out.byteLength))
let refused = ""
try { new FrameExporter(r, dir, { format: "exr", encode: "device" }) } catch (e) { refused = String(e.message) }
r.profile(1)
r.png({ source: TEX.EFFECT_INPUT })
r.profile(0)
console.log(JSON.stringify({ bound: r.pngBound({ channels: 4 }), refused, launches: r.profileRead().launches }))
"""


def plant(img):
    """the (H, W, 4) float32 plane whose linear U8_SRGB export is exactly `img` (tests/test_gpu_png.py)"""
    s = img[..., :3].astype(np.float64) / 255.0
    lin = np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)
    a = img[..., 3:4].astype(np.float64) / 255.0 if img.shape[-1] == 4 else np.ones(img.shape[:2] + (1,))
    return np.concatenate([lin, a], -1).astype(np.float32)


def test_node_frame_exporter_equals_python(tmp_path):
    from rfx_amd.context import Context
    W, H, N = 97, 55, 2
    imgs = [R.noisy_frame(W, H, 4, seed=70 + i) for i in range(N)]
    for i, img in enumerate(imgs):
        plant(img).tofile(str(tmp_path / ("in%d.bin" % i)))
    os.mkdir(str(tmp_path / "node"))
    os.mkdir(str(tmp_path / "python"))
    res = json.loads(subprocess.check_output([node, "-e", NODE_FRAMES, JS, str(W), str(H), str(tmp_path), str(N)], text=True).strip().splitlines()[-1])
    ctx = Context(W, H)
    fx = frames.FrameExporter(ctx, str(tmp_path / "python"), "png", tonemap="linear", exposure=1.0, encode="device")
    for img in imgs:
        ctx.upload(abi.TEX_EFFECT_INPUT, plant(img))
        fx.submit(abi.TEX_EFFECT_INPUT)
    fx.finish()
    want_rgba = ctx.png(abi.TEX_EFFECT_INPUT, 4, filter="paeth")
    assert res["bound"] == ctx.png_bound(4) == want_rgba.nbytes
    ctx.close()
    for i, img in enumerate(imgs):
        name = "frame_%05d.png" % i
        got = (tmp_path / "node" / name).read_bytes()
        assert got == (tmp_path / "python" / name).read_bytes(), i
        assert got == R.png_file(W, H, 3, [R.result_prefix(img[..., :3], 0)]), i  # ... and both are the restatement's file
        assert np.array_equal(imageio.read_png(str(tmp_path / "node" / name)), img[..., :3])
    n = 32 + int(np.frombuffer(want_rgba[:8].tobytes(), np.uint64)[0])
    assert (tmp_path / "node_rgba_paeth.bin").read_bytes()[:n] == want_rgba[:n].tobytes() == R.result_prefix(imgs[-1], 4)
    assert "png" in res["refused"]
    assert res["launches"][abi.PROF_KINDS_ALL.index("k8_png")] == 1 and len(res["launches"]) == len(abi.PROF_KINDS_ALL)


def test_run_dump_frames_encode_device(tmp_path):
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    W, H, N = 96, 54, 2
    dirs = []
    for i in range(N):
        d = str(tmp_path / ("dump%d" % i))
        write_dump(d, synthetic_frame(W, H, i))
        dirs.append(d)
    outs = {}
    for enc in ("host", "device"):
        out, fr = str(tmp_path / ("out_" + enc)), str(tmp_path / ("frames_" + enc))
        subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--steps", "8", "--refineSteps", "2", "--framesOut", fr,
                                "--framesEncode", json.dumps(enc)], text=True)
        outs[enc] = (out, fr)
    for name in ("final.bin", "compose.bin"):  # every other output is byte-identical
        assert open(os.path.join(outs["host"][0], name), "rb").read() == open(os.path.join(outs["device"][0], name), "rb").read()
    assert sorted(os.listdir(outs["device"][1])) == ["frame_%05d.png" % i for i in range(N)]
    for i in range(N):
        name = "frame_%05d.png" % i
        host = imageio.read_png(os.path.join(outs["host"][1], name))
        dev = imageio.read_png(os.path.join(outs["device"][1], name))
        assert np.array_equal(host, dev), i  # K7's bytes either way
    p = subprocess.run([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", str(tmp_path / "o"), "--framesOut", str(tmp_path / "f"), "--framesFormat", '"pfm"',
                        "--framesEncode", '"device"'], capture_output=True, text=True)
    assert p.returncode != 0 and "png" in p.stderr
