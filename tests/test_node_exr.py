"""GPU (-m gpu; also under --hostsim): the device-encoded EXR through the Node host.  The Node FrameExporter with compression: "zips" writes
files byte-identical to the Python host's for the same uploads, and `run_dump.js --framesOut DIR --framesFormat '"exr"' --framesCompression
'"zips"'` writes EXR files that the project's reader returns bit-identical to the uncompressed path's."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import exr_device_ref as E
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
const fx = new FrameExporter(r, dir + "/node", { format: "exr", compression: "zips" })
for (let i = 0; i < N; i++) {
  const b = fs.readFileSync(dir + "/in" + i + ".bin")
  r.upload(TEX.EFFECT_INPUT, new Float32Array(b.buffer, b.byteOffset, b.length / 4))
  fx.submit(TEX.EFFECT_INPUT)
}
fx.finish()
const out = r.exr({ source: TEX.EFFECT_INPUT, channels: 3 })
fs.writeFileSync(dir + "/node_rgb.bin", Buffer.from(out.buffer, out.byteOffset, out.byteLength))
const refused = []
for (const o of [{ format: "png", compression: "zips" }, { format: "pfm", compression: "zips" }, { format: "exr", compression: "zip" }, { format: "exr", encode: "device" }]) {
  try { new FrameExporter(r, dir, o); refused.push("") } catch (e) { refused.push(String(e.message)) }
}
const plain = new FrameExporter(r, dir, { format: "exr" })
r.profile(1)
r.exr({ source: TEX.EFFECT_INPUT })
r.profile(0)
console.log(JSON.stringify({ bound: r.exrBound({ channels: 3 }), bound4: r.exrBound(), refused, plain: plain.compression, launches: r.profileRead().launches }))
"""


def plane_of(halfs):
    a = np.ones(halfs.shape[:2] + (4,), np.float32)
    a[..., :halfs.shape[-1]] = halfs.astype(np.float32)
    return a


def same_halfs(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


def read_back(path, ch=4):
    planes = imageio.read_exr(path)
    return np.stack([planes[c] for c in "RGBA"[:ch]], -1).astype(np.float16)


def test_node_frame_exporter_equals_python(tmp_path):
    from rfx_amd.context import Context
    W, H, N = 97, 55, 2
    imgs = [E.smooth_noisy_halfs(W, H, 4, seed=80 + i) for i in range(N)]
    imgs[1][1::2] = E.random_halfs(W, H // 2, 4, seed=82)  # raw chunks between the compressed ones
    for i, img in enumerate(imgs):
        plane_of(img).tofile(str(tmp_path / ("in%d.bin" % i)))
    os.mkdir(str(tmp_path / "node"))
    os.mkdir(str(tmp_path / "python"))
    res = json.loads(subprocess.check_output([node, "-e", NODE_FRAMES, JS, str(W), str(H), str(tmp_path), str(N)], text=True).strip().splitlines()[-1])
    ctx = Context(W, H)
    fx = frames.FrameExporter(ctx, str(tmp_path / "python"), "exr", compression="zips")
    for img in imgs:
        ctx.upload(abi.TEX_EFFECT_INPUT, plane_of(img))
        fx.submit(abi.TEX_EFFECT_INPUT)
    fx.finish()
    want_rgb = ctx.exr(abi.TEX_EFFECT_INPUT, 3)
    assert res["bound"] == ctx.exr_bound(3) == want_rgb.nbytes and res["bound4"] == ctx.exr_bound(4)
    ctx.close()
    for i, img in enumerate(imgs):
        name = "frame_%05d.exr" % i
        got = (tmp_path / "node" / name).read_bytes()
        assert got == (tmp_path / "python" / name).read_bytes(), i
        assert got == imageio.exr_from_fragments(W, H, 4, [E.result_prefix(img)]), i  # ... and both are the restatement's file
        assert same_halfs(read_back(str(tmp_path / "node" / name)), img)
    n = 32 + E.header_of(want_rgb)[0]
    assert (tmp_path / "node_rgb.bin").read_bytes()[:n] == want_rgb[:n].tobytes() == E.result_prefix(imgs[-1][..., :3])
    assert all("exr" in m for m in res["refused"][:2]) and "none" in res["refused"][2] and "png" in res["refused"][3], res["refused"]
    assert res["plain"] == "none"
    assert res["launches"][abi.PROF_KINDS_ALL.index("k8_png")] == 1 and len(res["launches"]) == len(abi.PROF_KINDS_ALL)


def test_run_dump_frames_compression_zips(tmp_path):
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    W, H, N = 96, 54, 2
    dirs = []
    for i in range(N):
        d = str(tmp_path / ("dump%d" % i))
        write_dump(d, synthetic_frame(W, H, i))
        dirs.append(d)
    outs = {}
    for comp in ("none", "zips"):
        out, fr = str(tmp_path / ("out_" + comp)), str(tmp_path / ("frames_" + comp))
        subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--steps", "8", "--refineSteps", "2", "--framesOut", fr,
                                "--framesFormat", '"exr"', "--framesCompression", json.dumps(comp)], text=True)
        outs[comp] = (out, fr)
    for name in ("final.bin", "compose.bin"):  # every other output is byte-identical
        assert open(os.path.join(outs["none"][0], name), "rb").read() == open(os.path.join(outs["zips"][0], name), "rb").read()
    assert sorted(os.listdir(outs["zips"][1])) == ["frame_%05d.exr" % i for i in range(N)]
    for i in range(N):
        name = "frame_%05d.exr" % i
        plain, zips = os.path.join(outs["none"][1], name), os.path.join(outs["zips"][1], name)
        assert same_halfs(read_back(plain), read_back(zips)), i  # K7's halfs either way
        assert os.path.getsize(zips) <= os.path.getsize(plain)
    p = subprocess.run([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", str(tmp_path / "o"), "--framesOut", str(tmp_path / "f"), "--framesFormat", '"png"',
                        "--framesCompression", '"zips"'], capture_output=True, text=True)
    assert p.returncode != 0 and "exr" in p.stderr
