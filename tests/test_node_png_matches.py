"""GPU (-m gpu; also under --hostsim): the PNG fragment with run-length matches (rfx.h "Match form") through the Node host.  The Node
FrameExporter with encode: "device", matches: true writes files byte-identical to the Python host's for the same uploads, Renderer.png /
stagePng take { matches }, and `run_dump.js --framesEncode '"device"' --framesMatches true` writes PNGs with the pixels of the run without."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import match_cases as K
import match_device_ref as M
import png_device_ref as R
from rfx_amd import abi, frames, imageio
from test_node_png import plant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason="node not installed")]

NODE_FRAMES = r"""
const fs = require("fs")
const { Renderer, TEX, ENCODE_MATCHES } = require(process.argv[1] + "/Renderer")
const { FrameExporter } = require(process.argv[1] + "/frames")
const [W, H, N] = [Number(process.argv[2]), Number(process.argv[3]), Number(process.argv[5])]
const dir = process.argv[4]
const r = new Renderer(W, H)
const fx = new FrameExporter(r, dir + "/node", { format: "png", tonemap: "linear", exposure: 1, encode: "device", matches: true })
for (let i = 0; i < N; i++) {
  const b = fs.readFileSync(dir + "/in" + i + ".bin")
  r.upload(TEX.EFFECT_INPUT, new Float32Array(b.buffer, b.byteOffset, b.length / 4))
  fx.submit(TEX.EFFECT_INPUT)
}
fx.finish()
const save = (name, out) => fs.writeFileSync(dir + "/" + name, Buffer.from(out.buffer, out.byteOffset, out.byteLength))
save("node_on.bin", r.png({ source: TEX.EFFECT_INPUT, channels: 4 }, "paeth", undefined, { matches: true }))
save("node_off.bin", r.png({ source: TEX.EFFECT_INPUT, channels: 4 }, "paeth", undefined, { matches: false }))
const staged = new Uint8Array(r.pngBound({ channels: 4 }))
r.exportWait(r.stagePng({ source: TEX.EFFECT_INPUT, channels: 4 }, "paeth", staged, { matches: true }))
save("node_staged.bin", staged)
const refused = []
for (const o of [{ format: "png", matches: true }, { format: "exr", matches: true }, { format: "pfm", matches: true }]) {
  try { new FrameExporter(r, dir, o); refused.push("") } catch (e) { refused.push(String(e.message)) }
}
console.log(JSON.stringify({ refused, flag: ENCODE_MATCHES, off: new FrameExporter(r, dir, { format: "png", encode: "device" }).matches }))
"""


def test_node_frame_exporter_equals_python(tmp_path):
    from rfx_amd.context import Context
    W, H, N = 97, 55, 2
    imgs = [K.half_flat_bytes(W, H, 4, seed=70 + i) for i in range(N)]
    for i, img in enumerate(imgs):
        plant(img).tofile(str(tmp_path / ("in%d.bin" % i)))
    os.mkdir(str(tmp_path / "node"))
    os.mkdir(str(tmp_path / "python"))
    res = json.loads(subprocess.check_output([node, "-e", NODE_FRAMES, JS, str(W), str(H), str(tmp_path), str(N)], text=True).strip().splitlines()[-1])
    ctx = Context(W, H)
    fx = frames.FrameExporter(ctx, str(tmp_path / "python"), "png", tonemap="linear", exposure=1.0, encode="device", matches=True)
    for img in imgs:
        ctx.upload(abi.TEX_EFFECT_INPUT, plant(img))
        fx.submit(abi.TEX_EFFECT_INPUT)
    fx.finish()
    ctx.close()
    for i, img in enumerate(imgs):
        name = "frame_%05d.png" % i
        got = (tmp_path / "node" / name).read_bytes()
        assert got == (tmp_path / "python" / name).read_bytes(), i
        want = M.result_prefix_png(img[..., :3], 0)
        assert M.png_header_of(want)[4] > 0
        assert got == R.png_file(W, H, 3, [want]), i  # ... and both are the restatement's file
        assert np.array_equal(imageio.read_png(str(tmp_path / "node" / name)), img[..., :3])
    on, off = M.result_prefix_png(imgs[-1], 4), R.result_prefix(imgs[-1], 4)
    assert len(on) < len(off)
    assert (tmp_path / "node_on.bin").read_bytes()[:len(on)] == on == (tmp_path / "node_staged.bin").read_bytes()[:len(on)]
    assert (tmp_path / "node_off.bin").read_bytes()[:len(off)] == off
    assert all("framesMatches" in m for m in res["refused"]), res["refused"]
    assert res["flag"] == abi.ENCODE_MATCHES and res["off"] is False


def test_run_dump_frames_matches(tmp_path):
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    W, H, N = 96, 54, 2
    dirs = []
    for i in range(N):
        d = str(tmp_path / ("dump%d" % i))
        write_dump(d, synthetic_frame(W, H, i))
        dirs.append(d)
    outs = {}
    for matches in (False, True):
        out, fr = str(tmp_path / ("out_%d" % matches)), str(tmp_path / ("frames_%d" % matches))
        subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--steps", "8", "--refineSteps", "2", "--framesOut", fr,
                                "--framesEncode", '"device"', "--framesMatches", json.dumps(matches)], text=True)
        outs[matches] = (out, fr)
    for name in ("final.bin", "compose.bin"):  # every other output is byte-identical
        assert open(os.path.join(outs[False][0], name), "rb").read() == open(os.path.join(outs[True][0], name), "rb").read()
    for i in range(N):
        name = "frame_%05d.png" % i
        a, b = os.path.join(outs[False][1], name), os.path.join(outs[True][1], name)
        assert np.array_equal(imageio.read_png(a), imageio.read_png(b)), i  # K7's bytes either way
        assert os.path.getsize(b) <= os.path.getsize(a)
    p = subprocess.run([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", str(tmp_path / "o"), "--framesOut", str(tmp_path / "f"), "--framesMatches", "true"],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "framesMatches" in p.stderr
