"""The Node host of the PIZ device decode (rfx.h rfx_stage_exr_blocks_piz through the N-API addon).  Without a device: imageio.exrAovLayout(buf,
names, { forms: "blocks", piz: true }) against the Python host's layout, record for record, and its default still refusing the same files.  On
the device: a scanline and a tiled PIZ file through exrAovLayout + Renderer.stageExrBlocks against the Python HOST decode of the same file —
DEPTH, GBUFFER, VELOCITY and DIRECT_LIGHT byte for byte."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import exr_import_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
W, H = 97, 70
HALF = ("diffuse", "normal", "roughness", "metalness", "emissive", "direct")

NODE_LAYOUT = r"""
const fs = require("fs"), path = require("path"), crypto = require("crypto")
const { exrAovLayout, ExrNotStreamable } = require(path.join(process.argv[1], "imageio.js"))
const sha = a => crypto.createHash("sha1").update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest("hex")
const out = {}
for (const name of JSON.parse(process.argv[3])) {
	const file = fs.readFileSync(path.join(process.argv[2], name))
	const r = {}
	for (const [key, options] of [["default", { forms: "blocks" }], ["off", { forms: "blocks", piz: false }], ["scanline", { piz: true }]])
		try { exrAovLayout(file, undefined, options); r[key] = "taken" } catch (e) { r[key] = e instanceof ExrNotStreamable ? "not streamable" : String(e.message) }
	const l = exrAovLayout(file, undefined, { forms: "blocks", piz: true })
	Object.assign(r, { width: l.width, height: l.height, fileBytes: l.fileBytes, planes: l.planes, parts: Array.from(l.parts), blocks: sha(l.blocks), blockCount: l.blockCount })
	out[name] = r
}
console.log(JSON.stringify(out))
"""

NODE_STAGE = r"""
const fs = require("fs"), path = require("path"), crypto = require("crypto")
const [js, dir, W, H] = [process.argv[1], process.argv[2], +process.argv[3], +process.argv[4]]
const { Renderer, TEX, exrAovLayout } = require(js)
const sha = a => crypto.createHash("sha1").update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest("hex")
const slots = [TEX.DEPTH, TEX.GBUFFER, TEX.VELOCITY, TEX.DIRECT_LIGHT]
const r = new Renderer(W, H), out = {}
for (const name of JSON.parse(process.argv[5])) {
	const file = fs.readFileSync(path.join(dir, name))
	const pinned = Renderer.hostAlloc(Uint8Array, file.length)
	pinned.set(file)
	const layout = exrAovLayout(pinned, undefined, { forms: "blocks", piz: true })
	const bytes = r.exrBlocksStageBytes(pinned, layout), band = r.exrBlocksStageBytes(pinned, layout, 0, 6)
	r.stageExrBlocks(pinned, layout)
	r.stageFlip()
	out[name] = { status: r.exrAovStatus(), bytes, band, slots: slots.map(t => sha(r.download(t))) }
}
console.log(JSON.stringify(out))
"""


def write_files(tmp_path):
    from rfx_amd import imageio
    ch = X.channels(W, H, 6)
    half = {c for c in ch if c.split(".")[0] in HALF}
    imageio.write_exr(str(tmp_path / "piz.exr"), ch, "piz", half=half)
    imageio.write_exr(str(tmp_path / "tiled_piz.exr"), ch, "piz", half=half, tiles=(64, 64))
    imageio.write_exr_multipart(str(tmp_path / "parts_piz.exr"), X.as_parts(X.channels(33, 17, 6)), "piz", half=True)
    return ["piz.exr", "tiled_piz.exr", "parts_piz.exr"]


def words_of(lay):
    words = [len(lay.parts)]
    for comp, chans in lay.parts:
        words += [comp, len(chans)] + [x for c in chans for x in c]
    return words


@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_piz_layout_equals_the_python_hosts(tmp_path):
    from rfx_amd import imageio
    names = write_files(tmp_path)
    res = json.loads(subprocess.check_output([node, "-e", NODE_LAYOUT, JS, str(tmp_path), json.dumps(names)], text=True, timeout=120).strip().splitlines()[-1])
    for name in names:
        r, path = res[name], str(tmp_path / name)
        assert r["default"] == r["off"] == "not streamable" and "blocks" in r["scanline"], name
        lay = imageio.exr_aov_layout(path, forms="blocks", piz=True)
        size = (33, 17) if name == "parts_piz.exr" else (W, H)
        assert (r["width"], r["height"], r["fileBytes"], r["blockCount"]) == size + (lay.file_bytes, len(lay.blocks))
        assert {k: tuple(v) for k, v in r["planes"].items()} == lay.planes and r["parts"] == words_of(lay) and 4 in [comp for comp, _ in lay.parts]
        assert r["blocks"] == hashlib.sha1(lay.blocks.tobytes()).hexdigest(), name
    assert [int(v) for v in imageio.exr_aov_layout(str(tmp_path / "piz.exr"), forms="blocks", piz=True).blocks["rows"]] == [32, 32, 6]


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_stages_piz_files_like_the_python_host_decode(tmp_path):
    import test_gpu_exr_import as T
    from rfx_amd import imageio
    names = write_files(tmp_path)[:2]
    res = json.loads(subprocess.check_output([node, "-e", NODE_STAGE, JS, str(tmp_path), str(W), str(H), json.dumps(names)], text=True, timeout=120).strip().splitlines()[-1])
    for name in names:
        path = str(tmp_path / name)
        lay = imageio.exr_aov_layout(path, forms="blocks", piz=True)
        want = [hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest() for a in T.host_slots(W, H, path)]
        r = res[name]
        assert r["status"] == [0, -1, 0] and r["slots"] == want and len(set(want)) == 4, name
        raw = lay.blocks["rows"].astype(np.int64) * lay.blocks["cols"] * sum(2 if pt == 1 else 4 for pt, _, _ in lay.parts[0][1])
        assert (lay.blocks["packed_bytes"] < raw).any()
        assert r["bytes"] == int(lay.blocks["packed_bytes"].sum()) and r["band"] == int(lay.band_blocks(0, 6)["packed_bytes"].sum()) < r["bytes"]
