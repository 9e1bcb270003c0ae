"""The Node host of the EXR blocks (rfx.h rfx_stage_exr_blocks through the N-API addon).  Without a device: imageio.exrAovLayout(buf, names, { forms:
"blocks" }) against the Python host's layout, record for record, and its default still refusing the same files.  On the device: one tiled ZIP
and one PXR24 file through exrAovLayout + Renderer.stageExrBlocks against the Python host's slots for the same file — DEPTH, GBUFFER, VELOCITY
and DIRECT_LIGHT byte for byte."""
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
W, H = 97, 55
HALF = ("diffuse", "normal", "roughness", "metalness", "emissive", "direct")

NODE_LAYOUT = r"""
const fs = require("fs"), path = require("path"), crypto = require("crypto")
const { exrAovLayout, ExrNotStreamable } = require(path.join(process.argv[1], "imageio.js"))
const sha = a => crypto.createHash("sha1").update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest("hex")
const out = {}
for (const name of JSON.parse(process.argv[3])) {
	const file = fs.readFileSync(path.join(process.argv[2], name))
	const r = { scanline: null }
	try { exrAovLayout(file); r.scanline = "taken" } catch (e) { r.scanline = e instanceof ExrNotStreamable ? "not streamable" : String(e) }
	try {
		const l = exrAovLayout(file, undefined, { forms: "blocks" })
		Object.assign(r, { width: l.width, height: l.height, fileBytes: l.fileBytes, planes: l.planes, parts: Array.from(l.parts), blocks: sha(l.blocks), blockCount: l.blockCount,
			chunks: l.chunks === undefined })
	} catch (e) { r.blocks = e instanceof ExrNotStreamable ? "not streamable" : String(e) }
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
	const layout = exrAovLayout(pinned, undefined, { forms: "blocks" })
	const bytes = r.exrBlocksStageBytes(pinned, layout), band = r.exrBlocksStageBytes(pinned, layout, 16, 24)
	r.stageExrBlocks(pinned, layout)
	r.stageFlip()
	out[name] = { status: r.exrAovStatus(), bytes, band, slots: slots.map(t => sha(r.download(t))) }
}
console.log(JSON.stringify(out))
"""


def write_files(tmp_path, w, h):
    from rfx_amd import imageio
    ch = X.channels(w, h, 6)
    half = {c for c in ch if c.split(".")[0] in HALF}
    imageio.write_exr(str(tmp_path / "tiled_zip.exr"), ch, "zip", half=half, tiles=(32, 8))
    imageio.write_exr(str(tmp_path / "pxr24.exr"), ch, "pxr24", half=half)
    imageio.write_exr_multipart(str(tmp_path / "mixed_rle.exr"), X.as_parts(ch), "rle", half=set(HALF), tiles={"normal": (16, 16), "depth": (64, 64)})
    imageio.write_exr(str(tmp_path / "zips.exr"), ch, "zips", half=half)
    imageio.write_exr(str(tmp_path / "piz.exr"), ch, "piz", half=True)
    return ["tiled_zip.exr", "pxr24.exr", "mixed_rle.exr", "zips.exr", "piz.exr"]


def words_of(lay):
    words = [len(lay.parts)]
    for comp, chans in lay.parts:
        words += [comp, len(chans)] + [x for c in chans for x in c]
    return words


@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_layout_of_blocks_equals_the_python_hosts(tmp_path):
    from rfx_amd import imageio
    names = write_files(tmp_path, W, H)
    res = json.loads(subprocess.check_output([node, "-e", NODE_LAYOUT, JS, str(tmp_path), json.dumps(names)], text=True, timeout=120).strip().splitlines()[-1])
    for name in names:
        r, path = res[name], str(tmp_path / name)
        assert r["scanline"] == ("taken" if name == "zips.exr" else "not streamable"), name
        if name == "piz.exr":
            assert r["blocks"] == "not streamable"
            continue
        lay = imageio.exr_aov_layout(path, forms="blocks")
        assert (r["width"], r["height"], r["fileBytes"], r["blockCount"]) == (W, H, lay.file_bytes, len(lay.blocks)) and r["chunks"] is True
        assert {k: tuple(v) for k, v in r["planes"].items()} == lay.planes and r["parts"] == words_of(lay)
        assert r["blocks"] == hashlib.sha1(lay.blocks.tobytes()).hexdigest(), name


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_stages_tiled_zip_and_pxr24_files_like_the_python_host(tmp_path):
    from rfx_amd import abi, imageio
    from rfx_amd.context import Context
    names = write_files(tmp_path, W, H)[:3]
    res = json.loads(subprocess.check_output([node, "-e", NODE_STAGE, JS, str(tmp_path), str(W), str(H), json.dumps(names)], text=True, timeout=120).strip().splitlines()[-1])
    c = Context(W, H)
    for name in names:
        data = open(str(tmp_path / name), "rb").read()
        lay = imageio.exr_aov_layout(data, forms="blocks")
        c.stage_exr_blocks(data, lay)
        c.stage_flip()
        want = [hashlib.sha1(np.ascontiguousarray(c.download(t)).tobytes()).hexdigest() for t in (abi.TEX_DEPTH, abi.TEX_GBUFFER, abi.TEX_VELOCITY, abi.TEX_DIRECT_LIGHT)]
        r = res[name]
        assert r["status"] == [0, -1, 0] and r["slots"] == want and len(set(want)) == 4, name
        assert r["bytes"] == int(lay.blocks["packed_bytes"].sum()) and r["band"] == int(lay.band_blocks(16, 24)["packed_bytes"].sum()) < r["bytes"]
    c.close()
