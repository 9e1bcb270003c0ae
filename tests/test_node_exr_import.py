"""The Node host of the streamed EXR frames (rfx.h rfx_stage_exr_aov through the N-API addon): a 97 x 55 multi-part ZIP file through
imageio.exrAovLayout + Renderer.stageExrAov against the same frame's typed planes through Renderer.stageAov on a second renderer — DEPTH,
GBUFFER, VELOCITY and DIRECT_LIGHT byte for byte — and the layout against the Python host's."""
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

NODE_EXR = r"""
const fs = require("fs"), path = require("path"), crypto = require("crypto")
const [js, dir, W, H] = [process.argv[1], process.argv[2], +process.argv[3], +process.argv[4]]
const { Renderer, TEX, exrAovLayout, ExrNotStreamable } = require(js)
const sha = a => crypto.createHash("sha1").update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest("hex")
const file = fs.readFileSync(path.join(dir, "frame.exr"))
const pinned = Renderer.hostAlloc(Uint8Array, file.length)
pinned.set(file)
const layout = exrAovLayout(pinned)
const a = new Renderer(W, H), b = new Renderer(W, H)
const bytes = a.exrAovStageBytes(pinned, layout)
a.stageExrAov(pinned, layout)
a.stageFlip()
const status = a.exrAovStatus()
const planes = {}
for (const [name, half] of JSON.parse(process.argv[5])) {
	const raw = fs.readFileSync(path.join(dir, name + ".bin"))
	planes[name] = half ? new Uint16Array(raw.buffer, raw.byteOffset, raw.length / 2) : new Float32Array(raw.buffer, raw.byteOffset, raw.length / 4)
}
b.stageAov(planes)
b.stageFlip()
const slots = [TEX.DEPTH, TEX.GBUFFER, TEX.VELOCITY, TEX.DIRECT_LIGHT]
let refused = null
try { exrAovLayout(fs.readFileSync(path.join(dir, "piz.exr"))) } catch (e) { refused = e instanceof ExrNotStreamable }
console.log(JSON.stringify({ device: slots.map(t => sha(a.download(t))), host: slots.map(t => sha(b.download(t))), bytes, status, refused,
	width: layout.width, height: layout.height, planes: layout.planes, parts: Array.from(layout.parts), chunks: sha(layout.chunks), chunkCount: layout.chunkCount }))
"""


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_stages_an_exr_file_like_its_typed_planes(tmp_path):
    import hashlib

    from rfx_amd import imageio
    ch = X.channels(W, H, 6)
    path = str(tmp_path / "frame.exr")
    imageio.write_exr_multipart(path, X.as_parts(ch), "zip", half=set(HALF))
    imageio.write_exr(str(tmp_path / "piz.exr"), ch, "piz", half=True)
    t = imageio.exr_to_typed_planes(path)
    planes = dict(t["aov"], depth=t["depth"], direct=t["direct"])
    for k, v in planes.items():
        assert v.dtype == (np.float16 if k in HALF else np.float32), k
        np.ascontiguousarray(v).tofile(str(tmp_path / (k + ".bin")))
    res = json.loads(subprocess.check_output([node, "-e", NODE_EXR, JS, str(tmp_path), str(W), str(H), json.dumps([[k, k in HALF] for k in planes])],
                                             text=True, timeout=120).strip().splitlines()[-1])
    assert res["device"] == res["host"] and len(set(res["device"])) == 4
    lay = imageio.exr_aov_layout(path)
    assert res["status"] == [0, -1, 0] and res["bytes"] == int(lay.chunks["packed_bytes"].sum()) and res["refused"] is True
    assert (res["width"], res["height"], res["chunkCount"]) == (W, H, len(lay.chunks))
    assert {k: tuple(v) for k, v in res["planes"].items()} == lay.planes
    words = [len(lay.parts)]
    for comp, chans in lay.parts:
        words += [comp, len(chans)] + [x for c in chans for x in c]
    assert res["parts"] == words
    assert res["chunks"] == hashlib.sha1(lay.chunks.tobytes()).hexdigest()
