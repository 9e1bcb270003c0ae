"""GPU (-m gpu; also under --hostsim): the streamed frame export through the Node host.  The N-API calls give the Python host's bytes for the
same uploads, and `run_dump.js --framesOut` writes every frame — the device's bytes through the existing writers — without changing any
other output, plain, with --stream and with --motionBlur."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import export_cases as X
from rfx_amd import abi, imageio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason="node not installed")]

FORMS = (("f32", 3, "linear", 1.0), ("f32", 4, "linear", 1.0), ("f16", 3, "linear", 1.0), ("f16", 4, "linear", 1.0), ("u8_srgb", 3, "aces", 0.37),
         ("u8_srgb", 4, "linear", 2.5))

NODE_EXPORTS = r"""
const fs = require("fs")
const { Renderer, TEX, EXPORT_ARRAY } = require(process.argv[1] + "/Renderer")
const [W, H] = [Number(process.argv[2]), Number(process.argv[3])]
const forms = JSON.parse(process.argv[5])
const b = fs.readFileSync(process.argv[4] + "/in.bin")
const r = new Renderer(W, H)
r.upload(TEX.EFFECT_INPUT, new Float32Array(b.buffer, b.byteOffset, b.length / 4))
const save = (name, a) => fs.writeFileSync(process.argv[4] + "/" + name, Buffer.from(a.buffer, a.byteOffset, a.byteLength))
const tickets = []
forms.forEach((f, k) => {
  const p = { source: TEX.EFFECT_INPUT, format: f[0], channels: f[1], tonemap: f[2], exposure: f[3] }
  save("sync" + k + ".bin", r.exportFrame(p))
  const n = r.exportBytes(p) / EXPORT_ARRAY[r.exportParams(p).format].BYTES_PER_ELEMENT
  const out = Renderer.hostAlloc(EXPORT_ARRAY[r.exportParams(p).format], n)
  const t = r.stageExport(p, out)
  tickets.push(t)
  r.exportWait(t)
  save("staged" + k + ".bin", out)
})
let refused = ""
try { r.exportFrame({ source: TEX.DEPTH, format: "f32" }) } catch (e) { refused = String(e.message) }
console.log(JSON.stringify({ tickets, refused }))
"""


def test_node_exports_equal_python(tmp_path):
    from rfx_amd.context import Context
    W, H = 97, 55
    a = X.f16_input(W, H)
    a[np.isnan(a)] = 0.25
    a.tofile(str(tmp_path / "in.bin"))
    res = json.loads(subprocess.check_output([node, "-e", NODE_EXPORTS, JS, str(W), str(H), str(tmp_path), json.dumps(FORMS)], text=True).strip().splitlines()[-1])
    assert res["tickets"] == [2 * k + 2 for k in range(len(FORMS))]  # (exportFrame takes a ticket of its own)
    assert "rfx_export" in res["refused"]
    ctx = Context(W, H)
    ctx.upload(abi.TEX_EFFECT_INPUT, a)
    for k, f in enumerate(FORMS):
        want = ctx.export(abi.TEX_EFFECT_INPUT, *f).tobytes()
        assert open(str(tmp_path / ("sync%d.bin" % k)), "rb").read() == want, f
        assert open(str(tmp_path / ("staged%d.bin" % k)), "rb").read() == want, f
    ctx.close()


W, H, N = 96, 54, 3
BINS = ("final", "compose", "denoise_b0", "denoise_b1", "temporal0", "ssgi")
VARIANTS = {"plain": [], "stream": ["--stream", "true"], "motion_blur": ["--motionBlur", '{"samples":5,"intensity":2}']}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """run_dump.js runs over the first n dumps, made once per (variant, n, extra options) and shared by the cases"""
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    root = tmp_path_factory.mktemp("node_export")
    dirs = []
    for i in range(N):
        d = str(root / ("dump%d" % i))
        write_dump(d, synthetic_frame(W, H, i))
        dirs.append(d)
    done = {}

    def run(variant, n, *extra):
        key = (variant, n) + extra
        if key not in done:
            out = str(root / ("out%d" % len(done)))
            subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs[:n] + ["--out", out, "--steps", "8", "--refineSteps", "2"] + VARIANTS[variant] + list(extra), text=True)
            done[key] = out
        return done[key]
    return run


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _frames_run(runs, variant, n, fmt, root, *extra):
    d = os.path.join(str(root), "%s_%s_%d" % (variant, fmt, n))
    out = runs(variant, n, "--framesOut", d, "--framesFormat", json.dumps(fmt), *extra)
    return out, d


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_run_dump_writes_every_frame(runs, variant, tmp_path_factory):
    root = tmp_path_factory.mktemp("frames_" + variant)
    ref_variant = "plain" if variant == "stream" else variant  # --stream writes the same bytes as the plain run (tests/test_node_host.py)
    shown = "motion_blur" if variant == "motion_blur" else "final"  # the plane the images show
    base = runs(variant, N)
    last_pfm = os.path.join(str(root), "last.pfm")
    out_pfm, d_pfm = _frames_run(runs, variant, N, "pfm", root, "--pfm", json.dumps(last_pfm))
    out_png, d_png = _frames_run(runs, variant, N, "png", root)
    out_exr, d_exr = _frames_run(runs, variant, N, "exr", root)
    # every other output is byte-identical with and without --framesOut
    for out in (out_pfm, out_png, out_exr):
        for name in BINS + (("motion_blur",) if variant == "motion_blur" else ()):
            assert _read(os.path.join(out, name + ".bin")) == _read(os.path.join(base, name + ".bin")), (name, out)
    for d, ext in ((d_pfm, "pfm"), (d_png, "png"), (d_exr, "exr")):
        assert sorted(os.listdir(d)) == ["frame_%05d.%s" % (i, ext) for i in range(N)]
    # the last frame's .pfm is --pfm of the same run; each earlier one is --pfm of a run over the first i + 1 dumps
    assert _read(os.path.join(d_pfm, "frame_%05d.pfm" % (N - 1))) == _read(last_pfm)
    for i in range(N):
        if i < N - 1:
            ref_pfm = os.path.join(str(root), "ref%d.pfm" % i)
            ref_out = runs(ref_variant, i + 1, "--pfm", json.dumps(ref_pfm))
            assert _read(os.path.join(d_pfm, "frame_%05d.pfm" % i)) == _read(ref_pfm), i
        else:
            ref_out = base
        pfm = imageio.read_pfm(os.path.join(d_pfm, "frame_%05d.pfm" % i))
        # .png: the device's bytes, decoded, against tonemap of the matching .pfm under the margin rule
        v, ref = X.reference_v(pfm, 3, "aces", 1.0)
        X.check_margin(imageio.read_png(os.path.join(d_png, "frame_%05d.png" % i)), v, ref)
        # .exr: write_exr(half=True) of the same plane (RGBA: the run's own .bin of that frame)
        plane = np.fromfile(os.path.join(ref_out, shown + ".bin"), np.float32).reshape(H, W, 4)
        assert np.array_equal(plane[..., :3], pfm)
        want = os.path.join(str(root), "want%d.exr" % i)
        with np.errstate(over="ignore"):
            imageio.write_exr(want, {n: plane[..., k] for k, n in enumerate("RGBA")}, compression="none", half=True)
        assert _read(os.path.join(d_exr, "frame_%05d.exr" % i)) == _read(want), i
