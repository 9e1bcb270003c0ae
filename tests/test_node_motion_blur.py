"""MotionBlurEffect through the Node host (js/effects.js, N-API motionBlur, run_dump.js --motionBlur).
CPU: the option surface and the uniforms update() sets equal the Python host's (a recording renderer, no device calls).
GPU (-m gpu): run_dump.js --motionBlur, after SSGIEffect and in the README TRAA form, equals the Python host bit for bit."""
import json
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from rfx_amd import abi, effect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
pytestmark = pytest.mark.skipif(node is None, reason="no node")

RECORDER = r"""
const fx = require(process.argv[1] + "/effects")
const { TEX } = require(process.argv[1] + "/Renderer")
const calls = []
const r = { width: 8, height: 4, upload: (tex, a, row0, rows) => calls.push(["upload", tex, a.length, row0, rows]),
            motionBlur: u => calls.push(["motion_blur", u.source, u.center, u.centerAlphaOne, u.samples, u.intensity, u.jitter, u.frame,
                                         Math.fround(u.deltaTime), u.resolution, u.targetHalf, u.halfStoreRTZ]) }
const e = new fx.MotionBlurEffect(new fx.VelocityDepthNormalPass(null, null))
const surface = [e.intensity, e.jitter, e.samples]
e.intensity = 2.5; e.jitter = 0; e.samples = 4
surface.push(e.samples, e.uniforms.samples, e.uniforms.intensity, e.uniforms.jitter)
e.update(r, TEX.FINAL, 0); e.mainImage(r)
e.update(r, TEX.TEMPORAL0, 1 / 60); e.mainImage(r)
e.frame = 4097; e.resolution = [1920, 1080]
e.update(r, { texture: { type: fx.HalfFloatType }, data: new Float32Array(8 * 4 * 4).fill(1.0001) }, 1 / 30); e.mainImage(r)
const traa = new fx.TRAAEffect(null, null, null)
traa.uniforms.accumulatedTexture = TEX.TEMPORAL0
e.shareEffectPass(traa)
e.update(r, null, 1 / 60); e.mainImage(r)
const e2 = new fx.MotionBlurEffect(null, { samples: 7, intensity: -1 })
console.log(JSON.stringify({ surface, calls, e2: [e2.uniforms.samples, e2.uniforms.intensity, e2.uniforms.jitter], defaults: fx.defaultMotionBlurOptions }))
"""


class _Recorder:
    W, H = 8, 4

    def __init__(self):
        self.calls = []

    def upload(self, tex, a):
        self.calls.append(["upload", tex, a.size, 0, a.shape[0]])

    def motion_blur(self, p):
        self.calls.append(["motion_blur", p.source, p.center, p.centerAlphaOne, p.samples, p.intensity, p.jitter, p.frame, p.deltaTime,
                           list(p.resolution), p.targetHalf, p.halfStoreRTZ])


def test_node_option_surface_equals_python():
    """MotionBlurEffect.js:14,37-45,51-66,85-101 in both hosts: defaults, the fixed `samples` define, the reactive intensity / jitter, and
    the uniforms of update() for a slot input, TRAA's own-pass output (alpha 1), a HalfFloatType host buffer and the README form."""
    js = json.loads(subprocess.check_output([node, "-e", RECORDER, JS], text=True).strip().splitlines()[-1])
    e = effect.MotionBlurEffect(effect.VelocityDepthNormalPass(None, None))
    surface = [e.intensity, e.jitter, e.samples]
    e.intensity, e.jitter, e.samples = 2.5, 0, 4
    surface += [e.samples, e.uniforms.samples, e.uniforms.intensity, e.uniforms.jitter]
    r = _Recorder()
    e.update(r, abi.TEX_FINAL, 0)
    e.mainImage(r)
    e.update(r, abi.TEX_TEMPORAL0, 1 / 60)
    e.mainImage(r)
    e.frame, e.resolution = 4097, (1920, 1080)
    e.update(r, dict(texture=dict(type=effect.HalfFloatType), data=np.full((4, 8, 4), 1.0001, np.float32)), 1 / 30)
    e.mainImage(r)
    traa = effect.TRAAEffect(None, None, None)
    traa.uniforms["accumulatedTexture"] = abi.TEX_TEMPORAL0
    e.shareEffectPass(traa)
    e.update(r, None, 1 / 60)
    e.mainImage(r)
    e2 = effect.MotionBlurEffect(None, {"samples": 7, "intensity": -1})
    assert js["surface"] == surface
    assert js["calls"] == r.calls
    assert js["e2"] == [e2.uniforms.samples, e2.uniforms.intensity, e2.uniforms.jitter]
    assert js["defaults"] == effect.defaultMotionBlurOptions
    assert r.calls[1][1:4] == [abi.TEX_TEMPORAL0, -1, 1]  # TRAA's own-pass output: alpha 1


@pytest.mark.gpu
def test_node_run_dump_motion_blur_equals_python(tmp_path):
    from rfx_amd import imageio
    from rfx_amd.context import Context
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    W, H = 160, 96
    frames = [synthetic_frame(W, H, i) for i in range(2)]
    dirs = []
    for i, f in enumerate(frames):
        d = str(tmp_path / ("dump%d" % i))
        write_dump(d, f)
        dirs.append(d)
    opts = {"intensity": 2, "jitter": 1.5, "samples": 9}
    dt = 1 / 45
    # after SSGIEffect's final image, on the device
    out = str(tmp_path / "js_ssgi")
    res = subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--steps", "12", "--refineSteps", "3", "--importanceSampling",
                                   "false", "--motionBlur", json.dumps(opts), "--deltaTime", json.dumps(dt), "--exr", json.dumps(str(tmp_path / "mb.exr"))],
                                  text=True)
    assert json.loads(res.strip().splitlines()[-1])["frames"] == 2
    scene = types.SimpleNamespace(frame=None)
    cam = types.SimpleNamespace(**vars(frames[0].camera))
    fx = effect.SSGIEffect(None, scene, cam, dict(width=W, height=H, steps=12, refineSteps=3, importanceSampling=False), seeds=dict(ssgi=11, denoise=22),
                           half_store_rtz=True)
    mb = effect.MotionBlurEffect(effect.VelocityDepthNormalPass(scene, cam), opts)
    ctx = Context(W, H)
    for f in frames:
        scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        fx.update(ctx, None)
        fx.mainImage(ctx)
        mb.update(ctx, abi.TEX_FINAL, dt)
        mb.mainImage(ctx)
    py = mb.output(ctx)
    final = ctx.download(abi.TEX_FINAL)
    ctx.close()
    js = np.fromfile(os.path.join(out, "motion_blur.bin"), np.float32).reshape(py.shape)
    assert np.array_equal(py.view(np.uint8), js.view(np.uint8))
    assert not np.array_equal(py, final)
    assert np.array_equal(np.fromfile(os.path.join(out, "final.bin"), np.float32).reshape(final.shape).view(np.uint8), final.view(np.uint8))
    e = imageio.read_exr(str(tmp_path / "mb.exr"))
    assert np.array_equal(np.stack([e[c] for c in "RGBA"], -1), py)  # --exr carries the blurred frame
    # the README form after TRAAEffect, HalfFloatType composer buffers
    out = str(tmp_path / "js_traa")
    subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--traa", json.dumps("half"), "--motionBlur", json.dumps(opts)],
                            text=True)
    scene = types.SimpleNamespace(frame=None)
    cam = types.SimpleNamespace(**vars(frames[0].camera))
    vp = effect.VelocityDepthNormalPass(scene, cam)
    tx = effect.TRAAEffect(scene, cam, vp, dict(fullAccumulate=True), half_store_rtz=True)
    mb = effect.MotionBlurEffect(vp, opts)
    mb.shareEffectPass(tx)
    ctx = Context(W, H)
    for f in frames:
        scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        tx.update(ctx, dict(texture=dict(type=effect.HalfFloatType), width=W, height=H, data=f.direct))
        mb.update(ctx, None, 1 / 60)
        mb.mainImage(ctx)
    py = mb.output(ctx)
    ctx.close()
    js = np.fromfile(os.path.join(out, "motion_blur.bin"), np.float32).reshape(py.shape)
    assert np.array_equal(py.view(np.uint8), js.view(np.uint8))
    assert (py[..., 3] == 1).all() and np.array_equal(py, py.astype(np.float16).astype(np.float32))  # alpha 1, half texels
