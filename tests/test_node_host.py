"""The Node host (realism-effects_amd/js, N-API addon) against the Python host.

CPU: same option surface / defaults, and the SAME C-ABI call sequence with the same parameter
values for a 3-frame run (a recording renderer on both sides).
GPU (-m gpu): run_dump.js drives the real library over dumped frames; its outputs must be
bit-identical to the Python host's (both are thin drivers of the same librfx_hip.so)."""
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
pytestmark = pytest.mark.skipif(node is None, reason="node not installed")

RECORDER = r"""
const fx = require(process.argv[1] + "/effects")
const cam = JSON.parse(process.argv[2])
const calls = []
const r5 = x => Math.round(x * 1e5) / 1e5
const R = {
  uploadPlane() {},
  ssgiMarch(u) { calls.push(["ssgi", u.steps, u.refineSteps, u.useDirectLight, u.rayDistance, u.thickness, u.blueNoiseIndex]) },
  temporalReproject(u) { calls.push(["temporal", u.keepData, u.fullAccumulate, u.textureCount, u.inputType, u.reprojectSpecular, u.logTransform, r5(u.confidencePower), u.neighborhoodClampIntensity, u.maxBlend]) },
  poissonDenoise(u) { calls.push(["denoise", u.inputIsTemporal, u.writeToB, u.radius, u.normalPhi, u.roughnessPhi, u.specularPhi, u.isTextureSpecular, u.blueNoiseIndex]) },
  compose(u) { calls.push(["compose", u.inputType]) }
}
const e = new fx.SSGIEffect(null, { frame: {} }, cam, { width: 32, height: 16 }, { ssgi: 10, denoise: 20 })
e.update(R, null); e.update(R, null)
e.radius = 5; e.denoiseIterations = 2; e.steps = "8"; e.denoiseKernel = 3
e.update(R, null)
const t = new fx.TRAAEffect({}, cam, new fx.VelocityDepthNormalPass({}, cam), { fullAccumulate: true, maxBlend: 0.5 }).temporalParams()
// TRAAEffect.update end to end on a recording renderer, HalfFloatType then FloatType composer buffers
const traaCalls = []
const RT = {
  uploadPlane(tex, plane) { traaCalls.push(["upload", tex, plane.length]) },
  temporalReproject(u) { traaCalls.push(["temporal", u.keepData, u.fullAccumulate, u.textureCount, u.inputType, u.historySource, u.targetHalf, u.halfStoreRTZ, u.maxBlend, u.confidencePower]) },
  copyFramebuffer(tex) { traaCalls.push(["copy", tex]) }
}
const data = new Float32Array(32 * 16 * 4).fill(0.1)
for (const type of [fx.HalfFloatType, fx.FloatType]) {
  const sc = { frame: { velocity: new Uint32Array(32 * 16 * 4) } }
  const e2 = new fx.TRAAEffect(sc, cam, new fx.VelocityDepthNormalPass(sc, cam), { fullAccumulate: true })
  e2.update(RT, { texture: { type }, width: 32, height: 16, data }); e2.update(RT, { texture: { type }, width: 32, height: 16, data })
}
// the other Denoiser modes: same pass construction and source wiring on both hosts
const modeCalls = {}
for (const dm of ["full_temporal", "temporal", "denoised"]) {
  const mc = []
  const RM = {
    uploadPlane() {},
    ssgiMarch(u) { mc.push(["ssgi", u.historySource]) },
    temporalReproject(u) { mc.push(["temporal", u.textureCount, u.historySource, u.targetHalf]) },
    copyFramebuffer(t) { mc.push(["copy", t]) },
    poissonDenoise(u) { mc.push(["denoise", u.inputIsTemporal, u.writeToB]) },
    compose(u) { mc.push(["compose", u.inputType, u.giSource]) },
    finalCompose(u) { mc.push(["final", u.inputSource, u.fogMode]) }
  }
  const em = new fx.SSGIEffect(null, { frame: {}, fog: { isFogExp2: true, color: [0.1, 0.2, 0.3], density: 0.02 } }, cam, { width: 32, height: 16, denoiseMode: dm }, { ssgi: 1, denoise: 2 })
  em.update(RM, null); em.mainImage(RM)
  modeCalls[dm] = mc
}
const low = new fx.SSGIEffect(null, { frame: {} }, cam, { width: 32, height: 16, preset: "low" }, { ssgi: 1, denoise: 2 })
const half = new fx.SSGIEffect(null, { frame: {} }, cam, { width: 32, height: 16, resolutionScale: 0.5 }, { ssgi: 1, denoise: 2 })
const halfU = [half.ssgiPass.uniforms.resolutionScale, half.denoiser.temporalReprojectPass.uniforms.inputWidth, half.denoiser.temporalReprojectPass.uniforms.inputHeight]
const halfProbe = JSON.parse(process.argv[3]).map(fx.roundToHalf).map(x => Number.isFinite(x) ? x : String(x))
console.log(JSON.stringify({ calls, defaults: fx.SSGIEffect.DefaultOptions, traa: [t.textureCount, t.inputType, t.logTransform, t.maxBlend, t.confidencePower, t.neighborhoodClampIntensity],
                             traaCalls, halfProbe, r2: fx.r2Sequence.slice(0, 3), modeCalls, low: [low.steps, low.refineSteps, low.denoiser.options.denoiseMode], halfU }))
"""


class Rec:
    def __init__(self):
        self.calls = []
        self.W, self.H = 32, 16

    def held_rows(self, tex):
        return 0, 16

    def upload(self, *a, **k):
        pass

    def ssgi_march(self, p):
        self.calls.append(["ssgi", p.steps, p.refineSteps, p.useDirectLight, p.rayDistance, p.thickness, p.blueNoiseIndex])

    def temporal_reproject(self, p):
        self.calls.append(["temporal", p.keepData, p.fullAccumulate, p.textureCount, p.inputType, list(p.reprojectSpecular), p.logTransform,
                           round(p.confidencePower, 5), p.neighborhoodClampIntensity, p.maxBlend])

    def poisson_denoise(self, p):
        self.calls.append(["denoise", p.inputIsTemporal, p.writeToB, p.radius, p.normalPhi, p.roughnessPhi, p.specularPhi, list(p.isTextureSpecular),
                           p.blueNoiseIndex])

    def compose(self, p):
        self.calls.append(["compose", p.inputType])


class RecTRAA(Rec):
    def upload(self, tex, array, row0=None, rows=None):
        self.calls.append(["upload", tex, int(np.asarray(array).size)])

    def temporal_reproject(self, p):
        self.calls.append(["temporal", p.keepData, p.fullAccumulate, p.textureCount, p.inputType, p.historySource, p.targetHalf, p.halfStoreRTZ,
                           round(p.maxBlend, 5), p.confidencePower])

    def copy_framebuffer(self, tex):
        self.calls.append(["copy", tex])


HALF_PROBE = [0.0, 1.0, -1.0, 0.1, 1.0 / 3.0, 65504.0, 65519.9, 65520.0, 1e-8, 5.9604645e-08, 2.9802322e-08, 3.0e-08, 6.1e-05, 6.1035156e-05, 1000.5,
              2049.0, 2051.0, -0.33333334, 123456.0]


def test_js_and_python_hosts_issue_the_same_calls():
    from rfx_amd.scene import synthetic_frame
    f = synthetic_frame(32, 16, 0)
    camd = {k: [float(x) for x in np.asarray(getattr(f.camera, k)).ravel()] for k in
            ("projectionMatrix", "projectionMatrixInverse", "matrixWorld", "matrixWorldInverse", "position", "quaternion")}
    camd.update(near=f.camera.near, far=f.camera.far)
    out = subprocess.check_output([node, "-e", RECORDER, JS, json.dumps(camd), json.dumps(HALF_PROBE)], cwd=JS)
    js = json.loads(out)

    scene = types.SimpleNamespace(frame=f)
    fx = effect.SSGIEffect(None, scene, f.camera, dict(width=32, height=16), seeds=dict(ssgi=10, denoise=20))
    r = Rec()
    fx.update(r, None)
    fx.update(r, None)
    fx.radius = 5
    fx.denoiseIterations = 2
    fx.steps = "8"
    fx.denoiseKernel = 3
    fx.update(r, None)
    assert js["calls"] == json.loads(json.dumps(r.calls))
    assert js["defaults"] == json.loads(json.dumps(effect.defaultSSGIOptions))
    t = effect.TRAAEffect(scene, f.camera, effect.VelocityDepthNormalPass(scene, f.camera), dict(fullAccumulate=True, maxBlend=0.5)).temporal_params()
    assert js["traa"] == [t.textureCount, t.inputType, t.logTransform, pytest.approx(t.maxBlend), t.confidencePower, t.neighborhoodClampIntensity]
    # TRAAEffect.update: same device calls from both hosts (velocity upload, input-buffer upload, K2, framebuffer copy)
    rt = RecTRAA()
    data = np.full((16, 32, 4), 0.1, np.float32)
    for ttype in (effect.HalfFloatType, effect.FloatType):
        sc = types.SimpleNamespace(frame=types.SimpleNamespace(velocity=np.zeros((16, 32, 4), np.uint32)))
        e2 = effect.TRAAEffect(sc, f.camera, effect.VelocityDepthNormalPass(sc, f.camera), dict(fullAccumulate=True))
        for _ in range(2):
            e2.update(rt, dict(texture=dict(type=ttype), width=32, height=16, data=data))
    # the Python host skips re-sending a resident plane (same ndarray), the JS host wraps the buffer in a fresh view per frame
    py = [c for c in rt.calls if c[0] != "upload"]
    assert [c for c in js["traaCalls"] if c[0] != "upload"] == json.loads(json.dumps(py))
    assert [c[:2] for c in js["traaCalls"] if c[0] == "upload"][:2] == [["upload", abi.TEX_VELOCITY], ["upload", abi.TEX_SSGI]]
    # denoiseMode "full_temporal" / "temporal" / "denoised": same passes, same source wiring
    class RecModes(Rec):
        def ssgi_march(self, p):
            self.calls.append(["ssgi", p.historySource])

        def temporal_reproject(self, p):
            self.calls.append(["temporal", p.textureCount, p.historySource, p.targetHalf])

        def copy_framebuffer(self, t):
            self.calls.append(["copy", t])

        def poisson_denoise(self, p):
            self.calls.append(["denoise", p.inputIsTemporal, p.writeToB])

        def compose(self, p):
            self.calls.append(["compose", p.inputType, p.giSource])

        def final_compose(self, p):
            self.calls.append(["final", p.inputSource, p.fogMode])

    for dm in ("full_temporal", "temporal", "denoised"):
        rm = RecModes()
        sc = types.SimpleNamespace(frame=f, fog=types.SimpleNamespace(isFogExp2=True, color=(0.1, 0.2, 0.3), density=0.02))
        em = effect.SSGIEffect(None, sc, f.camera, dict(width=32, height=16, denoiseMode=dm), seeds=dict(ssgi=1, denoise=2))
        em.update(rm, None)
        em.mainImage(rm)
        assert js["modeCalls"][dm] == rm.calls, dm
    low = effect.SSGIEffect(None, scene, f.camera, dict(width=32, height=16, preset="low"), seeds=dict(ssgi=1, denoise=2))
    assert js["low"] == [low.steps, low.refineSteps, low.denoiser.options["denoiseMode"]] == [10, 2, "full_temporal"]
    hs = effect.SSGIEffect(None, scene, f.camera, dict(width=32, height=16, resolutionScale=0.5), seeds=dict(ssgi=1, denoise=2))
    tu = hs.denoiser.temporalReprojectPass.uniforms
    assert js["halfU"] == [hs.ssgiPass.uniforms.resolutionScale, tu.inputWidth, tu.inputHeight] == [0.5, 16, 8]
    # the JS float->half rounding (no Float16Array in Node 12) against numpy's
    want = np.array(HALF_PROBE, np.float32).astype(np.float16).astype(np.float32)
    got = np.array([float(x) for x in js["halfProbe"]], np.float32)
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), (want, got)
    assert np.allclose(js["r2"], effect.r2Sequence[:3], rtol=0, atol=0)


def test_addon_loads_and_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = subprocess.run([node, "-e", "const r=require('./index'); console.log(r.abiVersion()); new r.Renderer(64,64)"], cwd=JS, capture_output=True,
                       text=True)
    assert p.stdout.strip() == str(abi.RFX_ABI_VERSION)
    assert p.returncode != 0 and "rfx_create failed" in p.stderr


@pytest.mark.gpu
def test_node_host_drives_the_gpu_bit_identically(tmp_path):
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
    out = str(tmp_path / "js_out")
    from rfx_amd.scene import synthetic_environment
    envimg = synthetic_environment(64, 32)
    envf = str(tmp_path / "env.bin")
    envimg.tofile(envf)
    res = subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--steps", "12", "--refineSteps", "3", "--env", json.dumps(envf),
                                   "--envWidth", "64", "--envHeight", "32"], text=True)  # default options: importanceSampling
    assert json.loads(res.strip().splitlines()[-1])["frames"] == 2

    scene = types.SimpleNamespace(frame=None, environment=dict(data=envimg))
    cam = types.SimpleNamespace(**vars(frames[0].camera))
    fx = effect.SSGIEffect(None, scene, cam, dict(width=W, height=H, steps=12, refineSteps=3), seeds=dict(ssgi=11, denoise=22), half_store_rtz=True)
    ctx = Context(W, H)
    for f in frames:
        scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        fx.update(ctx, None)
    fx.mainImage(ctx)
    for name, tex in (("final", abi.TEX_FINAL), ("compose", abi.TEX_COMPOSE), ("denoise_b0", abi.TEX_DENOISE_B0), ("denoise_b1", abi.TEX_DENOISE_B1), ("temporal0", abi.TEX_TEMPORAL0),
                      ("ssgi", abi.TEX_SSGI)):
        py = ctx.download(tex)
        js = np.fromfile(os.path.join(out, name + ".bin"), py.dtype).reshape(py.shape)
        assert np.array_equal(py.view(np.uint8), js.view(np.uint8)), name
    final_py = ctx.download(abi.TEX_FINAL)
    ctx.close()
    # --stream (pinned planes on the upload stream, frame n+1 staged while frame n is drawn) writes the same bytes; --png / --exr carry
    # the final image: the EXR holds its exact float32 texels, the PNG is the ACES tone map of them (to 1 LSB of the Python twin)
    from rfx_amd import imageio
    out_s = str(tmp_path / "js_stream")
    res = subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out_s, "--steps", "12", "--refineSteps", "3", "--env", json.dumps(envf),
                                   "--envWidth", "64", "--envHeight", "32", "--stream", "true", "--png", json.dumps(str(tmp_path / "f.png")),
                                   "--exr", json.dumps(str(tmp_path / "f.exr"))], text=True)
    assert json.loads(res.strip().splitlines()[-1])["haloViolations"] == 0
    for name in ("final", "compose", "denoise_b1"):
        assert open(os.path.join(out, name + ".bin"), "rb").read() == open(os.path.join(out_s, name + ".bin"), "rb").read(), name
    e = imageio.read_exr(str(tmp_path / "f.exr"))
    assert np.array_equal(np.stack([e[c] for c in "RGBA"], -1), final_py)
    assert np.abs(imageio.read_png(str(tmp_path / "f.png")).astype(np.int32) - imageio.tonemap(final_py).astype(np.int32)).max() <= 1
    # the Node host from UNPACKED attribute planes (device-side importer) == the Python host from the same planes
    gen_frames = [__import__("rfx_amd.scene", fromlist=["AnalyticScene"]).AnalyticScene(1234).render(W, H, i, aov=True) for i in range(2)]
    adirs = []
    for i, fr in enumerate(gen_frames):
        d = str(tmp_path / ("aov%d" % i))
        write_dump(d, fr, packed=False)
        adirs.append(d)
    out = str(tmp_path / "js_aov")
    subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + adirs + ["--out", out, "--steps", "12", "--refineSteps", "3"], text=True)
    from rfx_amd.dump import read_dump
    scene = types.SimpleNamespace(frame=None)
    cam = types.SimpleNamespace(**vars(gen_frames[0].camera))
    fx2 = effect.SSGIEffect(None, scene, cam, dict(width=W, height=H, steps=12, refineSteps=3), seeds=dict(ssgi=11, denoise=22), half_store_rtz=True)
    ctx = Context(W, H)
    for d, fr in zip(adirs, gen_frames):
        scene.frame = read_dump(d)
        assert scene.frame.gbuffer is None and scene.frame.aov is not None
        for k, v in vars(fr.camera).items():
            setattr(cam, k, v)
        fx2.update(ctx, None)
    py = ctx.download(abi.TEX_COMPOSE)
    js = np.fromfile(os.path.join(out, "compose.bin"), np.float32).reshape(py.shape)
    assert np.array_equal(py.view(np.uint8), js.view(np.uint8))
    ctx.close()
    # TRAAEffect through both hosts
    for mode, ttype in (("half", effect.HalfFloatType), ("float", effect.FloatType)):
        out = str(tmp_path / ("js_traa_" + mode))
        subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--traa", json.dumps(mode)], text=True)
        scene = types.SimpleNamespace(frame=None)
        cam = types.SimpleNamespace(**vars(frames[0].camera))
        tx = effect.TRAAEffect(scene, cam, effect.VelocityDepthNormalPass(scene, cam), dict(fullAccumulate=True), half_store_rtz=True)
        ctx = Context(W, H)
        for f in frames:
            scene.frame = f
            for k, v in vars(f.camera).items():
                setattr(cam, k, v)
            tx.update(ctx, dict(texture=dict(type=ttype), width=W, height=H, data=f.direct))
        py = tx.output(ctx)
        js = np.fromfile(os.path.join(out, "traa.bin"), np.float32).reshape(py.shape)
        assert np.array_equal(py.view(np.uint8), js.view(np.uint8)), mode
        ctx.close()


TILED_RECORDER = r"""
const fx = require(process.argv[1] + "/effects")
const { TiledRenderer } = require(process.argv[1] + "/tiling")
const cam = JSON.parse(process.argv[2])
const calls = []
const inner = {
  uploadPlane() {}, heldRows() { return [0, 0] },
  setRowWindow(a, b) { calls.push(["window", a, b]) },
  ssgiMarch(u) { calls.push(["ssgi", u.historySource]) }, ssgiTrace(u) { calls.push(["trace", u.historySource]) }, ssgiShade(u) { calls.push(["shade", u.historySource]) },
  temporalReproject(u) { calls.push(["temporal"]) }, poissonDenoise(u) { calls.push(["denoise", u.writeToB]) },
  compose(u) { calls.push(["compose", u.writeHistoryRGB]) }, sync() { calls.push(["sync"]) }
}
const comm = { haloExchange(tex, up, down) { calls.push(["halo", tex, up, down]) }, allgatherHistory(tex) { calls.push(["gather", tex]) },
  gatherHistoryRows(tex) { calls.push(["gather_rows", tex]); return 0 }, commWait() { calls.push(["wait"]) },
  peerExport(tex) { calls.push(["peer_export", tex]); return Buffer.alloc(192, 1 + rank) }, peerOpen(tex, blobs, r, n) { calls.push(["peer_open", tex, Array.from(blobs.filter((_, i) => i % 192 === 0)), r, n]) },
  peerGatherHistory(tex) { calls.push(["peer_gather", tex]); return 0 } }
let rank = 0
const out = {}
for (const rn of [[0, 3, "bounded"], [1, 3, "bounded"], [2, 3, "bounded"], [0, 1, "bounded"], [1, 3, "all"], [0, 3, "peer"], [2, 3, "peer"], [0, 1, "peer"]]) {
  calls.length = 0
  rank = rn[0]
  const r = new TiledRenderer(96, 66, rn[0], rn[1], 6, null, { inner, comm, historyGather: rn[2] === "peer" ? "all" : rn[2] })
  if (rn[2] === "peer") r.usePeerHistory(b => Array.from({ length: rn[1] }, (_, q) => (q === rn[0] ? b : Buffer.alloc(192, 1 + q))))
  const e = new fx.SSGIEffect(null, { frame: {} }, cam, { width: 96, height: 66 }, { ssgi: 10, denoise: 20 })
  e.update(r, null); e.update(r, null); r.sync()
  out[rn.join("/")] = { calls: calls.slice(), tile: [r.tileY0, r.tileRows], exchanges: r.exchangeCount }
}
console.log(JSON.stringify(out))
"""


def test_node_tiled_renderer_call_sequence_equals_python(tmp_path):
    """js/tiling.js TiledRenderer (the Node multi-process host's exchange protocol over the C ABI's RCCL entry points) against
    rfx_amd.tiling.CommTiledRenderer, both on recording stand-ins for the tile renderer and the exchange layer: the same draws, windows
    (interior first, then the boundary strips), halo exchanges, gathers and waits, in the same order, for a bottom, a middle and a top
    rank of three and for a single rank — in the three forms of the composed-GI exchange ("all", "bounded", "peer")."""
    from rfx_amd import tiling
    from rfx_amd.scene import synthetic_frame
    f = synthetic_frame(32, 16, 0)
    cam_json = json.dumps({k: [float(x) for x in np.asarray(getattr(f.camera, k)).ravel()] for k in
                           ("projectionMatrix", "projectionMatrixInverse", "matrixWorld", "matrixWorldInverse", "position", "quaternion")} |
                          dict(near=f.camera.near, far=f.camera.far))
    js = json.loads(subprocess.check_output([node, "-e", TILED_RECORDER, JS, cam_json], text=True).strip().splitlines()[-1])

    W, H, halo = 96, 66, 6

    class RecCtx:
        def __init__(self, rank, world):
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
            self.calls.append(["ssgi", p.historySource])

        def ssgi_trace(self, p):
            self.calls.append(["trace", p.historySource])

        def ssgi_shade(self, p):
            self.calls.append(["shade", p.historySource])

        def temporal_reproject(self, p):
            self.calls.append(["temporal"])

        def poisson_denoise(self, p):
            self.calls.append(["denoise", p.writeToB])

        def compose(self, p):
            self.calls.append(["compose", p.writeHistoryRGB])

        def halo_exchange(self, tex, up, down):
            self.calls.append(["halo", tex, up, down])

        def allgather_history(self, tex):
            self.calls.append(["gather", tex])

        def gather_history_rows(self, tex):
            self.calls.append(["gather_rows", tex])
            return 0

        def peer_export(self, tex):
            self.calls.append(["peer_export", tex])
            return bytes([1 + self.rank]) * 192

        def peer_open(self, tex, blobs, rank, world):
            self.calls.append(["peer_open", tex, [b[0] for b in blobs], rank, world])

        def peer_gather_history(self, tex):
            self.calls.append(["peer_gather", tex])
            return 0

        def comm_wait(self):
            self.calls.append(["wait"])

        def sync(self):
            self.calls.append(["sync"])

    for rank, world, mode in ((0, 3, "bounded"), (1, 3, "bounded"), (2, 3, "bounded"), (0, 1, "bounded"), (1, 3, "all"), (0, 3, "peer"), (2, 3, "peer"), (0, 1, "peer")):
        ctx = RecCtx(rank, world)
        r = tiling.CommTiledRenderer(ctx, rank, world, b"\0" * 128, history_gather="all" if mode == "peer" else mode)
        if mode == "peer":  # the device-driven pull (rfx_peer_*): the blobs travel once, then one call between trace and shade, no collective
            r.use_peer_history(lambda b: [b if q == rank else bytes([1 + q]) * 192 for q in range(world)])
        scene = types.SimpleNamespace(frame=types.SimpleNamespace(depth=np.zeros((0, W), np.float32), gbuffer=np.zeros((0, W, 4), np.uint32),
                                                                  velocity=np.zeros((0, W, 4), np.uint32), direct=np.zeros((0, W, 4), np.float32),
                                                                  camera=f.camera, aov=None))
        fx = effect.SSGIEffect(None, scene, f.camera, dict(width=W, height=H), seeds=dict(ssgi=10, denoise=20))
        fx.update(r, None)
        fx.update(r, None)
        r.sync()
        got = js["%d/%d/%s" % (rank, world, mode)]
        assert got["tile"] == [ctx.tile_y0, ctx.tile_rows]
        if world > 1:  # the composed GI travels either between trace and shade (bounded) or after K4 (all), never both
            kinds = {c[0] for c in ctx.calls}
            assert ("gather_rows" in kinds) == (mode == "bounded") and ("gather" in kinds) == (mode == "all") and ("peer_gather" in kinds) == (mode == "peer"), kinds
        assert got["calls"] == json.loads(json.dumps(ctx.calls)), (rank, world, got["calls"][:12], ctx.calls[:12])
        assert got["exchanges"] == r.exchange_count


CUBE_RECORDER = r"""
const fx = require(process.argv[1] + "/effects")
const cam = JSON.parse(process.argv[2])
const calls = []
const R = {
  uploadPlane() {}, ssgiMarch(u) { calls.push(["ssgi", u.useEnvMap, u.importanceSampling]) }, temporalReproject() {}, poissonDenoise() {}, compose() {},
  cubeToEquirect(faces, size, w, h, mips) { calls.push(["cube", faces.length, size, w, h, !!mips]); const o = new Float32Array(w * h * 4); for (let i = 0; i < o.length; i++) o[i] = 0.25 + (i % 7) * 0.125; return o },
  setEnvironment(data, w, h, half, rtz) { calls.push(["env", data ? data.length : null, w, h, !!half]) },
  setEnvironmentImportance(m, c, t) { calls.push(["imp", m.length, c.length]) }
}
const S = 32
const scene = { frame: {}, environment: { isCubeTexture: true, faces: new Float32Array(6 * S * S * 4).fill(1), size: S } }
const e = new fx.SSGIEffect(null, scene, cam, { width: 32, height: 16 }, { ssgi: 10, denoise: 20 })
e.update(R, null); e.update(R, null)
scene.environment = { isCubeTexture: true, faces: scene.environment.faces, size: S, minFilter: fx.LinearFilter, generateMipmaps: false }
e.update(R, null)
let refused = false
scene.environment = { isCubeTexture: true, faces: scene.environment.faces, size: S, minFilter: fx.NearestFilter }
try { e.update(R, null) } catch (err) { refused = /minFilter/.test(err.message) }
const big = new fx.CubeToEquirectEnvPass().generateEquirectEnvMap({ cubeToEquirect: (f, s, w, h) => new Float32Array(4) }, { faces: null, size: 2048 })
console.log(JSON.stringify({ calls, refused, big: [big.width, big.height] }))
"""


def test_cube_environment_js_and_python_hosts_issue_the_same_calls():
    """scene.environment as a CubeTexture (SSGIEffect.js:316-321 -> CubeToEquirectEnvPass.generateEquirectEnvMap): both hosts convert once, at
    the reference's target size, with the chain three's sampler state implies, and continue with a FloatType equirectangular map."""
    from rfx_amd.scene import synthetic_frame
    f = synthetic_frame(32, 16, 0)
    camd = {k: [float(x) for x in np.asarray(getattr(f.camera, k)).ravel()] for k in
            ("projectionMatrix", "projectionMatrixInverse", "matrixWorld", "matrixWorldInverse", "position", "quaternion")}
    camd.update(near=f.camera.near, far=f.camera.far)
    js = json.loads(subprocess.check_output([node, "-e", CUBE_RECORDER, JS, json.dumps(camd)], cwd=JS, text=True).strip().splitlines()[-1])

    class RecCube(Rec):
        def ssgi_march(self, p):
            self.calls.append(["ssgi", p.useEnvMap, p.importanceSampling])

        def temporal_reproject(self, p):
            pass

        def poisson_denoise(self, p):
            pass

        def compose(self, p):
            pass

        def cube_to_equirect(self, faces, w, h, generate_mipmaps=False):
            self.calls.append(["cube", int(np.asarray(faces).size), int(np.asarray(faces).shape[1]), w, h, bool(generate_mipmaps)])
            return (0.25 + (np.arange(w * h * 4) % 7) * 0.125).astype(np.float32).reshape(h, w, 4)

        def set_environment(self, data, half_float_type=True, half_store_rtz=True):
            self.calls.append(["env", None if data is None else int(data.size), data.shape[1], data.shape[0], bool(half_float_type)])

        def set_environment_importance(self, m, c, t):
            self.calls.append(["imp", int(np.asarray(m).size), int(np.asarray(c).size)])

    S = 32
    faces = np.ones((6, S, S, 4), np.float32)
    scene = types.SimpleNamespace(frame=f, environment=dict(isCubeTexture=True, faces=faces))
    fx = effect.SSGIEffect(None, scene, f.camera, dict(width=32, height=16), seeds=dict(ssgi=10, denoise=20))
    r = RecCube()
    fx.update(r, None)
    fx.update(r, None)
    scene.environment = dict(isCubeTexture=True, faces=faces, minFilter=effect.LinearFilter, generateMipmaps=False)
    fx.update(r, None)
    scene.environment = dict(isCubeTexture=True, faces=faces, minFilter=effect.NearestFilter)
    with pytest.raises(NotImplementedError):
        fx.update(r, None)
    assert js["refused"] is True
    assert js["calls"] == json.loads(json.dumps(r.calls))
    assert ["cube", 6 * S * S * 4, S, 128, 64, True] in js["calls"] and ["cube", 6 * S * S * 4, S, 128, 64, False] in js["calls"]
    assert js["big"] == [4096, 2048]  # maxWidth (:71-74)
    assert effect.CubeToEquirectEnvPass().generateEquirectEnvMap(types.SimpleNamespace(cube_to_equirect=lambda fa, w, h, generate_mipmaps: np.zeros((h, w, 4), np.float32)),
                                                                 dict(faces=np.zeros((6, 2048, 1, 4), np.float32)))["data"].shape == (2048, 4096, 4)


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("RFX_HOSTSIM") != "1", reason="one Node process per tile without RCCL / without N GPUs: pytest --hostsim")
@pytest.mark.parametrize("ranks", [2, 3])
def test_node_row_tiled_run_equals_single_process(tmp_path, ranks):
    """`run_dump.js --ranks N`: N Node processes, each driving its tile through the N-API addon, exchanging halo rows and the composed GI
    through the C ABI (rfx_comm_* / rfx_halo_exchange / rfx_allgather_history — under --hostsim over tests/hostsim/fakerccl.c), stitched by
    the parent: the same bytes as one process rendering the whole frame with one launch per draw."""
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    W, H = 160, 96
    dirs = []
    for i in range(3):
        d = str(tmp_path / ("dump%d" % i))
        write_dump(d, synthetic_frame(W, H, i))
        dirs.append(d)
    env = dict(os.environ, RFX_ONE_GPU="1")
    one, many = str(tmp_path / "one"), str(tmp_path / "many")
    subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", one, "--steps", "12", "--refineSteps", "3"], text=True, env=env)
    res = subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", many, "--steps", "12", "--refineSteps", "3", "--ranks", str(ranks)],
                                  text=True, env=env, timeout=600)
    info = json.loads(res.strip().splitlines()[-1])
    assert info["ranks"] == ranks and info["haloViolations"] == 0 and info["frames"] == 3
    for name in ("final", "compose", "denoise_b0", "denoise_b1", "temporal0", "ssgi"):
        a, b = open(os.path.join(one, name + ".bin"), "rb").read(), open(os.path.join(many, name + ".bin"), "rb").read()
        assert a == b, name


PEER_WORKERS = r"""
"use strict"
// Two row tiles of one frame, one worker thread each, both on device 0: js/tiling.js TiledRenderer with historyGather "peer" (the real
// N-API rfx_peer_* calls: the two contexts' barrier and pull kernels meet on the device), and a TEST exchange layer for the halo rows —
// host copies between the two threads in lock step — because two RCCL ranks cannot share one GPU.
const { Worker, isMainThread, workerData } = require("worker_threads")
const fs = require("fs"), path = require("path")
const N = 2
if (isMainThread) {
  const [JS, dumps, out, opt] = [process.argv[2], JSON.parse(process.argv[3]), process.argv[4], JSON.parse(process.argv[5])]
  const shared = { ctl: new SharedArrayBuffer(16), blobs: new SharedArrayBuffer(192 * N), rows: new SharedArrayBuffer(N * 2 * (1 << 20)) }
  let left = N
  const info = []
  for (let rank = 0; rank < N; rank++)
    new Worker(__filename, { workerData: Object.assign({ JS, dumps, out, opt, rank }, shared) })
      .on("message", m => (info[rank] = m)).on("error", e => { console.error(e); process.exit(1) })
      .on("exit", code => { if (code) process.exit(code); if (!--left) console.log(JSON.stringify(info)) })
} else {
  const { JS, dumps, out, opt, rank } = workerData
  const rfx = require(JS + "/index")
  const addon = require(JS + "/../napi/rfx_napi.node")
  const ctl = new Int32Array(workerData.ctl)
  const barrier = () => {
    const g = Atomics.load(ctl, 1)
    if (Atomics.add(ctl, 0, 1) === N - 1) { Atomics.store(ctl, 0, 0); Atomics.add(ctl, 1, 1); Atomics.notify(ctl, 1) }
    else { const t0 = Date.now(); while (Atomics.load(ctl, 1) === g) { Atomics.wait(ctl, 1, g, 200); if (Date.now() - t0 > 60000) throw new Error("rank " + rank + ": the other tile never arrived") } }
  }
  const slot = (r, k) => new Uint8Array(workerData.rows, (r * 2 + k) * (1 << 20), 1 << 20)
  let R
  const put = (k, a) => { const b = new Uint8Array(a.buffer, a.byteOffset, a.byteLength); slot(rank, k).set(b); return a }
  const get = (r, k, like) => { const b = new Uint8Array(like.byteLength); b.set(slot(r, k).subarray(0, like.byteLength)); return new like.constructor(b.buffer) }
  const comm = {
    haloExchange(tex, up, down) {
      const y0 = R.tileY0, y1 = y0 + R.tileRows, h = R.haloRows
      let top, bottom
      if (up >= 0) top = put(0, R.inner.download(tex, y1 - h, h))
      if (down >= 0) bottom = put(1, R.inner.download(tex, y0, h))
      barrier()
      if (up >= 0) R.inner.upload(tex, get(up, 1, top), y1, h)
      if (down >= 0) R.inner.upload(tex, get(down, 0, bottom), y0 - h, h)
      barrier()
    },
    allgatherHistory() { throw new Error("not in this mode") }, gatherHistoryRows() { throw new Error("not in this mode") },
    commWait: () => addon.commWait(R.inner._h),
    peerExport: tex => addon.peerExport(R.inner._h, tex), peerOpen: (tex, blobs, r, n) => addon.peerOpen(R.inner._h, tex, blobs, r, n),
    // the two tiles issue the call together, as ranks in lock step do: each worker reads and uploads its next dump before the frame, and under a
    // loaded host that alone can put one thread's call past the other's bounded device poll (~2 s); the kernels still meet on the device
    peerGatherHistory: tex => { barrier(); return addon.peerGatherHistory(R.inner._h, tex) }, peerClose: () => addon.peerClose(R.inner._h)
  }
  const first = rfx.readDump(dumps[0])
  R = new rfx.TiledRenderer(first.width, first.height, rank, N, opt.halo, null, { comm, device: 0 })
  R.usePeerHistory(blob => {
    new Uint8Array(workerData.blobs, 192 * rank, 192).set(blob)
    barrier()
    return Array.from({ length: N }, (_, q) => Buffer.from(new Uint8Array(workerData.blobs, 192 * q, 192)))
  })
  const scene = { frame: first }, camera = Object.assign({}, first.camera)
  const effect = new rfx.SSGIEffect(null, scene, camera, { width: first.width, height: first.height, steps: opt.steps, refineSteps: opt.refineSteps }, { ssgi: 11, denoise: 22 }, true)
  for (const d of dumps) {
    const f = d === dumps[0] ? first : rfx.readDump(d)
    scene.frame = f
    Object.assign(camera, f.camera)
    effect.update(R, null)
  }
  R.sync()
  effect.mainImage(R)
  for (const [name, tex] of [["final", rfx.TEX.FINAL], ["compose", rfx.TEX.COMPOSE], ["denoise_b0", rfx.TEX.DENOISE_B0], ["temporal0", rfx.TEX.TEMPORAL0], ["ssgi", rfx.TEX.SSGI]]) {
    const a = R.download(tex, R.tileY0, R.tileRows)
    fs.writeFileSync(path.join(out, name + ".rank" + rank + ".bin"), Buffer.from(a.buffer, a.byteOffset, a.byteLength))
  }
  const pulled = R.historyBytesReceived.slice() // (each call reports what the call before it pulled)
  barrier() // neither plane is unmapped while the other tile may still read it
  require("worker_threads").parentPort.postMessage({ rank, pulled, haloViolations: R.haloViolations(), exchanges: R.exchangeCount, mode: R.historyGather })
}
"""


@pytest.mark.gpu
def test_node_peer_history_gather_between_two_tiles_on_one_gpu(tmp_path):
    """js/tiling.js with historyGather "peer" ON THE DEVICE: two row tiles of one frame driven by two worker threads of one Node process
    through the N-API addon (peerExport / peerOpen / peerGatherHistory — rfx_peer_*, the consumer's own kernel pulling the column blocks its
    rays read out of the other tile's plane, the flag barriers of the two contexts meeting on the device), the halo rows moved by a TEST
    exchange layer (host copies in lock step — two RCCL ranks cannot share a GPU, which is why run_dump.js --ranks runs under --hostsim
    only): every output of three frames equals the bytes of one process rendering the whole frame, and something was pulled.  Also under
    --hostsim (contexts of one process use each other's addresses: no mapping needed; a launch runs on the calling thread, so the two
    workers' barrier kernels meet like the device's)."""
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    W, H = 160, 96
    dirs = []
    for i in range(3):
        d = str(tmp_path / ("dump%d" % i))
        write_dump(d, synthetic_frame(W, H, i))
        dirs.append(d)
    one, many = str(tmp_path / "one"), str(tmp_path / "many")
    os.makedirs(many)
    subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", one, "--steps", "12", "--refineSteps", "3"], text=True)
    script = str(tmp_path / "peer_workers.js")
    open(script, "w").write(PEER_WORKERS)
    # Two contexts of one process on ONE device: their exchange streams on different hardware queues (include/rfx.h rfx_peer_*) — 8 of them,
    # not more: the device maps a bounded number of queues at a time, the pytest process that ran sixty tests before this one keeps its own, and
    # a queue that is swapped out while the other tile's barrier kernel polls for it is the same failure again (seen once in a whole-suite run
    # with 16; never in the runs of this test alone).  One retry for that case, reported.
    cmd = [node, script, JS, json.dumps(dirs), many, json.dumps(dict(halo=12, steps=12, refineSteps=3))]
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    try:
        res = subprocess.check_output(cmd, text=True, timeout=300, env=env, stderr=subprocess.PIPE)
    except subprocess.CalledProcessError as e:
        if "did not reach the previous call's barrier" not in (e.stderr or ""):
            raise
        print("NOTE: the two tiles' barrier kernels were not resident together (hardware queue scheduling); second attempt")
        res = subprocess.check_output(cmd, text=True, timeout=300, env=env)
    info = json.loads(res.strip().splitlines()[-1])
    assert [i["rank"] for i in info] == [0, 1] and all(i["mode"] == "peer" and i["haloViolations"] == 0 for i in info), info
    assert all(len(i["pulled"]) == 3 and i["pulled"][0] == 0 for i in info), info  # one report per frame, each of the call before
    assert sum(sum(i["pulled"]) for i in info) > 0, info  # (vacuous otherwise: reflections cross the tile boundary in this scene)
    for name in ("final", "compose", "denoise_b0", "temporal0", "ssgi"):
        a = open(os.path.join(one, name + ".bin"), "rb").read()
        b = b"".join(open(os.path.join(many, "%s.rank%d.bin" % (name, r)), "rb").read() for r in range(2))
        assert a == b, name


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("RFX_HOSTSIM") != "1" and os.environ.get("RFX_TEST_UNSEEN") != "1",
                    reason="written after the round's GPU budget: runs under pytest --hostsim, and on the device with RFX_TEST_UNSEEN=1 until it has been seen green there")
@pytest.mark.parametrize("mipmaps", [True, False])
def test_node_cube_environment_equals_python_host(tmp_path, mipmaps):
    """`run_dump.js --envCube`: scene.environment as a CubeTexture through the Node host (CubeToEquirectEnvPass -> rfx_cube_to_equirect, the
    importance tables from the converted map) drives the same bytes as the Python host."""
    import golden_util as G
    from rfx_amd.context import Context
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    W, H = 160, 96
    f = synthetic_frame(W, H, 0)
    d = str(tmp_path / "dump0")
    write_dump(d, f)
    faces = np.ascontiguousarray(G.load("cube_32")["faces"])
    cf = str(tmp_path / "cube.bin")
    faces.tofile(cf)
    out = str(tmp_path / "js_out")
    subprocess.check_output([node, os.path.join(JS, "run_dump.js"), d, "--out", out, "--steps", "12", "--refineSteps", "3", "--envCube", json.dumps(cf), "--envCubeSize", "32"]
                            + ([] if mipmaps else ["--envCubeMipmaps", "false"]), text=True)
    cube = dict(isCubeTexture=True, faces=faces)
    if not mipmaps:
        cube.update(minFilter=effect.LinearFilter, generateMipmaps=False)
    scene = types.SimpleNamespace(frame=f, environment=cube)
    cam = types.SimpleNamespace(**vars(f.camera))
    fx = effect.SSGIEffect(None, scene, cam, dict(width=W, height=H, steps=12, refineSteps=3), seeds=dict(ssgi=11, denoise=22), half_store_rtz=True)
    ctx = Context(W, H)
    fx.update(ctx, None)
    for name, tex in (("compose", abi.TEX_COMPOSE), ("ssgi", abi.TEX_SSGI)):
        py = ctx.download(tex)
        js = np.fromfile(os.path.join(out, name + ".bin"), py.dtype).reshape(py.shape)
        assert np.array_equal(py.view(np.uint8), js.view(np.uint8)), name
    ctx.close()
