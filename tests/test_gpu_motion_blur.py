"""GPU (-m gpu; also under --hostsim): K6, MotionBlurEffect (rfx_motion_blur).  The kernel against the reference's own GLSL on llvmpipe
(the committed fixtures tests/golden/motion_blur_*.npz) and against the numpy restatement (tests/motion_blur_ref.py) on seeded random
cases; row windows and on-device chaining bit for bit; the TRAA (README) form; error codes; the per-draw profile."""
import os

import numpy as np
import pytest

import motion_blur_ref as R
from rfx_amd import abi, effect
from rfx_amd.context import Context, RfxError, load_blue_noise_table

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOSTSIM = bool(os.environ.get("RFX_HOSTSIM"))
BOUND = 1e-4
# the kernel's bit-identical share against the reference GLSL under RFX_UV_REFERENCE_GL as measured on an MI355X, less 0.002: lowest of the
# six float-fixture draws 0.9892; option cases 0.9952 0.9993 1.0 0.9728 1.0 (the numpy restatement's shares exactly).  A lowering of `mix`
# or of the sampler's lerps that differs from llvmpipe's drops them by 0.05-0.5 (tools/probe_motion_blur_gl.py)
FLOAT_FLOOR = 0.987
CASE_FLOORS = (0.993, 0.997, 0.998, 0.970, 0.998)


def _vel4(v):
    return np.concatenate([v, np.zeros(v.shape[:2] + (2,), np.float32)], -1).astype(np.float32)


def _params(source=abi.TEX_EFFECT_INPUT, center=-1, alpha_one=0, samples=16, intensity=1.0, jitter=1.0, deltaTime=1 / 60, frame=0,
            resolution=None, half=0, rtz=1, W=1, H=1):
    p = abi.MotionBlurParams()
    p.source, p.center, p.centerAlphaOne, p.samples = source, center, alpha_one, samples
    p.intensity, p.jitter, p.deltaTime, p.frame = intensity, jitter, max(1 / 1000, deltaTime), frame
    p.resolution[:] = list(resolution or (W, H))
    p.targetHalf, p.halfStoreRTZ = half, rtz
    return p


def _within(got, ref):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert (np.isnan(got) == np.isnan(ref)).all()
    ok = np.isnan(ref) | (np.abs(got - ref) <= BOUND * np.maximum(1.0, np.abs(ref)))
    assert ok.all(), (np.nanmax(np.abs(got - ref)), np.argwhere(~ok)[:5])


def _halfs_adjacent(got, ref):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    g16, r16 = got.astype(np.float16).view(np.int16).astype(np.int64), ref.astype(np.float16).view(np.int16).astype(np.int64)
    assert ((np.abs(g16 - r16) <= 1) | (np.abs(got - ref) <= BOUND * np.maximum(1.0, np.abs(ref)))).all()


def _ctx(W, H, uv_model="reference_gl"):
    c = Context(W, H)
    c.set_uv_model(uv_model)
    return c


def _draw(ctx, velocity, source, p, center=None, center_slot=None):
    ctx.upload(abi.TEX_VELOCITY, _vel4(velocity[..., :2]))
    ctx.upload(p.source, np.ascontiguousarray(source, np.float32))
    if center is not None:
        ctx.upload(center_slot, np.ascontiguousarray(center, np.float32))
    ctx.motion_blur(p)
    return ctx.download(abi.TEX_MOTION_BLUR)


@pytest.mark.parametrize("uv_model", ["reference_gl", "ideal"])
def test_kernel_vs_reference_glsl_fixtures(uv_model):
    bn = load_blue_noise_table()
    g = np.load(os.path.join(GOLDEN, "motion_blur_float_97x55.npz"))
    W, H = int(g["width"]), int(g["height"])
    ctx = _ctx(W, H, uv_model)
    exact = []
    for fi, f in enumerate(g["frames"]):
        for di, dt in enumerate(g["deltaTimes"]):
            got = _draw(ctx, g["velocity"], g["source"], _params(frame=int(f), deltaTime=float(dt), W=W, H=H))
            _within(got, g["outputs"][fi, di])
            exact.append((got == g["outputs"][fi, di]).mean())
            _within(got, R.motion_blur(_vel4(g["velocity"]), g["source"], blue_noise=bn, frame=int(f), deltaTime=float(dt), uv_model=uv_model))
    if uv_model == "reference_gl":
        assert min(exact) >= FLOAT_FLOOR, exact
    ctx.close()
    g = np.load(os.path.join(GOLDEN, "motion_blur_cases_128x72.npz"))
    W, H = int(g["width"]), int(g["height"])
    ctx = _ctx(W, H, uv_model)
    for k, (c, ref) in enumerate(zip(g["cases"], g["outputs_rgb"])):
        s, i, j, rx, ry, f, dt = c
        got = _draw(ctx, g["velocity"], g["source"], _params(samples=int(s), intensity=i, jitter=j, resolution=(rx, ry), frame=int(f), deltaTime=dt))
        _within(got[..., :3], ref)
        if uv_model == "reference_gl":
            share = (got[..., :3] == ref).mean()
            assert share >= CASE_FLOORS[k], (k, share)
    ctx.close()
    g = np.load(os.path.join(GOLDEN, "motion_blur_half_96x54.npz"))
    W, H = int(g["width"]), int(g["height"])
    ctx = _ctx(W, H, uv_model)
    src, acc = g["source"].astype(np.float32), g["accumulated"].astype(np.float32)
    for k, c in enumerate(g["cases"]):
        s, i, j, rx, ry, f, dt = c
        kw = dict(samples=int(s), intensity=i, jitter=j, resolution=(rx, ry), frame=int(f), deltaTime=dt, half=1)
        own = _draw(ctx, g["velocity"], src, _params(**kw))
        _halfs_adjacent(own, g["outputs_own"][k])
        traa = _draw(ctx, g["velocity"], src, _params(source=abi.TEX_SSGI, center=abi.TEX_TEMPORAL0, alpha_one=1, **kw), acc, abi.TEX_TEMPORAL0)
        _halfs_adjacent(traa, g["outputs_traa"][k])
        if uv_model == "reference_gl":
            assert (own == g["outputs_own"][k].astype(np.float32)).mean() >= 0.99
            assert (traa == g["outputs_traa"][k].astype(np.float32)).mean() >= 0.99
    ctx.close()


SIZES = [(1, 1), (2, 1), (1, 3), (5, 7), (17, 9), (33, 16), (64, 1), (63, 65), (97, 55), (130, 31)]


def _random_case(seed):
    rng = np.random.default_rng(seed)
    W, H = SIZES[seed % len(SIZES)]
    vel = rng.uniform(-0.2, 0.2, (H, W, 2)).astype(np.float32)
    kind = rng.integers(0, 10, (H, W))
    vel[kind == 0] = 0
    vel[kind == 1] = 1e-6
    vel[kind == 2] = rng.uniform(-3, 3, (int((kind == 2).sum()), 2))
    vel[kind == 3, 0] = np.nan
    vel[kind == 4] = np.inf if seed % 7 == 0 else vel[kind == 4]
    src = rng.uniform(0, 4, (H, W, 4)).astype(np.float32)
    o = dict(samples=int(rng.choice([1, 2, 7, 16, 33])), intensity=float(rng.choice([1.0, 0.0, -1.0, 3.5, 0.25])),
             jitter=float(rng.choice([0.0, 1.0, 2.5])), deltaTime=float(rng.choice([0.0, 1 / 1000, 1 / 60, 0.5, 2.0])),
             frame=int(rng.choice([0, 1, 77, 4095])), resolution=[(W, H), (1920, 1080), (3, 2), (65536, 1)][seed % 4],
             half=int(seed % 5 == 0), rtz=int(seed % 2))
    return W, H, vel, src, o


@pytest.mark.parametrize("uv_model", ["reference_gl", "ideal"])
def test_kernel_vs_restatement_random(uv_model):
    bn = load_blue_noise_table()
    for seed in range(40):
        W, H, vel, src, o = _random_case(seed)
        ctx = _ctx(W, H, uv_model)
        got = _draw(ctx, vel, src, _params(**o))
        ctx.close()
        ref = R.motion_blur(_vel4(vel), src, blue_noise=bn, samples=o["samples"], intensity=o["intensity"], jitter=o["jitter"],
                            deltaTime=max(1 / 1000, o["deltaTime"]), frame=o["frame"], resolution=o["resolution"], target_half=bool(o["half"]),
                            half_rtz=bool(o["rtz"]), uv_model=uv_model)
        (_halfs_adjacent if o["half"] else _within)(got, ref)


def test_row_windows_equal_the_whole_draw():
    W, H = 61, 47
    rng = np.random.default_rng(5)
    vel, src = rng.uniform(-0.3, 0.3, (H, W, 2)).astype(np.float32), rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
    ctx = _ctx(W, H)
    p = _params(samples=9, frame=3, W=W, H=H)
    whole = _draw(ctx, vel, src, p)
    ctx.clear(abi.TEX_MOTION_BLUR)
    for y0, y1 in ((0, 5), (5, 6), (6, 30), (30, 47)):
        ctx.set_row_window(y0, y1)
        ctx.motion_blur(p)
    ctx.set_row_window()
    assert np.array_equal(ctx.download(abi.TEX_MOTION_BLUR).view(np.uint32), whole.view(np.uint32))
    ctx.close()


def test_on_device_chaining_after_the_final_compose():
    """SSGIEffect's final image (rfx_final_compose -> RFX_TEX_FINAL) blurred on the device equals blurring the downloaded image from
    RFX_TEX_EFFECT_INPUT, bit for bit."""
    W, H = (160, 90) if HOSTSIM else (1920, 1080)
    rng = np.random.default_rng(1080)
    ctx = _ctx(W, H)
    depth = rng.uniform(0.2, 1.0, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.2] = 1.0
    ctx.upload(abi.TEX_DEPTH, depth)
    ctx.upload(abi.TEX_COMPOSE, rng.uniform(0, 3, (H, W, 4)).astype(np.float32))
    ctx.upload(abi.TEX_DIRECT_LIGHT, rng.uniform(0, 3, (H, W, 4)).astype(np.float32))
    ctx.upload(abi.TEX_VELOCITY, _vel4(rng.uniform(-0.05, 0.05, (H, W, 2)).astype(np.float32)))
    fp = abi.FinalParams()
    ctx.final_compose(fp)
    mb = effect.MotionBlurEffect(effect.VelocityDepthNormalPass(None, None), {"samples": 12})
    mb.update(ctx, abi.TEX_FINAL, 1 / 60)
    assert mb.mainImage(ctx) == abi.TEX_MOTION_BLUR
    on_device = mb.output(ctx).copy()
    final = ctx.download(abi.TEX_FINAL)
    mb.frame = 0  # the same frame as the first update
    mb.update(ctx, final, 1 / 60)
    mb.mainImage(ctx)
    assert np.array_equal(mb.output(ctx).view(np.uint32), on_device.view(np.uint32))
    assert not np.array_equal(on_device, final)
    ctx.close()


def test_traa_form_vs_restatement():
    """README form: inputColor = TRAA's NEAREST target (RFX_TEX_TEMPORAL0) with alpha 1, taps = TRAA's input plane (RFX_TEX_SSGI)."""
    W, H = 83, 41
    rng = np.random.default_rng(83)
    vel, src, acc = rng.uniform(-0.1, 0.1, (H, W, 2)).astype(np.float32), rng.uniform(0, 2, (H, W, 4)).astype(np.float32), rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
    ctx = _ctx(W, H)
    ctx.upload(abi.TEX_SSGI, src)
    ctx.upload(abi.TEX_TEMPORAL0, acc)
    ctx.upload(abi.TEX_VELOCITY, _vel4(vel))
    traa = effect.TRAAEffect(None, None, None)
    traa.uniforms["accumulatedTexture"] = abi.TEX_TEMPORAL0
    mb = effect.MotionBlurEffect(None)
    mb.shareEffectPass(traa)
    mb.frame = 9
    mb.update(ctx, None, 1 / 60)
    mb.mainImage(ctx)
    ref = R.motion_blur(_vel4(vel), src, center=acc, center_nearest=True, center_alpha_one=True, blue_noise=load_blue_noise_table(), frame=9)
    got = mb.output(ctx)
    _within(got, ref)
    assert (got[..., 3] == 1).all()
    ctx.close()


def test_traa_own_pass_output_as_the_input_buffer():
    """TRAA drawn in its own EffectPass, MotionBlurEffect in the next: the input buffer is what traa_compose.frag wrote — TEMPORAL0's rgb,
    alpha 1 — read LINEAR for inputColor and the taps alike (not TRAA's NEAREST target read as in the README form)."""
    W, H = 57, 33
    rng = np.random.default_rng(57)
    vel, acc = rng.uniform(-0.1, 0.1, (H, W, 2)).astype(np.float32), rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
    ctx = _ctx(W, H)
    ctx.upload(abi.TEX_TEMPORAL0, acc)
    ctx.upload(abi.TEX_VELOCITY, _vel4(vel))
    mb = effect.MotionBlurEffect(None)
    mb.frame = 2
    mb.update(ctx, abi.TEX_TEMPORAL0, 1 / 60)
    mb.mainImage(ctx)
    got = mb.output(ctx)
    composer = acc.copy()
    composer[..., 3] = 1  # the buffer TRAA's pass wrote
    ref = R.motion_blur(_vel4(vel), composer, blue_noise=load_blue_noise_table(), frame=2)
    _within(got, ref)
    assert (got[..., 3] == 1).all()
    ctx.close()


def test_error_codes():
    W, H = 16, 8
    ctx = _ctx(W, H)
    with pytest.raises(RfxError, match=r"\(-4\)"):  # nothing uploaded yet
        ctx.motion_blur(_params(W=W, H=H))
    ctx.download(abi.TEX_VELOCITY)  # allocates a zero-filled plane: still not uploaded
    ctx.upload(abi.TEX_EFFECT_INPUT, np.zeros((H, W, 4), np.float32))
    with pytest.raises(RfxError, match=r"\(-4\)"):
        ctx.motion_blur(_params(W=W, H=H))
    ctx.upload(abi.TEX_VELOCITY, np.zeros((H, W, 4), np.float32))
    ctx.upload(abi.TEX_EFFECT_INPUT, np.zeros((H, W, 4), np.float32))
    ctx.motion_blur(_params(W=W, H=H))
    for bad in (dict(source=abi.TEX_DEPTH), dict(source=abi.TEX_COUNT), dict(center=abi.TEX_MOTION_BLUR), dict(samples=0),
                dict(deltaTime=float("nan")), dict(deltaTime=float("inf")), dict(resolution=(0, 8)), dict(frame=-1)):
        p = _params(W=W, H=H, **{k: v for k, v in bad.items() if k != "deltaTime"})
        if "deltaTime" in bad:
            p.deltaTime = bad["deltaTime"]
        with pytest.raises(RfxError, match=r"\(-1\)"):
            ctx.motion_blur(p)
    p = _params(W=W, H=H)
    p.deltaTime = 0.0
    with pytest.raises(RfxError, match=r"\(-1\)"):
        ctx.motion_blur(p)
    with pytest.raises(RfxError, match=r"\(-4\)"):  # FINAL never drawn or uploaded
        ctx.motion_blur(_params(source=abi.TEX_FINAL, W=W, H=H))
    ctx.close()
    tiled = Context(W, H, tile_y0=0, tile_rows=4, halo_rows=2)
    tiled.upload(abi.TEX_VELOCITY, np.zeros((6, W, 4), np.float32))
    tiled.upload(abi.TEX_EFFECT_INPUT, np.zeros((6, W, 4), np.float32))
    with pytest.raises(RfxError, match=r"\(-5\)"):
        tiled.motion_blur(_params(W=W, H=H))
    tiled.close()


def test_profile_names_the_motion_blur_draw():
    W, H = 32, 16
    ctx = _ctx(W, H)
    ctx.upload(abi.TEX_VELOCITY, np.full((H, W, 4), 0.1, np.float32))
    ctx.upload(abi.TEX_EFFECT_INPUT, np.ones((H, W, 4), np.float32))
    ctx.profile(True)
    for _ in range(3):
        ctx.motion_blur(_params(W=W, H=H))
    prof = ctx.profile_read()
    ctx.profile(False)
    assert prof["k6_motion_blur"][1] == 3 and prof["k6_motion_blur"][0] >= 0
    ctx.close()
