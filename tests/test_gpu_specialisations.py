"""-m gpu: every kernel specialisation the launchers can select (realism-effects_amd/csrc/rfx_launch.h: a run-time option becomes a template
argument), one test per kernel, the test's id the kernel's key (tests/specialisations.py): 54 k1_ssgi_march, 24 k2_temporal_reproject, 4 k3_generic
+ 40 k3_tiled, every (pitch, skip) layout of k3_tiled's staged rectangle, and 3 k0_aov_pack.  Each case is the device against the C restatement on identical
inputs through assert_close of tests/test_gpu_parity.py — its metric, its bounds, every out-of-tolerance pixel proven — or, where the
specialisation differs from one held that way only in how the work is cut (trace + shade for march, row tiles for the whole frame),
bit-identical to that one.  tests/test_specialisation_cases.py (CPU) holds the tables below against the full cross products: a template
argument added to a launcher fails there until a case exists here.

The frames are the smallest at which the specialisation exists (the cases also run thread by thread under --hostsim); every test asserts,
from the plans of the loaded library, that its inputs select the kernel it is named after."""
import functools

import numpy as np
import pytest

import specialisations as SP

pytestmark = pytest.mark.gpu

STEPS, REFINE = 12, 3
ORTHO_HALF_HEIGHT = 3.2   # the orthographic camera of test_orthographic_camera_vs_oracle
JITTER_FRAME = 5          # TRAAEffect's view offset of that frame (rfx_amd.effect.r2Sequence): (0.387, 0.462) pixel

# ---------------------------------------------------------------- K1
# pow2 1: every 16:9 frame.  pow2 0: the smallest frames that keep plain rows are 9232 rows high (W <= 256: a padded row holds 16 cells, and
# 16 x 577 cells exceed the 9216-cell table).  The draw is restricted to K1_WINDOW there (rfx_set_row_window) and the restatement to the same
# rows: a band in the middle of the table's rows whose rays hit and read the history; its first row is no multiple of the tile height.
K1_FRAME = {1: (96, 54), 0: (32, 9232)}
K1_WINDOW = (4603, 4699)
K1_CASES = list(SP.K1_KEYS)


def k1_camera(proj, W, H):
    """the synthetic camera of frame 1 (centred), the same with a TRAA view offset (perspective), the orthographic one (general)"""
    from rfx_amd.effect import r2Sequence
    from rfx_amd.scene import Camera
    cam = Camera.orbit(1, W / H, ortho_half_height=ORTHO_HALF_HEIGHT if proj == "general" else None)
    if proj == "perspective":
        cam = SP.view_offset_camera(cam, W, H, *r2Sequence[JITTER_FRAME])
    return cam


def k1_inputs(key):
    """(SsgiParams, W, H, entry point) of a K1 case: what the CPU test derives the key from and the device test draws with"""
    from rfx_amd import abi
    _, proj, pow2, em, stage = key
    W, H = K1_FRAME[pow2]
    sp = abi.SsgiParams(camera=abi.Camera.from_scene(k1_camera(proj, W, H)), steps=STEPS, refineSteps=REFINE, mode=0, useDirectLight=1, missedRays=0,
                        importanceSampling=int(em == 2), useEnvMap=int(em >= 1), rayDistance=10, thickness=10, envBlur=0.5, blueNoiseIndex=77)
    return sp, W, H, stage


# ---------------------------------------------------------------- K2
K2_FRAME = (96, 54)
K2_CASES = list(SP.K2_KEYS)


def k2_inputs(key):
    """(TemporalParams, whole) of a K2 case.  inputType 0: SSGIEffect's pass (two textures), 1: TRAAEffect's (the raw texel), 2: SSREffect's"""
    from rfx_amd import abi
    from rfx_amd.scene import Camera
    _, it, lt, hf, wh = key
    W, H = K2_FRAME
    cam, prev = (abi.Camera.from_scene(Camera.orbit(fi, W / H)) for fi in (1, 0))
    tp = abi.TemporalParams(camera=cam, prevCamera=prev, textureCount=2 if it == 0 else 1, inputType=it, logTransform=lt, fullAccumulate=0,
                            confidencePower=4 if it == 1 else 0.75, neighborhoodClampIntensity=1 if it == 1 else 0.5, maxBlend=0.9 if it == 1 else 1.0,
                            keepData=1.0, historySource=2 if hf else 0)
    tp.reprojectSpecular[:] = ([0, 1], [0, 0], [1, 1])[it]
    tp.neighborhoodClamp[:] = ([0, 1], [1, 1], [1, 1])[it]
    return tp, bool(wh)


# ---------------------------------------------------------------- K3
# (W, H, radius) per (IN_T, TC, pitch), from the plan (pitch 0: k3_generic): H = 24, the narrowest frames are narrower than one 64-texel tile
K3_FRAME = {
    (0, 1, 0): (40, 24, 7.0), (0, 2, 0): (40, 24, 7.0), (1, 1, 0): (40, 24, 6.0), (1, 2, 0): (40, 24, 6.0),
    (0, 1, 72): (40, 24, 2.0), (0, 1, 74): (40, 24, 2.5), (0, 1, 76): (40, 24, 3.0), (0, 1, 80): (40, 24, 4.0), (0, 1, 96): (40, 24, 5.0),
    (0, 2, 72): (40, 24, 2.0), (0, 2, 74): (40, 24, 2.5), (0, 2, 76): (40, 24, 3.0), (0, 2, 80): (40, 24, 4.0), (0, 2, 96): (40, 24, 5.0),
    (1, 1, 72): (40, 24, 2.5), (1, 1, 74): (40, 24, 2.75), (1, 1, 76): (40, 24, 3.5), (1, 1, 80): (40, 24, 4.0), (1, 1, 96): (51, 24, 4.0),
    (1, 2, 72): (40, 24, 2.5), (1, 2, 74): (40, 24, 3.0), (1, 2, 76): (40, 24, 3.5), (1, 2, 80): (40, 24, 4.0), (1, 2, 96): (51, 24, 4.0),
}
# one more case per pitch on a frame with an interior tile column (three tile columns: 132 texels)
K3_WIDE = [
    (("k3_tiled", 0, 2, 72, 1), (132, 24, 0.5)), (("k3_tiled", 0, 2, 74, 1), (132, 24, 0.75)), (("k3_tiled", 0, 2, 76, 1), (132, 24, 1.0)),
    (("k3_tiled", 0, 2, 80, 1), (132, 24, 1.25)), (("k3_tiled", 0, 2, 96, 1), (132, 24, 1.5)),
    (("k3_tiled", 1, 2, 72, 1), (132, 24, 0.75)), (("k3_tiled", 1, 2, 76, 1), (132, 24, 1.0)), (("k3_tiled", 1, 2, 80, 1), (132, 24, 1.25)),
    (("k3_tiled", 1, 2, 96, 1), (132, 24, 1.75)),
]
# (key, (W, H, radius), tag); tag "tiles": k3_generic has no template argument for a row tile, but it rebases rows there all the same
K3_CASES = ([(k, K3_FRAME[(k[1], k[2], k[3] if k[0] == "k3_tiled" else 0)], "") for k in SP.K3_KEYS] + [(k, f, "wide") for k, f in K3_WIDE] +
            [(k, K3_FRAME[(k[1], k[2], 0)], "tiles") for k in SP.K3_GENERIC_KEYS])
# the (pitch, skip) layouts of pass 0's staged rectangle (two textures, whole frame): every pair the sweep SP.LAYOUT_SWEEP selects
K3_LAYOUT_CASES = [
    (("layout", 72, 0), (40, 24, 0.0)), (("layout", 72, 2), (42, 24, 2.0)), (("layout", 72, 4), (40, 24, 2.5)),
    (("layout", 74, 0), (50, 24, 2.25)), (("layout", 74, 2), (40, 24, 3.0)), (("layout", 74, 4), (44, 24, 2.5)),
    (("layout", 76, 0), (132, 24, 1.0)), (("layout", 76, 2), (44, 24, 3.0)), (("layout", 76, 4), (40, 24, 3.5)),
    (("layout", 80, 0), (40, 24, 4.0)), (("layout", 80, 2), (65, 24, 3.0)), (("layout", 80, 4), (40, 24, 5.0)),
    (("layout", 96, 0), (51, 24, 4.0)), (("layout", 96, 2), (140, 9, 1.0)), (("layout", 96, 4), (93, 24, 4.0)),
]


def k3_inputs(key, frame, tag=""):
    """(DenoiseParams, W, H, whole) of a K3 case: pass 0 (IN_T 1) reads K2's targets and writes A, a later pass (IN_T 0) reads A and writes B"""
    from rfx_amd import abi
    W, H, radius = frame
    in_t, tc, wh = (1, 2, 1) if key[0] == "layout" else (key[1], key[2], key[4] if key[0] == "k3_tiled" else int(tag != "tiles"))
    dp = abi.DenoiseParams(radius=radius, phi=0.5, lumaPhi=5, depthPhi=2, normalPhi=50, roughnessPhi=50, specularPhi=50, textureCount=tc,
                           blueNoiseIndex=31, inputIsTemporal=in_t, writeToB=0 if in_t else 1, halfStoreRTZ=1)
    dp.isTextureSpecular[:] = [0, 1] if tc == 2 else [0, 0]
    return dp, W, H, bool(wh)


# ---------------------------------------------------------------- K0 AOV pack
K0_AOV_CASES = list(SP.K0_AOV_KEYS)


def k0_aov_inputs(key):
    """the staged planes of a K0 AOV pack case: the 7 x 3 frame of tests/aov_cases.py (five groups and a tail) all float32, as the typed set, all halves"""
    import aov_cases as AC
    return AC.stage(AC.form_frame(0), {0: 0, 1: AC.TYPED, 2: AC.ALL}[key[1]])


# ---------------------------------------------------------------- shared by the tests
@functools.lru_cache(maxsize=None)
def _plans():
    from rfx_amd import abi
    return SP.Plans(abi.load_library())


@functools.lru_cache(maxsize=None)
def _frame(W, H, fi, ortho=False):
    """a synthetic frame, rendered once (the tests only read it)"""
    from rfx_amd.scene import synthetic_frame
    return synthetic_frame(W, H, fi, ortho_half_height=ORTHO_HALF_HEIGHT if ortho else None)


@functools.lru_cache(maxsize=None)
def _environment():
    """the environment image, the restatement's mip chain of it and the importance tables"""
    from rfx_amd.envmap import build_importance
    from rfx_amd.scene import synthetic_environment
    import rfx_oracle as O
    img = synthetic_environment(128, 64)
    plain, mis = O.EnvMap(img, half=True, rtz=True), O.EnvMap(img, half=True, rtz=True)
    tables = build_importance(mis.level(0))
    mis.set_importance(*tables)
    return img, plain, mis, tables


def _h8(o):
    import rfx_oracle as O
    return O.half_bits_to_float(np.ascontiguousarray(o).view(np.uint16))


def _two_tiles(W, H, halo):
    from test_gpu_parity import _LocalTiles
    return _LocalTiles(W, H, 2, halo)


def _close_all(*ctxs):
    for c in ctxs:
        for x in getattr(c, "ctxs", [c]):
            assert x.halo_violations() == 0
            x.close()


# ---------------------------------------------------------------- K1
@pytest.mark.parametrize("key", K1_CASES, ids=SP.key_id)
def test_k1(blue_noise, key):
    """march: the device against the restatement, every out-of-tolerance pixel proven.  trace / shade: the two halves leave exactly the texels
    the march leaves — the trace while the history slot holds junk (it may not read it), the shade with ANOTHER history than the trace saw
    (it must read the slot as it is then)."""
    from rfx_amd import abi
    from rfx_amd.context import Context
    from test_gpu_parity import FLIP, FLIP_ENV, assert_close
    import rfx_oracle as O
    _, proj, pow2, em, stage = key
    sp, W, H, entry = k1_inputs(key)
    assert SP.k1_key(_plans(), sp, W, H, entry) == key and _plans().k1(W, H)["pow2"] == pow2
    f = _frame(W, H, 1, proj == "general")
    assert np.array_equal(f.camera.matrixWorld, k1_camera(proj, W, H).matrixWorld)  # the planes are this camera's (but for the sub-pixel view offset)
    win = None if pow2 else K1_WINDOW
    y0, y1 = win or (0, H)
    rs = np.random.RandomState(4)
    comp, comp2 = rs.rand(H, W, 4).astype(np.float32), rs.rand(H, W, 4).astype(np.float32)
    img, env_plain, env_mis, tables = _environment() if em else (None, None, None, None)
    env = (None, env_plain, env_mis)[em]
    ctx = Context(W, H)
    if em:
        ctx.set_environment(img, half_float_type=True, half_store_rtz=True)
    if em == 2:
        ctx.set_environment_importance(*tables)
    ctx.upload_frame(f)
    if win:
        ctx.set_row_window(*win)

    def march(history):
        ctx.clear(abi.TEX_SSGI)
        ctx.upload(abi.TEX_COMPOSE, history)
        ctx.ssgi_march(sp)
        return ctx.download(abi.TEX_SSGI)

    got = march(comp)
    assert (got[y0:y1] != 0).any() and not got[:y0].any() and not got[y1:].any(), "the draw wrote nothing, or outside its row window"
    if stage == "march":
        oracle = lambda: O.ssgi(f.depth, f.gbuffer, f.direct, comp, blue_noise, sp, rows=(y0, y1), env=env)  # noqa: E731
        want = oracle()
        # (whole-frame arrays: the proofs re-run the restatement under a frame-sized pixel mask; rows outside the window are zero on both sides)
        bound = FLIP_ENV if em else FLIP["ssgi"]
        frac, _ = assert_close(SP.key_id(key), _h8(got), _h8(want), bound, prove=lambda: _h8(oracle()))
        bad, pixels = round(frac * H * W), (y1 - y0) * W
        assert bad <= float(bound) * pixels + 2, "%d of the %d drawn pixels outside the metric (bound %.4f%% + 2)" % (bad, pixels, 100 * float(bound))
        if em:  # the environment contributes
            sp.useEnvMap = sp.importanceSampling = 0
            assert (march(comp)[y0:y1] != got[y0:y1]).any(axis=-1).mean() > 0.05
    else:
        seen = comp if stage == "trace" else comp2  # what the shade must read
        want = got if stage == "trace" else march(comp2)
        assert (want != got).any() or stage == "trace", "the history does not reach the output: the case would be vacuous"
        ctx.clear(abi.TEX_SSGI)
        ctx.upload(abi.TEX_COMPOSE, np.full((H, W, 4), 1e6, np.float32) if stage == "trace" else comp)
        ctx.ssgi_trace(sp)
        ctx.upload(abi.TEX_COMPOSE, seen)
        ctx.ssgi_shade(sp)
        out = ctx.download(abi.TEX_SSGI)
        assert np.array_equal(out, want), "%s: %.4f%% texels differ from the march" % (SP.key_id(key), 100 * (out != want).any(axis=-1).mean())
    _close_all(ctx)


# ---------------------------------------------------------------- K2
def _spice_halfs(h, rs, n):
    """zero, the smallest subnormal and two very small halfs in the colour channels of n random texels of an (H, W, 4) plane of half bits"""
    H, W = h.shape[:2]
    tiny = np.array([0x0000, 0x0001, 0x0100, 0x068e], np.uint16)  # 0, 6e-8, 1.5e-5, 1.0002e-4 (a K1 texel stores radiance + 1e-4)
    ys, xs = rs.randint(0, H, n), rs.randint(0, W, n)
    h[ys, xs, :3] = tiny[rs.randint(0, 4, (n, 3))]
    return h


@functools.lru_cache(maxsize=None)
def _k2_planes(it, hf):
    """the inputs of a K2 case, shared by its logTransform and whole / tiled variants: frame 1's velocity, the input texels (inputType 0 / 2: the
    restatement's K1 output in mode "ssgi" / "ssr", 1: the composer's buffer) and the history, with zero and very small radiance in all of them
    — what logTransform 0 passes through unchanged and logTransform 1 takes the logarithm of"""
    from rfx_amd import abi
    from rfx_amd.context import load_blue_noise_table
    import rfx_oracle as O
    W, H = K2_FRAME
    f = _frame(W, H, 1)
    rs = np.random.RandomState(10 + it)
    n = W * H // 6
    if it == 1:
        raw = f.direct.copy()
        ys, xs = rs.randint(0, H, n), rs.randint(0, W, n)
        raw[ys, xs, :3] = np.array([0.0, 1e-30, 1e-7, 3e-5], np.float32)[rs.randint(0, 4, (n, 3))]
        raw[rs.randint(0, H, 40), rs.randint(0, W, 40), 0] = -1.0  # "not sampled" texels (temporal_reproject.frag:124-145)
        inp = np.ascontiguousarray(raw).view(np.uint32)
    else:
        sp = abi.SsgiParams(camera=abi.Camera.from_scene(f.camera), steps=8, refineSteps=2, mode=0 if it == 0 else 1, useDirectLight=1, rayDistance=10,
                            thickness=10, envBlur=0.5, blueNoiseIndex=50)
        packed = O.ssgi(f.depth, f.gbuffer, f.direct, rs.rand(H, W, 4).astype(np.float32), load_blue_noise_table(), sp)
        halfs = np.ascontiguousarray(packed).view(np.uint16).reshape(H, W, 2, 4)  # the packed texel: two vec4s of halfs (unpackTwoVec4)
        for k in range(2):
            halfs[:, :, k] = _spice_halfs(halfs[:, :, k].copy(), rs, n)
        inp = halfs.reshape(H, W, 8).view(np.uint32)
    scale = np.array([1, 1, 1, 6], np.float32)
    if hf:  # what rfx_copy_framebuffer copies into the Float target
        hist = [(rs.rand(H, W, 4).astype(np.float32) * scale)]
        ys, xs = rs.randint(0, H, n), rs.randint(0, W, n)
        hist[0][ys, xs, :3] = np.array([0.0, 1e-30, 1e-12, 3e-5], np.float32)[rs.randint(0, 4, (n, 3))]
    else:
        hist = [_spice_halfs((rs.rand(H, W, 4).astype(np.float32) * scale).astype(np.float16).view(np.uint16), rs, n) for _ in range(2 if it == 0 else 1)]
    for a in [inp] + hist:
        a.setflags(write=False)
    return f, inp, hist


def _k2_draw(r, tp, f, inp, hist):
    """upload, (copy the history into the Float target,) draw; r: a Context or _LocalTiles.  Returns the targets."""
    from rfx_amd import abi
    H, W = f.depth.shape
    texs = SP.k2_textures(abi, tp)
    r.upload(abi.TEX_VELOCITY, f.velocity)
    r.upload(abi.TEX_SSGI, inp)
    if tp.historySource == 2:
        r.upload(abi.TEX_TEMPORAL0, hist[0])
        r.copy_framebuffer(abi.TEX_FBCOPY_F32)
        if hasattr(r, "after_copy_framebuffer"):
            r.after_copy_framebuffer(abi.TEX_FBCOPY_F32)
    else:
        for t, h in zip(texs[2:4], hist):
            r.upload(t, h)
    for t in set(texs[4:6]):
        r.upload(t, np.zeros((H, W, 4), np.float32))
    r.temporal_reproject(tp)
    return [r.download(t) for t in texs[4:4 + tp.textureCount]]


@pytest.mark.parametrize("key", K2_CASES, ids=SP.key_id)
def test_k2(key):
    """whole 1: the device against the restatement, every out-of-tolerance pixel proven.  whole 0: the frame drawn as two row tiles with
    host-staged halos is bit-identical to the whole-frame draw."""
    from rfx_amd import abi, tiling
    from rfx_amd.context import Context
    from test_gpu_parity import FLIP, assert_close
    import rfx_oracle as O
    _, it, lt, hf, wh = key
    tp, whole = k2_inputs(key)
    W, H = K2_FRAME
    f, inp, hist = _k2_planes(it, hf)
    assert np.array_equal(abi.Camera.from_scene(f.camera).projectionMatrix[:], tp.camera.projectionMatrix[:])
    texs = SP.k2_textures(abi, tp)
    ctx = Context(W, H)
    assert SP.k2_key(tp, SP.views_whole(H, [ctx.held_rows(t) for t in texs])) == key[:4] + (1,)
    got = _k2_draw(ctx, tp, f, inp, hist)
    if hf:
        assert np.array_equal(ctx.download(abi.TEX_FBCOPY_F32).view(np.uint32), hist[0].view(np.uint32))
    if whole:
        h = [hist[0], hist[-1]]

        def oracle():
            out = [np.zeros((H, W, 4), np.float32) for _ in range(tp.textureCount)]
            O.temporal(inp, f.velocity, h[0], h[1], tp, out[0], out[1] if tp.textureCount == 2 else None)
            return out
        want = oracle()
        for j in range(tp.textureCount):
            assert_close("%s [%d]" % (SP.key_id(key), j), got[j], want[j], FLIP["temporal"], prove=lambda j=j: oracle()[j])
            assert (got[j] != 0).any(axis=-1).mean() > 0.5
    else:
        vmax = float(np.abs(f.velocity[..., 1].view(np.float32)).max())
        tiles = _two_tiles(W, H, tiling.required_halo(0.0, vmax, H, W))
        for c in tiles.ctxs:
            assert SP.k2_key(tp, SP.views_whole(H, [c.held_rows(t) for t in texs])) == key
        out = _k2_draw(tiles, tp, f, inp, hist)
        for j in range(tp.textureCount):
            assert np.array_equal(out[j].view(np.uint32), got[j].view(np.uint32)), "%s [%d]: the row tiles differ from the whole frame" % (SP.key_id(key), j)
        _close_all(tiles)
    _close_all(ctx)


# ---------------------------------------------------------------- K3
def _k3_draw(r, dp, f, ins, init):
    from rfx_amd import abi
    texs = SP.k3_textures(abi, dp)
    r.upload(abi.TEX_DEPTH, f.depth)
    r.upload(abi.TEX_GBUFFER, f.gbuffer)
    for t, a in list(zip(texs[2:4], ins)) + list(zip(texs[4:6], init)):
        r.upload(t, a)
    r.poisson_denoise(dp)
    return [r.download(t) for t in texs[4:4 + dp.textureCount]]


def _k3_case(blue, name, dp, W, H, whole, want_key, want_layout=None):
    """both half-store roundings (and, with one texture, isTextureSpecular both ways) of one draw: whole frame -> against the restatement;
    two row tiles -> bit-identical to the whole frame"""
    from rfx_amd import abi, tiling
    from rfx_amd.context import Context
    from test_gpu_parity import FLIP, assert_close
    import rfx_oracle as O
    f = _frame(W, H, 0)
    assert (f.depth == 1.0).any() and (f.depth < 1.0).mean() > 0.5  # (background texels: discarded, they keep what the target held)
    tc = dp.textureCount
    texs = SP.k3_textures(abi, dp)
    rs = np.random.RandomState(3)
    planes = [rs.rand(H, W, 4).astype(np.float32) * np.array([2, 2, 2, 6], np.float32) for _ in range(2)]  # random finite planes
    ins = planes if dp.inputIsTemporal else [p.astype(np.float16).view(np.uint16) for p in planes]
    init = [(rs.rand(H, W, 4) * 3).astype(np.float16).view(np.uint16) for _ in range(2)]
    ctx = Context(W, H)
    assert SP.k3_key(_plans(), dp, W, H, SP.views_whole(H, [ctx.held_rows(t) for t in texs])) == (want_key[:4] + (1,) if want_key[0] == "k3_tiled" else want_key)
    if want_layout is not None:
        assert SP.k3_layout(_plans(), dp, W, H) == want_layout
    tiles = None
    if not whole:
        halo = tiling.required_halo(dp.radius, 0.0, H, W)
        tiles = _two_tiles(W, H, halo)
        for c in tiles.ctxs:
            held = [c.held_rows(t) for t in texs]
            assert not SP.views_whole(H, held) and SP.k3_key(_plans(), dp, W, H, SP.views_whole(H, held)) == want_key
    for spec in ([0, 1],) if tc == 2 else ([0, 0], [1, 1]):
        dp.isTextureSpecular[:] = spec
        for rtz in (1, 0):
            dp.halfStoreRTZ = rtz
            got = _k3_draw(ctx, dp, f, ins, init)
            tag = "%s spec=%d rtz=%d" % (name, spec[0], rtz)
            if whole:
                def oracle():
                    out = [a.copy() for a in init]
                    O.denoise(f.depth, f.gbuffer, ins[0], ins[1] if tc == 2 else ins[0], blue, dp, out[0], out[1] if tc == 2 else None)
                    return out
                want = oracle()
                for j in range(tc):
                    assert_close("%s [%d]" % (tag, j), _h8(got[j]), _h8(want[j]), FLIP["denoise"], prove=lambda j=j: _h8(oracle()[j]))
                    kept = (got[j] == init[j]).all(-1)
                    assert np.array_equal(kept, (want[j] == init[j]).all(-1)) and kept.any() and not kept.all(), "%s: the discarded texels" % tag
            else:
                out = _k3_draw(tiles, dp, f, ins, init)
                for j in range(tc):
                    assert np.array_equal(out[j], got[j]), "%s [%d]: the row tiles differ from the whole frame" % (tag, j)
    _close_all(ctx, *([tiles] if tiles else []))


@pytest.mark.parametrize("key,frame,tag", K3_CASES, ids=[SP.key_id(k) + ("-" + tag if tag else "") for k, _, tag in K3_CASES])
def test_k3(blue_noise, key, frame, tag):
    dp, W, H, whole = k3_inputs(key, frame, tag)
    _k3_case(blue_noise, SP.key_id(key), dp, W, H, whole, key)


@pytest.mark.parametrize("key,frame", K3_LAYOUT_CASES, ids=[SP.key_id(k) for k, _ in K3_LAYOUT_CASES])
def test_k3_pass0_layout(blue_noise, key, frame):
    """pass 0 with two textures: `skip` texels shaved off each end of the staged rectangle, on every pitch"""
    dp, W, H, whole = k3_inputs(key, frame)
    _k3_case(blue_noise, SP.key_id(key), dp, W, H, whole, ("k3_tiled", 1, 2, key[1], 1), want_layout=key)


# ---------------------------------------------------------------- K0 AOV pack
@pytest.mark.parametrize("key", K0_AOV_CASES, ids=SP.key_id)
def test_k0_aov(key):
    """the staged frame's four slots against the C restatement's packers on the widened planes, byte for byte"""
    from rfx_amd import abi
    from rfx_amd.context import Context
    import aov_cases as AC
    staged = k0_aov_inputs(key)
    assert SP.k0_aov_key(staged) == key
    ctx = Context(AC.FORM_W, AC.FORM_H)
    ctx.stage_aov(staged)
    ctx.stage_flip()
    got = [ctx.download(t) for t in (abi.TEX_DEPTH, abi.TEX_GBUFFER, abi.TEX_VELOCITY, abi.TEX_DIRECT_LIGHT)]
    diff = AC.differing(got, AC.reference(AC.widen(staged)))
    assert not diff, "%s: %s" % (SP.key_id(key), diff)
    _close_all(ctx)
