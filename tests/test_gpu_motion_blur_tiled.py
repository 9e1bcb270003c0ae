"""GPU (-m gpu; also under --hostsim): MotionBlurEffect (K6) on ROW-TILED contexts.  rfx_motion_blur_stage copies the tile's rows of the source
into RFX_TEX_BLUR_SOURCE, rfx_motion_blur_reach_mask names the source texels the tile's draw will load, the test plays the transport (it uploads
exactly the named column blocks of the foreign rows, NaN everywhere else) and the tiled draw must equal the whole-frame context's rows bit for
bit: a texel the mask missed shows as a NaN or a wrong value, a superset is harmless.  Then how tight the mask is (bounds derived from the
streak length), the error codes, and one frame pair through CommTiledRenderer on a ring of one over the real RCCL."""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest

from rfx_amd import abi, effect, tiling
from rfx_amd.context import Context, RfxError

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HALO = 2


def _vel4(v):
    return np.concatenate([v[..., :2], np.zeros(v.shape[:2] + (2,), np.float32)], -1).astype(np.float32)


def _params(W, H, form="own", half=0, samples=16, intensity=1.0, jitter=1.0, deltaTime=1 / 60, frame=0, resolution=None):
    p = abi.MotionBlurParams()
    if form == "own":  # the effect's own EffectPass: inputColor is the LINEAR fetch of the taps' buffer
        p.source, p.center, p.centerAlphaOne = abi.TEX_EFFECT_INPUT, -1, 0
    else:  # the README form: TRAA's NEAREST target is the centre (alpha 1), its input plane the taps' buffer
        p.source, p.center, p.centerAlphaOne = abi.TEX_SSGI, abi.TEX_TEMPORAL0, 1
    p.samples, p.intensity, p.jitter, p.deltaTime, p.frame = samples, intensity, jitter, max(1 / 1000, deltaTime), frame
    p.resolution[:] = list(resolution or (W, H))
    p.targetHalf, p.halfStoreRTZ = half, 1
    return p


@functools.lru_cache(maxsize=None)
def _fixture(name):
    g = np.load(os.path.join(GOLDEN, name))
    W, H = int(g["width"]), int(g["height"])
    src = np.ascontiguousarray(g["source"], np.float32)
    centre = np.ascontiguousarray(src[::-1, ::-1] * 0.5 + 0.25, np.float32)  # TRAA's target: any plane that is not the source
    return W, H, _vel4(np.asarray(g["velocity"], np.float32)), src, centre


def _upload_inputs(ctx, p, vel, src, centre):
    for tex, plane in ((abi.TEX_VELOCITY, vel), (p.source, src)) + (((p.center, centre),) if p.center != -1 else ()):
        r0, n = ctx.held_rows(tex)
        ctx.upload(tex, plane[r0:r0 + n], r0, n)


def _key(p):
    return bytes(p)


_REFS = {}


def _reference(name, uv_model, p):
    """the whole-frame context's draw, computed once per (fixture, uv model, params) and shared"""
    k = (name, uv_model, _key(p))
    if k not in _REFS:
        W, H, vel, src, centre = _fixture(name)
        ctx = Context(W, H)
        ctx.set_uv_model(uv_model)
        _upload_inputs(ctx, p, vel, src, centre)
        ctx.motion_blur(p)
        out = ctx.download(abi.TEX_MOTION_BLUR)
        mask = ctx.motion_blur_reach_mask(p)
        ctx.close()
        out.setflags(write=False)
        mask.setflags(write=False)
        _REFS[k] = (out, mask)
    return _REFS[k]


def _column_blocks(W):
    return (np.arange(W) * 32) // W


def _play_transport(ctx, mask, src, y0, rows):
    """what a host's transport does: every foreign row with bits, its named column blocks from the whole source, every other texel NaN"""
    W = src.shape[1]
    blocks = _column_blocks(W)
    moved = 0
    for y in np.nonzero(mask)[0]:
        if y0 <= y < y0 + rows:
            continue
        row = np.full((1, W, 4), np.nan, np.float32)
        sel = ((int(mask[y]) >> blocks) & 1).astype(bool)
        row[0, sel] = src[y, sel]
        ctx.upload(abi.TEX_BLUR_SOURCE, row, int(y), 1)
        moved += int(sel.sum())
    return moved


def _tiled_draw(name, uv_model, p, world, windows=False):
    W, H, vel, src, centre = _fixture(name)
    ref, ref_mask = _reference(name, uv_model, p)
    union = np.zeros(H, np.uint32)
    for y0, rows in tiling.split_rows(H, world):
        ctx = Context(W, H, tile_y0=y0, tile_rows=rows, halo_rows=HALO)
        ctx.set_uv_model(uv_model)
        _upload_inputs(ctx, p, vel, src, centre)
        assert ctx.held_rows(abi.TEX_BLUR_SOURCE) == (0, H)
        ctx.upload(abi.TEX_BLUR_SOURCE, np.full((H, W, 4), np.nan, np.float32))
        ctx.motion_blur_stage(p)
        mask = ctx.motion_blur_reach_mask(p)
        union |= mask
        _play_transport(ctx, mask, src, y0, rows)
        ctx.motion_blur(p)
        got = ctx.download(abi.TEX_MOTION_BLUR, y0, rows)
        assert got.tobytes() == ref[y0:y0 + rows].tobytes(), "world %d tile [%d, %d): %d texels differ" % (
            world, y0, y0 + rows, int((got.view(np.uint32) != ref[y0:y0 + rows].view(np.uint32)).any(-1).sum()))
        if windows:  # arming persists: the draw in three row windows equals the draw in one
            ctx.clear(abi.TEX_MOTION_BLUR)
            a, b = y0 + 1, y0 + rows // 2 + 1
            for w0, w1 in ((y0, a), (a, b), (b, y0 + rows)):
                ctx.set_row_window(w0, w1)
                ctx.motion_blur(p)
            ctx.set_row_window()
            assert ctx.download(abi.TEX_MOTION_BLUR, y0, rows).tobytes() == got.tobytes()
        assert ctx.halo_violations() == 0
        ctx.close()
    # the same per-pixel reduction, whatever the tiling: the tiles' masks add up to the whole-frame context's
    assert np.array_equal(union, ref_mask)


FLOAT = "motion_blur_float_97x55.npz"   # static, sub-threshold, NaN and off-frame streaks, a fast block; 18 / 18 / 19 rows at three tiles
CASES = "motion_blur_cases_128x72.npz"


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("form", ["own", "traa"])
@pytest.mark.parametrize("uv_model", ["reference_gl", "ideal"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_tiled_draw_equals_the_whole_frame_rows(world, uv_model, form, half):
    g = np.load(os.path.join(GOLDEN, FLOAT))
    W, H = int(g["width"]), int(g["height"])
    assert (W, H) == (97, 55) and [r for _, r in tiling.split_rows(H, 3)] == [18, 18, 19]
    p = _params(W, H, form=form, half=half, frame=int(g["frames"][-1]), deltaTime=float(g["deltaTimes"][0]))
    _tiled_draw(FLOAT, uv_model, p, world, windows=(form == "own" and half == 0))


@pytest.mark.parametrize("world", [2, 3, 4])
def test_tiled_draw_option_cases(world):
    g = np.load(os.path.join(GOLDEN, CASES))
    W, H = int(g["width"]), int(g["height"])
    for s, i, j, rx, ry, f, dt in g["cases"]:
        p = _params(W, H, samples=int(s), intensity=float(i), jitter=float(j), resolution=(float(rx), float(ry)), frame=int(f), deltaTime=float(dt))
        _tiled_draw(CASES, "reference_gl", p, world)


# ---------------------------------------------------------------- tightness: bounds derived from the streak, not measured
def _tile_masks(W, H, vel, p, world=3):
    src = np.ones((H, W, 4), np.float32)
    out = []
    for y0, rows in tiling.split_rows(H, world):
        ctx = Context(W, H, tile_y0=y0, tile_rows=rows, halo_rows=HALO)
        _upload_inputs(ctx, p, _vel4(vel), src, src)
        out.append((y0, rows, ctx.motion_blur_reach_mask(p)))
        ctx.close()
    return out


def test_static_velocity_reaches_one_row_around_the_tile():
    """no fragment is moved: only the centre fetch's LINEAR footprint at vUv is loaded — the pixel's own row and one neighbour"""
    W, H = 97, 55
    for y0, rows, mask in _tile_masks(W, H, np.zeros((H, W, 2), np.float32), _params(W, H)):
        named = np.nonzero(mask)[0]
        assert named.size and named.min() >= max(0, y0 - 1) and named.max() < min(H, y0 + rows + 1), (y0, rows, named)
        assert (mask[y0 + 1:y0 + rows - 1] == 0xffffffff).all()  # ... and every column block of the rows in between


def test_vertical_pan_reaches_the_streak_length():
    """v = (0, 4 / H), intensity 1, jitter 0, deltaTime 1/60 (frameSpeed 0.6): a streak spans 4 * 0.6 rows centred on the pixel, so a tap lies
    within ceil(0.5 * 4 * 0.6) rows of it, + 1 for the LINEAR footprint's second row, + 1 for the rounding of the coordinates: 4"""
    W, H = 97, 55
    vel = np.zeros((H, W, 2), np.float32)
    vel[..., 1] = 4 / H
    reach = int(np.ceil(0.5 * 4 * 0.6)) + 2
    assert reach == 4
    for form in ("own", "traa"):
        for y0, rows, mask in _tile_masks(W, H, vel, _params(W, H, form=form, jitter=0.0)):
            named = np.nonzero(mask)[0]
            assert named.size and named.min() >= y0 - reach and named.max() < y0 + rows + reach, (form, y0, rows, named)
            assert named.min() < y0 or y0 == 0  # (it does reach past the tile: the bound is not vacuous)


def test_motion_in_the_left_quarter_names_the_left_column_blocks_only():
    """the same pan on the columns < W / 4 of a 96-wide frame, TRAA form (the centre is not the source): outside the tile only streak taps are
    loaded, of columns <= 24 (the footprint's second column) = column blocks 0 .. 8"""
    W, H = 96, 54
    vel = np.zeros((H, W, 2), np.float32)
    vel[:, :W // 4, 1] = 4 / H
    for y0, rows, mask in _tile_masks(W, H, vel, _params(W, H, form="traa", jitter=0.0)):
        outside = np.concatenate([mask[:y0], mask[y0 + rows:]])
        assert outside.any() and (outside >> 9 == 0).all(), (y0, rows, [hex(int(m)) for m in outside if m])


def test_reach_mask_on_a_whole_frame_context():
    W, H, vel, src, centre = _fixture(FLOAT)
    p = _params(W, H)
    _, mask = _reference(FLOAT, "reference_gl", p)
    assert mask.shape == (H,) and mask.dtype == np.uint32 and mask.any()
    ctx = Context(W, H)
    _upload_inputs(ctx, p, vel, src, centre)
    ctx.set_row_window(10, 12)  # the row window bounds the rows the mask is reduced over
    m = ctx.motion_blur_reach_mask(p)
    ctx.set_row_window()
    assert m.any() and (m & ~mask == 0).all() and not np.array_equal(m, mask)
    ctx.close()


# ---------------------------------------------------------------- error codes
def test_error_codes_of_the_tiled_calls():
    W, H = 16, 8
    tiled = Context(W, H, tile_y0=0, tile_rows=4, halo_rows=2)
    p = _params(W, H)
    for call in (tiled.motion_blur_stage, tiled.motion_blur_reach_mask):
        with pytest.raises(RfxError, match=r"\(-4\).*an input slot holds nothing yet"):  # host-filled inputs not uploaded
            call(p)
    tiled.upload(abi.TEX_VELOCITY, np.zeros((6, W, 4), np.float32))
    tiled.upload(abi.TEX_EFFECT_INPUT, np.zeros((6, W, 4), np.float32))
    with pytest.raises(RfxError, match=r"\(-5\).*rfx_motion_blur_stage.*rfx_motion_blur_gather"):  # tiled and unarmed
        tiled.motion_blur(p)
    bad = _params(W, H, samples=0)
    for call in (tiled.motion_blur_stage, tiled.motion_blur_reach_mask):
        with pytest.raises(RfxError, match=r"\(-1\)"):  # rfx_motion_blur's validation
            call(bad)
    linear = _params(W, H)
    linear.center = abi.TEX_EFFECT_INPUT  # an explicit LINEAR centre: its footprint leaves the rows a tile draws, and nothing gathers it
    for call in (tiled.motion_blur_stage, tiled.motion_blur_reach_mask, tiled.motion_blur):
        with pytest.raises(RfxError, match=r"\(-5\).*center must be -1 or RFX_TEX_TEMPORAL0"):
            call(linear)
    m = np.zeros(H + 1, np.uint32)
    lib = abi.load_library()
    assert lib.rfx_motion_blur_reach_mask(tiled._h, C.byref(p), m.ctypes.data_as(C.POINTER(C.c_uint32)), H + 1) == abi.RFX_EINVAL  # rows != H
    assert lib.rfx_motion_blur_reach_mask(tiled._h, C.byref(p), m.ctypes.data_as(C.POINTER(C.c_uint32)), H - 1) == abi.RFX_EINVAL
    assert tiled.motion_blur_reach_mask(p).shape == (H,)  # (the mask needs no stage)
    with pytest.raises(RfxError, match=r"\(-5\)"):
        tiled.motion_blur(p)
    tiled.motion_blur_stage(p)
    tiled.motion_blur(p)
    tiled.upload(abi.TEX_DIRECT_LIGHT, np.zeros((6, W, 4), np.float32))
    other = _params(W, H)
    other.source = abi.TEX_DIRECT_LIGHT
    with pytest.raises(RfxError, match=r"\(-4\)"):  # armed for another source
        tiled.motion_blur(other)
    tiled.motion_blur_stage(other)
    tiled.motion_blur(other)
    with pytest.raises(RfxError, match=r"\(-4\)"):
        tiled.motion_blur(p)
    with pytest.raises(RfxError, match=r"\(-4\).*communicator"):  # rfx_motion_blur_gather without a communicator
        tiled.motion_blur_gather(p)
    tiled.close()


def test_profile_names_the_reach_reduction():
    W, H = 32, 16
    ctx = Context(W, H)
    ctx.upload(abi.TEX_VELOCITY, np.full((H, W, 4), 0.1, np.float32))
    ctx.upload(abi.TEX_EFFECT_INPUT, np.ones((H, W, 4), np.float32))
    ctx.profile(True)
    for _ in range(2):
        ctx.motion_blur_reach_mask(_params(W, H))
    prof = ctx.profile_read()
    ctx.profile(False)
    assert prof["k6_motion_blur_reach"][1] == 2 and prof["k6_motion_blur_reach"][0] >= 0 and "k6_motion_blur" not in prof
    ctx.close()


# ---------------------------------------------------------------- a ring of one on the real RCCL
def test_comm_tiled_motion_blur_on_a_single_rank_ring():
    """CommTiledRenderer.motion_blur (rfx_motion_blur_gather + rfx_comm_wait + the draw) around a whole-frame context on the real RCCL: the
    reach reduction, the all-gather of the one mask with its host-side wait, no block travels — and the blurred frame is the plain context's."""
    if os.environ.get("RFX_HOSTSIM") == "1":
        pytest.skip("--hostsim: the multi-process run of test_motion_blur_tiled_hostsim.py covers the exchange over the stand-in library")
    from rfx_amd.effect import MotionBlurEffect, SSGIEffect
    from rfx_amd.scene import synthetic_frame

    W, H = 96, 54
    outs = []
    for tiled in (False, True):
        ctx = Context(W, H)
        r = tiling.CommTiledRenderer(ctx, 0, 1, Context.comm_unique_id()) if tiled else ctx
        scene = types.SimpleNamespace(frame=None)
        cam = types.SimpleNamespace(**vars(synthetic_frame(W, H, 0).camera))
        fx = SSGIEffect(None, scene, cam, dict(width=W, height=H), seeds=dict(ssgi=3, denoise=4), half_store_rtz=True)
        mb = MotionBlurEffect(None)
        for fi in range(2):
            f = synthetic_frame(W, H, fi)
            scene.frame = f
            for k, v in vars(f.camera).items():
                setattr(cam, k, v)
            fx.update(r, None)
            mb.update(r, fx.mainImage(r), 1 / 60)
            assert mb.mainImage(r) == abi.TEX_MOTION_BLUR
        outs.append(mb.output(r).copy())
        if tiled:
            assert r.blur_bytes_received == [0, 0]
            ctx.comm_destroy()
        ctx.close()
    assert outs[0].tobytes() == outs[1].tobytes() and np.isfinite(outs[0]).all()
