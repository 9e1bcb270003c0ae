"""GPU (-m gpu; also under --hostsim): K7, the streamed frame export (rfx_export / rfx_stage_export / rfx_export_wait).  F32 bit for bit against
download(), F16 against numpy's float16 rounding, U8_SRGB against imageio.tonemap under the margin rule of tests/export_cases.py; row tiles
against the whole frame; the two-buffer staging, its tickets and its growth; the error codes; the per-draw profile."""
import ctypes as C

import numpy as np
import pytest

import export_cases as X
from rfx_amd import abi
from rfx_amd.context import Context, RfxError

pytestmark = pytest.mark.gpu

SOURCES = (abi.TEX_FINAL, abi.TEX_MOTION_BLUR, abi.TEX_COMPOSE, abi.TEX_TEMPORAL0, abi.TEX_DIRECT_LIGHT, abi.TEX_EFFECT_INPUT)


def _bits(W, H, seed):
    """(H, W, 4) float32 of random BITS: quiet and signalling NaNs, infinities, subnormals — F32 must move every one of them unchanged"""
    return np.random.default_rng(seed).integers(0, 2 ** 32, (H, W, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: "%dx%d" % s)
def test_f32_is_the_sources_bits(size, channels):
    W, H = size
    ctx = Context(W, H)
    for k, src in enumerate(SOURCES):
        ctx.upload(src, _bits(W, H, 100 + k))
    for src in SOURCES:
        got = ctx.export(src, "f32", channels)
        assert got.dtype == np.float32 and got.shape == (H, W, channels)
        assert ctx.export_bytes(ctx.export_params(src, "f32", channels)) == got.nbytes == W * H * channels * 4
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ctx.download(src)[..., :channels]).view(np.uint32)), abi.TEX_NAMES[src]
    ctx.close()


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: "%dx%d" % s)
def test_f16_rounds_like_numpy(size, channels):
    W, H = size
    a = X.f16_input(W, H)
    ctx = Context(W, H)
    ctx.upload(abi.TEX_EFFECT_INPUT, a)
    X.check_f16(ctx.export(abi.TEX_EFFECT_INPUT, "f16", channels), a, channels)
    ctx.close()


@pytest.mark.parametrize("case", X.u8_cases(), ids=X.case_id)
def test_u8_srgb_meets_the_margin_rule(case):
    W, H, channels, family, exposure, operator = case
    a = X.linear_input(W, H, family)
    v, ref = X.reference_v(a, channels, operator, exposure)
    ctx = Context(W, H)
    ctx.upload(abi.TEX_FINAL, a)
    got = ctx.export(abi.TEX_FINAL, "u8_srgb", channels, operator, exposure)
    ctx.close()
    X.check_margin(got, v, ref)


def test_row_tiles_export_their_own_rows():
    W, H, halo = 97, 55, 2
    a = X.f16_input(W, H)
    a[np.isnan(a)] = 0.25  # (bytes are compared: keep every format's output a function of the value)
    forms = (("f32", 4, "linear", 1.0), ("f32", 3, "linear", 1.0), ("f16", 3, "linear", 1.0), ("f16", 4, "linear", 1.0), ("u8_srgb", 3, "aces", 0.37),
             ("u8_srgb", 4, "linear", 2.5))
    whole = Context(W, H)
    want = {}
    for src in (abi.TEX_EFFECT_INPUT, abi.TEX_COMPOSE):  # a band slot and one every context holds whole
        whole.upload(src, a)
        for f in forms:
            want[(src,) + f] = whole.export(src, *f)
    whole.close()
    for rank in range(3):
        y0, n = Context.split_rows(H, 3, rank)
        t = Context(W, H, tile_y0=y0, tile_rows=n, halo_rows=halo)
        for src in (abi.TEX_EFFECT_INPUT, abi.TEX_COMPOSE):
            r0, rn = t.held_rows(src)
            t.upload(src, a[r0:r0 + rn])
            for f in forms:
                got = t.export(src, *f)
                assert got.shape == (n, W, f[1])
                assert got.tobytes() == want[(src,) + f][y0:y0 + n].tobytes(), (rank, abi.TEX_NAMES[src], f)
        t.close()


def test_staged_exports_two_buffers_six_frames():
    W, H, frames = 960, 540, 6
    rng = np.random.default_rng(7)
    planes = [np.concatenate([rng.lognormal(-1.0, 1.5, (H, W, 3)), np.ones((H, W, 1))], -1).astype(np.float32) for _ in range(frames)]
    ctx = Context(W, H)
    want = []
    for p in planes:
        ctx.upload(abi.TEX_EFFECT_INPUT, p)
        want.append(ctx.export(abi.TEX_EFFECT_INPUT, "u8_srgb", 3, "aces", 1.0).copy())
    assert any(not np.array_equal(want[0], w) for w in want[1:])
    wait = ctx.lib.rfx_export_wait  # (the C call: its code, not an exception)
    bufs = [ctx.host_alloc((H, W, 3), np.uint8) for _ in range(2)]
    base, tickets, got = None, [], [None] * frames
    for i, p in enumerate(planes):
        ctx.upload(abi.TEX_EFFECT_INPUT, p)
        t = ctx.stage_export(abi.TEX_EFFECT_INPUT, "u8_srgb", 3, "aces", 1.0, out=bufs[i & 1])
        base = t if base is None else base
        assert t == base + i  # tickets count up (behind the ones the synchronous exports above took)
        tickets.append(t)
        if i >= 1 and i % 2 == 1:  # two in flight: wait for the NEWER one first, then the older (out of order)
            ctx.export_wait(tickets[i])
            got[i] = bufs[i & 1].copy()
            ctx.export_wait(tickets[i - 1])
            got[i - 1] = bufs[(i - 1) & 1].copy()
    for i in range(frames):
        assert np.array_equal(got[i], want[i]), i
    for t in tickets:  # waiting again: RFX_OK at once, for the retired ones and the last two alike
        assert wait(ctx._h, t) == abi.RFX_OK
    assert wait(ctx._h, tickets[-1] + 1) == abi.RFX_EINVAL and wait(ctx._h, 0) == abi.RFX_EINVAL  # never issued
    ctx.close()


def test_sync_publishes_a_staged_export_and_the_staging_buffer_grows():
    W, H = 97, 55
    a = X.linear_input(W, H, "uniform_1p2", planted=False)
    ctx = Context(W, H)
    ctx.upload(abi.TEX_EFFECT_INPUT, a)
    small = ctx.host_alloc((H, W, 3), np.uint8)
    small[...] = 0
    ctx.stage_export(abi.TEX_EFFECT_INPUT, "u8_srgb", 3, out=small)
    ctx.sync()  # no export_wait: rfx_sync drains the download stream
    want_small = ctx.export(abi.TEX_EFFECT_INPUT, "u8_srgb", 3)
    assert np.array_equal(small, want_small) and small.any()
    # a larger format through the same two staging buffers: each of them grows (12 -> 64 bytes per group), twice over
    big = [ctx.host_alloc((H, W, 4), np.float32) for _ in range(2)]
    t = [ctx.stage_export(abi.TEX_EFFECT_INPUT, "f32", 4, out=b) for b in big]
    mid = ctx.host_alloc((H, W, 4), np.float16)
    t.append(ctx.stage_export(abi.TEX_EFFECT_INPUT, "f16", 4, out=mid))  # ... and a smaller one after the larger
    for k in t:
        ctx.export_wait(k)
    for b in big:
        assert np.array_equal(b.view(np.uint32), a.view(np.uint32))
    X.check_f16(mid, a, 4)
    assert np.array_equal(ctx.export(abi.TEX_EFFECT_INPUT, "u8_srgb", 3), want_small)
    ctx.close()


def test_pageable_buffers_are_accepted():
    W, H = 97, 55
    a = X.linear_input(W, H, "uniform_1p2", planted=False)
    ctx = Context(W, H)
    ctx.upload(abi.TEX_DIRECT_LIGHT, a)
    out = np.zeros((H, W, 3), np.float32)
    ctx.export_wait(ctx.stage_export(abi.TEX_DIRECT_LIGHT, "f32", 3, out=out))
    assert np.array_equal(out, a[..., :3])
    ctx.close()


def _raw(ctx, fn, p, nbytes=None):
    """the C call itself -> (code, message)"""
    n = ctx.export_bytes(p) if nbytes is None else nbytes
    buf = np.zeros(max(n, 16), np.uint8)
    if fn == "rfx_export":
        rc = ctx.lib.rfx_export(ctx._h, C.byref(p), buf.ctypes.data_as(C.c_void_p), n)
    else:
        t = C.c_int(0)
        rc = ctx.lib.rfx_stage_export(ctx._h, C.byref(p), buf.ctypes.data_as(C.c_void_p), n, C.byref(t))
        if rc == abi.RFX_OK:  # `buf` goes when this returns
            assert ctx.lib.rfx_export_wait(ctx._h, t) == abi.RFX_OK
    return rc, ctx.lib.rfx_last_error(ctx._h).decode()


BAD_PARAMS = {
    "source_not_rgba32f": dict(source=abi.TEX_DENOISE_B0),
    "source_depth": dict(source=abi.TEX_DEPTH),
    "source_out_of_range": dict(source=abi.TEX_COUNT),
    "format": dict(format=3),
    "channels_2": dict(channels=2),
    "channels_5": dict(channels=5),
    "operator": dict(format=abi.EXPORT_U8_SRGB, tonemap=2),
    "exposure_negative": dict(format=abi.EXPORT_U8_SRGB, exposure=-1.0),
    "exposure_nan": dict(format=abi.EXPORT_U8_SRGB, exposure=float("nan")),
    "exposure_inf": dict(format=abi.EXPORT_U8_SRGB, exposure=float("inf")),
    "operator_with_f16": dict(format=abi.EXPORT_F16, tonemap=1),
    "exposure_with_f32": dict(format=abi.EXPORT_F32, exposure=2.0),
}


@pytest.mark.parametrize("fn", ["rfx_export", "rfx_stage_export"])
@pytest.mark.parametrize("name", sorted(BAD_PARAMS))
def test_bad_params_are_einval(name, fn):
    ctx = Context(16, 8)
    ctx.upload(abi.TEX_EFFECT_INPUT, np.zeros((8, 16, 4), np.float32))
    kw = dict(source=abi.TEX_EFFECT_INPUT, format=abi.EXPORT_F32, channels=3, tonemap=0, exposure=1.0)
    kw.update(BAD_PARAMS[name])
    p = abi.ExportParams(**kw)
    assert ctx.export_bytes(p) == 0
    rc, msg = _raw(ctx, fn, p, nbytes=16 * 8 * 3 * 4)
    assert rc == abi.RFX_EINVAL and msg.startswith(fn + ":"), (rc, msg)
    ctx.close()


@pytest.mark.parametrize("fn", ["rfx_export", "rfx_stage_export"])
def test_wrong_byte_count_and_empty_source(fn):
    ctx = Context(16, 8)
    p = abi.ExportParams(abi.TEX_EFFECT_INPUT, abi.EXPORT_U8_SRGB, 3, 1, 1.0)
    assert ctx.export_bytes(p) == 16 * 8 * 3
    rc, msg = _raw(ctx, fn, p)  # never uploaded
    assert rc == abi.RFX_ESTATE and msg.startswith(fn + ":"), (rc, msg)
    rc, msg = _raw(ctx, fn, abi.ExportParams(abi.TEX_FINAL, abi.EXPORT_F16, 4, 0, 0.0))  # never drawn
    assert rc == abi.RFX_ESTATE and msg.startswith(fn + ":"), (rc, msg)
    ctx.upload(abi.TEX_EFFECT_INPUT, np.zeros((8, 16, 4), np.float32))
    for n in (16 * 8 * 3 - 1, 16 * 8 * 3 + 1, 16 * 8 * 4):
        rc, msg = _raw(ctx, fn, p, nbytes=n)
        assert rc == abi.RFX_EINVAL and msg.startswith(fn + ":") and "rfx_export_bytes" in msg, (rc, msg)
    assert _raw(ctx, fn, p)[0] == abi.RFX_OK
    with pytest.raises(RfxError, match="rfx_export_wait"):
        ctx.export_wait(99)
    ctx.close()


def test_row_window_does_not_apply_and_the_encode_is_profiled():
    W, H = 97, 55
    a = X.linear_input(W, H, "uniform_1p2", planted=False)
    ctx = Context(W, H)
    ctx.upload(abi.TEX_EFFECT_INPUT, a)
    want = ctx.export(abi.TEX_EFFECT_INPUT, "f16", 3)
    ctx.set_row_window(10, 20)
    ctx.profile(True)
    got = ctx.export(abi.TEX_EFFECT_INPUT, "f16", 3)
    ctx.profile(False)
    ctx.set_row_window()
    assert got.tobytes() == want.tobytes()
    prof = ctx.profile_read()
    assert prof["k7_export"][1] == 1 and prof["k7_export"][0] >= 0.0 and list(prof) == ["k7_export"]
    ctx.close()
