"""GPU (-m gpu; also under --hostsim): K8's EXR pre-transform, the ZIPS chunks encoded on the device (rfx_exr / rfx_stage_exr).  For every case
the result buffer must be byte-identical to the restatement's (tests/exr_device_ref.py) of the halfs ctx.export(source, "f16", channels)
returns, and the wrapped file must decode — zlib checks each chunk's Adler-32, imageio.read_exr undoes the predictor — to exactly those halfs."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np
import pytest

import exr_device_ref as E
import export_cases as X
import png_device_ref as R
from rfx_amd import abi, imageio
from rfx_amd.context import Context, RfxError

pytestmark = pytest.mark.gpu

SRC = abi.TEX_EFFECT_INPUT


def plane_of(halfs):
    """(H, W, 3|4) float16 -> the (H, W, 4) float32 plane whose F16 export is exactly `halfs` (widening is exact; a missing alpha is 1)"""
    a = np.ones(halfs.shape[:2] + (4,), np.float32)
    a[..., :halfs.shape[-1]] = halfs.astype(np.float32)
    return a


def decode(tmp_path, W, H, ch, results):
    """the wrapped file through imageio.read_exr -> (H, W, ch) float16 in the export's channel order"""
    path = tmp_path / "frame.exr"
    path.write_bytes(imageio.exr_from_fragments(W, H, ch, results))
    planes = imageio.read_exr(str(path))
    assert sorted(planes) == sorted("RGBA"[:ch])
    assert set(imageio.exr_channel_types(str(path)).values()) == {"half"}
    return np.stack([planes[c] for c in "RGBA"[:ch]], -1).astype(np.float16)


def same_halfs(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


def check(ctx, plane, ch, first_y=0):
    """upload `plane`, encode: the device's result buffer against the restatement of ctx.export's halfs -> (result buffer, exported halfs)"""
    ctx.upload(SRC, plane)
    exported = ctx.export(SRC, "f16", ch)
    rows, W = exported.shape[:2]
    got = ctx.exr(SRC, ch)
    assert got.dtype == np.uint8 and got.nbytes == ctx.exr_bound(ch) == E.bound(W, rows, ch)
    want = E.result_prefix(exported, first_y)
    n = struct.unpack("<Q", got[:8].tobytes())[0]
    assert 32 + n <= got.nbytes
    assert got[:32].tobytes() == want[:32], (E.header_of(got), E.header_of(want))
    assert got[:32 + n].tobytes() == want
    # every chunk on its own: zlib verifies the Adler-32; a chunk of n bytes is the raw block
    nline = 2 * W * ch
    for (y, d), raw in zip(E.chunks_of(got), E.raw_blocks(exported)):
        assert len(d) <= nline
        assert (d if len(d) == nline else imageio._exr_unpredict(zlib.decompress(d))) == raw, y
    return got, exported


def run_case(tmp_path, plane, ch):
    H, W = plane.shape[:2]
    ctx = Context(W, H)
    got, exported = check(ctx, plane, ch)
    ctx.close()
    assert same_halfs(decode(tmp_path, W, H, ch, [got]), exported)
    return got, exported


@functools.lru_cache(maxsize=None)
def family_input(W, H, family):
    a = X.f16_input(W, H) if family == "f16_specials" else X.linear_input(W, H, family)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("family", X.FAMILIES + ("f16_specials",))
@pytest.mark.parametrize("shape", [(97, 55, 4), (128, 72, 3)], ids=lambda s: "%dx%dx%d" % s)
def test_families_and_planted_specials(shape, family, tmp_path):
    W, H, ch = shape
    got, exported = run_case(tmp_path, family_input(W, H, family), ch)
    X.check_f16(exported, family_input(W, H, family), ch)  # (the export itself: the halfs in the file are the converted input)


@pytest.mark.parametrize("shape", [(1, 1, 3), (1, 1, 4), (5, 3, 3), (32, 2, 4), (43, 2, 3)], ids=lambda s: "%dx%dx%d" % s)
def test_short_scanlines_and_sweep_boundaries(shape, tmp_path):
    """n = 6 / 8: the raw form with idle lanes; n = 30: the even / odd boundary at byte 15 inside a lane's group of four; n = 256: exactly one
    sweep; n = 258: one pair of bytes into a second sweep"""
    W, H, ch = shape
    got, _ = run_case(tmp_path, plane_of(E.smooth_noisy_halfs(W, H, ch, seed=W)), ch)
    if W == 1:
        assert E.header_of(got)[4] == H  # too short to gain: raw
    if W >= 32:
        assert E.header_of(got)[4] == 0  # both sweep cases go through the bit window


def test_bits_carried_across_windows(tmp_path):
    W, H, ch = 1300, 3, 4
    got, exported = run_case(tmp_path, plane_of(E.smooth_noisy_halfs(W, H, ch, seed=2)), ch)
    assert E.header_of(got)[4] == 0 and E.header_of(got)[0] < 0.8 * exported.nbytes  # the compressed form


@pytest.mark.parametrize("kind", ["smooth", "random"])
def test_scanline_longer_than_16_bits(kind, tmp_path):
    """n = 65 544: nothing 16-bit in sizes or offsets (the random row's chunk size is n itself)"""
    W, H, ch = 8193, 1, 4
    halfs = E.smooth_noisy_halfs(W, H, ch, seed=3) if kind == "smooth" else E.random_halfs(W, H, ch, seed=3)
    got, _ = run_case(tmp_path, plane_of(halfs), ch)
    assert E.header_of(got)[3] == 65544 and E.header_of(got)[4] == (0 if kind == "smooth" else 1)


def test_all_zeros_then_one_constant_colour(tmp_path):
    """two- and three-symbol codes: d is 0 then 128s for a zero scanline; a constant colour adds the steps between the byte planes"""
    W, H, ch = 8, 4, 4
    ctx = Context(W, H)
    for plane in (np.zeros((H, W, 4), np.float32), np.tile(np.array([0.25, 1.0, 3.0, 0.5], np.float32), (H, W, 1))):
        got, exported = check(ctx, plane, ch)
        assert E.header_of(got)[4] == 0
        assert same_halfs(decode(tmp_path, W, H, ch, [got]), exported)
    ctx.close()


def test_random_halfs_take_the_raw_form_and_the_bound_is_tight(tmp_path):
    W, H, ch = 64, 4, 4
    got, _ = run_case(tmp_path, plane_of(E.random_halfs(W, H, ch, seed=4)), ch)
    nbytes, chunks, first_y, raw, raw_chunks, zero = E.header_of(got)
    assert raw_chunks == 4 == chunks and nbytes + 32 == got.nbytes == E.bound(W, H, ch) and raw == H * 2 * W * ch and zero == 0 and first_y == 0


def test_smooth_and_random_rows_alternating(tmp_path):
    W, H, ch = 97, 6, 3
    halfs = E.smooth_noisy_halfs(W, H, ch, seed=5)
    halfs[1::2] = E.random_halfs(W, H // 2, ch, seed=6)
    got, _ = run_case(tmp_path, plane_of(halfs), ch)
    n = 2 * W * ch
    sizes = [len(d) for _, d in E.chunks_of(got)]
    assert [s == n for s in sizes] == [True, False] * 3  # (scanline 0 is the top row, H - 1: odd, random)
    assert E.header_of(got)[4] == 3


def test_three_row_tiles_concatenate_to_the_whole_frame(tmp_path):
    W, H, ch, halo = 97, 55, 4, 2
    a = family_input(W, H, "lognormal")
    whole = Context(W, H)
    ref, exported = check(whole, a, ch)
    whole.close()
    results = []
    for rank in (2, 1, 0):  # top tile first
        y0, n = Context.split_rows(H, 3, rank)
        t = Context(W, H, tile_y0=y0, tile_rows=n, halo_rows=halo)
        r0, rn = t.held_rows(SRC)
        got, _ = check(t, a[r0:r0 + rn], ch, first_y=H - y0 - n)
        results.append(got.copy())
        t.close()
    frag = b"".join(r[32:32 + E.header_of(r)[0]].tobytes() for r in results)
    assert frag == ref[32:32 + E.header_of(ref)[0]].tobytes()
    assert sum(E.header_of(r)[4] for r in results) == E.header_of(ref)[4]
    assert imageio.exr_from_fragments(W, H, ch, results) == imageio.exr_from_fragments(W, H, ch, [ref])
    assert same_halfs(decode(tmp_path, W, H, ch, results), exported)


def test_mixed_sequence_on_the_two_staging_buffers():
    """stage_exr, stage_png, stage_export, stage_exr over different uploads: one ticket sequence, each ticket yields its own frame"""
    W, H = 97, 55
    halfs = [E.smooth_noisy_halfs(W, H, 4, seed=30 + i) for i in range(4)]
    ctx = Context(W, H)
    plan = [("exr", 4), ("png", 3), ("f16", 3), ("exr", 3)]
    outs, tickets, want = [], [], []
    for i, (kind, ch) in enumerate(plan):
        ctx.upload(SRC, plane_of(halfs[i]))
        if kind == "exr":
            out = ctx.host_alloc((ctx.exr_bound(ch),), np.uint8)
            t = ctx.stage_exr(SRC, ch, out=out)
            want.append(E.result_prefix(halfs[i][..., :ch]))
        elif kind == "png":
            out = ctx.host_alloc((ctx.png_bound(ch),), np.uint8)
            t = ctx.stage_png(SRC, ch, filter=0, out=out)
            want.append(None)
        else:
            out = ctx.host_alloc((H, W, ch), np.float16)
            t = ctx.stage_export(SRC, "f16", ch, out=out)
            want.append(None)
        outs.append(out)
        tickets.append(t)
        assert t == tickets[0] + i
        if i:
            ctx.export_wait(tickets[i - 1])  # one frame late
    ctx.export_wait(tickets[-1])
    for i, (kind, ch) in enumerate(plan):
        if kind == "exr":
            assert outs[i][:len(want[i])].tobytes() == want[i], i
        elif kind == "png":
            ctx.upload(SRC, plane_of(halfs[i]))
            u8 = ctx.export(SRC, "u8_srgb", ch)
            w = R.result_prefix(u8, 0)
            assert outs[i][:len(w)].tobytes() == w, i
        else:
            assert same_halfs(outs[i], halfs[i][..., :ch]), i
    for t in tickets:
        assert ctx.lib.rfx_export_wait(ctx._h, t) == abi.RFX_OK
    ctx.close()


def _raw(ctx, fn, p, nbytes):
    buf = np.zeros(max(nbytes, 64), np.uint8)
    if fn == "rfx_exr":
        rc = ctx.lib.rfx_exr(ctx._h, C.byref(p), buf.ctypes.data_as(C.c_void_p), nbytes)
    else:
        t = C.c_int(0)
        rc = ctx.lib.rfx_stage_exr(ctx._h, C.byref(p), buf.ctypes.data_as(C.c_void_p), nbytes, C.byref(t))
        if rc == abi.RFX_OK:
            assert ctx.lib.rfx_export_wait(ctx._h, t) == abi.RFX_OK
    return rc, ctx.lib.rfx_last_error(ctx._h).decode()


@pytest.mark.parametrize("fn", ["rfx_exr", "rfx_stage_exr"])
def test_error_codes(fn):
    W, H = 16, 8
    ctx = Context(W, H)
    good = abi.ExportParams(SRC, abi.EXPORT_F16, 4, 0, 1.0)
    bound = ctx.exr_bound(4)
    assert bound == E.bound(W, H, 4) == int(ctx.lib.rfx_exr_bound(ctx._h, C.byref(good)))
    rc, msg = _raw(ctx, fn, good, bound)  # never uploaded
    assert rc == abi.RFX_ESTATE and msg.startswith(fn + ":"), (rc, msg)
    ctx.upload(SRC, np.zeros((H, W, 4), np.float32))
    for fmt in (abi.EXPORT_F32, abi.EXPORT_U8_SRGB):
        p = abi.ExportParams(SRC, fmt, 4, 0, 1.0)
        assert ctx.lib.rfx_exr_bound(ctx._h, C.byref(p)) == 0
        rc, msg = _raw(ctx, fn, p, bound)
        assert rc == abi.RFX_EINVAL and msg.startswith(fn + ":"), (rc, msg)
    for n in (bound - 1, bound + 1, W * H * 8):
        rc, msg = _raw(ctx, fn, good, n)
        assert rc == abi.RFX_EINVAL and msg.startswith(fn + ":") and "rfx_exr_bound" in msg, (rc, msg)
    for bad in (abi.ExportParams(abi.TEX_DEPTH, abi.EXPORT_F16, 4, 0, 1.0), abi.ExportParams(SRC, abi.EXPORT_F16, 2, 0, 1.0),
                abi.ExportParams(SRC, abi.EXPORT_F16, 4, 1, 1.0), abi.ExportParams(SRC, abi.EXPORT_F16, 4, 0, 0.5)):
        assert ctx.lib.rfx_exr_bound(ctx._h, C.byref(bad)) == 0
        rc, msg = _raw(ctx, fn, bad, bound)
        assert rc == abi.RFX_EINVAL and msg.startswith(fn + ":"), (rc, msg)
    assert _raw(ctx, fn, good, bound)[0] == abi.RFX_OK
    with pytest.raises(RfxError, match="rfx_exr"):
        ctx.exr(SRC, 2)
    ctx.close()


def test_the_exr_encode_is_profiled_as_k8():
    W, H = 97, 55
    ctx = Context(W, H)
    ctx.upload(SRC, plane_of(E.smooth_noisy_halfs(W, H, 4)))
    ctx.profile(True)
    ctx.exr(SRC, 4)
    ctx.profile(False)
    prof = ctx.profile_read()
    assert list(prof) == ["k7_export", "k8_png"]
    assert prof["k8_png"][1] == 1 and prof["k8_png"][0] >= 0.0 and prof["k7_export"][1] == 1
    ctx.close()
