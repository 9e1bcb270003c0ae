"""GPU (-m gpu; also under --hostsim): K8, the PNG fragment encoded on the device (rfx_png / rfx_stage_png).  For every case the fragment must be
byte-identical to the restatement's (tests/png_device_ref.py) of the bytes ctx.export returns, and the wrapped file must decode — zlib checks
the combined Adler-32, imageio.read_png undoes the filters — to exactly those bytes."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

import png_device_ref as R
from rfx_amd import abi, imageio
from rfx_amd.context import Context, RfxError

pytestmark = pytest.mark.gpu

SRC = abi.TEX_EFFECT_INPUT
SIZES = ((5, 3), (97, 55), (128, 72))


def plant(img):
    """(H, W, 3|4) uint8 -> the (H, W, 4) float32 plane whose linear U8_SRGB export is exactly `img`: colour through the inverse transfer
    function at the byte's centre (v = s * 255 + 0.5 lands on k + 0.5), alpha = k / 255"""
    s = img[..., :3].astype(np.float64) / 255.0
    lin = np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)
    a = img[..., 3:4].astype(np.float64) / 255.0 if img.shape[-1] == 4 else np.ones(img.shape[:2] + (1,))
    return np.concatenate([lin, a], -1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def frame(W, H, channels):
    img = R.noisy_frame(W, H, channels, seed=W * 7 + channels)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def want_prefix(W, H, channels, filt):
    return R.result_prefix(frame(W, H, channels), filt)


def check(ctx, img, filt, want=None):
    """the device's result buffer for the planted `img` against the restatement; the wrapped file against ctx.export; -> the result buffer"""
    H, W, ch = img.shape
    exported = ctx.export(SRC, "u8_srgb", ch)
    assert np.array_equal(exported, img)  # the planted bytes are what K7 stages
    got = ctx.png(SRC, ch, filter=filt)
    assert got.dtype == np.uint8 and got.nbytes == ctx.png_bound(ch) == R.bound(W, H, ch)
    want = R.result_prefix(img, filt) if want is None else want
    n = struct.unpack("<Q", got[:8].tobytes())[0]
    assert 32 + n <= got.nbytes
    assert got[:32].tobytes() == want[:32], (struct.unpack("<QIIQQ", got[:32].tobytes()), struct.unpack("<QIIQQ", want[:32]))
    assert got[:32 + n].tobytes() == want
    return got


def decode(tmp_path, W, H, ch, results):
    path = tmp_path / "frame.png"
    path.write_bytes(imageio.png_from_fragments(W, H, ch, results))
    return imageio.read_png(str(path))


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4], ids=["adaptive", "none", "sub", "up", "paeth"])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_fragment_equals_the_restatement(size, channels, filt, tmp_path):
    W, H = size
    img = frame(W, H, channels)
    ctx = Context(W, H)
    ctx.upload(SRC, plant(img))
    got = check(ctx, img, filt, want_prefix(W, H, channels, filt))
    ctx.close()
    assert np.array_equal(decode(tmp_path, W, H, channels, [got]), img)


@pytest.mark.parametrize("channels,filt", [(3, 0), (4, 4)], ids=["rgb-adaptive", "rgba-paeth"])
def test_rows_longer_than_one_step_of_the_bit_window(channels, filt, tmp_path):
    """1300 pixels: a row is several steps of the kernel's sweeps (256 bytes each) and ends inside one, so bits are carried from window to window"""
    W, H = 1300, 3
    img = frame(W, H, channels)
    ctx = Context(W, H)
    ctx.upload(SRC, plant(img))
    got = check(ctx, img, filt)
    ctx.close()
    assert struct.unpack("<Q", got[:8].tobytes())[0] < 0.8 * img.size  # the compressed form
    assert np.array_equal(decode(tmp_path, W, H, channels, [got]), img)


def test_adaptive_uses_every_filter_somewhere():
    """a premise of the adaptive cases above: they are not one filter under another name"""
    types = set()
    for (W, H) in SIZES[1:]:
        types |= {int(l[0]) for l in R.filtered_rows(frame(W, H, 3), 0)}
    assert types >= {1, 2, 4}, types


def test_random_bytes_take_two_stored_blocks_per_row(tmp_path):
    W, H, ch = 16385, 2, 4
    img = np.random.default_rng(11).integers(0, 256, (H, W, ch), dtype=np.uint8)
    ctx = Context(W, H)
    ctx.upload(SRC, plant(img))
    got = check(ctx, img, 0)
    ctx.close()
    n = 1 + W * ch
    assert n > 65535 and struct.unpack("<Q", got[:8].tobytes())[0] == H * (12 + 10 + n)  # every chunk in form (b), two blocks
    assert np.array_equal(decode(tmp_path, W, H, ch, [got]), img)


def test_fibonacci_frequencies_meet_the_length_limit(tmp_path):
    """900 x 2 x 3 with filter None: the literals' frequencies are planted in Fibonacci proportion, so the unconstrained code is deeper than 15"""
    W, H, ch = 900, 2, 3
    fib = [1, 1]
    while len(fib) < 16:
        fib.append(fib[-1] + fib[-2])
    counts = fib[::-1]  # byte 0 the most frequent ... byte 15 once
    counts[0] += W * ch - sum(counts)
    row = np.repeat(np.arange(16, dtype=np.uint8), counts)
    rng = np.random.default_rng(5)
    img = np.stack([rng.permutation(row), rng.permutation(row)]).reshape(H, W, ch)
    freq = np.bincount(np.concatenate([[0], img[0].reshape(-1)]), minlength=257)
    freq[256] = 1
    assert max(R.code_lengths(freq, 99)) > 15 and max(R.code_lengths(freq, 15)) == 15
    ctx = Context(W, H)
    ctx.upload(SRC, plant(img))
    got = check(ctx, img, 1)
    ctx.close()
    assert np.array_equal(decode(tmp_path, W, H, ch, [got]), img)


@pytest.mark.parametrize("filt", [0, 1, 4])
def test_constant_image_single_literal(filt, tmp_path):
    W, H, ch = 70, 4, 3
    img = np.zeros((H, W, ch), np.uint8)
    ctx = Context(W, H)
    ctx.upload(SRC, plant(img))
    got = check(ctx, img, filt)
    ctx.close()
    assert np.array_equal(decode(tmp_path, W, H, ch, [got]), img)


def test_three_row_tiles_stitch(tmp_path):
    W, H, ch, halo = 97, 55, 3, 2
    img = frame(W, H, ch)
    a = plant(img)
    results = []
    for rank in (2, 1, 0):  # top tile first
        y0, n = Context.split_rows(H, 3, rank)
        t = Context(W, H, tile_y0=y0, tile_rows=n, halo_rows=halo)
        r0, rn = t.held_rows(SRC)
        t.upload(SRC, a[r0:r0 + rn])
        results.append(check(t, img[y0:y0 + n], 0).copy())
        t.close()
    assert np.array_equal(decode(tmp_path, W, H, ch, results), img)
    whole = want_prefix(W, H, ch, 0)
    assert sum(struct.unpack("<Q", r[:8].tobytes())[0] for r in results) != len(whole) - 32  # (each tile's first scanline has no upper neighbour)


def test_interleaved_export_and_png_tickets_with_growth():
    """five frames through the mixed sequence: stage_export and stage_png share the tickets, the two staging buffers and the back pressure; the
    formats change size on the way, so both kinds of device buffer grow"""
    W, H = 97, 55
    imgs = [R.noisy_frame(W, H, 4, seed=40 + i) for i in range(5)]
    ctx = Context(W, H)
    plan = [("png", 3, 0), ("u8", 4, None), ("png", 4, 4), ("f32", 4, None), ("png", 4, 0)]
    outs, tickets = [], []
    for i, (kind, ch, filt) in enumerate(plan):
        ctx.upload(SRC, plant(imgs[i]))
        if kind == "png":
            out = ctx.host_alloc((ctx.png_bound(ch),), np.uint8)
            t = ctx.stage_png(SRC, ch, filter=filt, out=out)
        elif kind == "u8":
            out = ctx.host_alloc((H, W, ch), np.uint8)
            t = ctx.stage_export(SRC, "u8_srgb", ch, out=out)
        else:
            out = ctx.host_alloc((H, W, ch), np.float32)
            t = ctx.stage_export(SRC, "f32", ch, out=out)
        outs.append(out)
        tickets.append(t)
        assert t == tickets[0] + i
        if i:
            ctx.export_wait(tickets[i - 1])  # one frame late
    ctx.export_wait(tickets[-1])
    for i, (kind, ch, filt) in enumerate(plan):
        if kind == "png":
            want = R.result_prefix(imgs[i][..., :ch], filt)
            assert outs[i][:len(want)].tobytes() == want, i
        elif kind == "u8":
            assert np.array_equal(outs[i], imgs[i][..., :ch]), i
        else:
            assert np.array_equal(outs[i], plant(imgs[i])[..., :ch]), i
    for t in tickets:
        assert ctx.lib.rfx_export_wait(ctx._h, t) == abi.RFX_OK
    ctx.close()


def _raw(ctx, fn, p, filt, nbytes):
    buf = np.zeros(max(nbytes, 64), np.uint8)
    if fn == "rfx_png":
        rc = ctx.lib.rfx_png(ctx._h, C.byref(p), filt, buf.ctypes.data_as(C.c_void_p), nbytes)
    else:
        t = C.c_int(0)
        rc = ctx.lib.rfx_stage_png(ctx._h, C.byref(p), filt, buf.ctypes.data_as(C.c_void_p), nbytes, C.byref(t))
        if rc == abi.RFX_OK:
            assert ctx.lib.rfx_export_wait(ctx._h, t) == abi.RFX_OK
    return rc, ctx.lib.rfx_last_error(ctx._h).decode()


@pytest.mark.parametrize("fn", ["rfx_png", "rfx_stage_png"])
def test_error_codes(fn):
    W, H = 16, 8
    ctx = Context(W, H)
    good = abi.ExportParams(SRC, abi.EXPORT_U8_SRGB, 3, 0, 1.0)
    bound = ctx.png_bound(3)
    assert bound == R.bound(W, H, 3) == int(ctx.lib.rfx_png_bound(ctx._h, C.byref(good)))
    rc, msg = _raw(ctx, fn, good, 0, bound)  # never uploaded
    assert rc == abi.RFX_ESTATE and msg.startswith(fn + ":"), (rc, msg)
    ctx.upload(SRC, np.zeros((H, W, 4), np.float32))
    for fmt in (abi.EXPORT_F32, abi.EXPORT_F16):
        p = abi.ExportParams(SRC, fmt, 3, 0, 1.0)
        assert ctx.lib.rfx_png_bound(ctx._h, C.byref(p)) == 0
        rc, msg = _raw(ctx, fn, p, 0, bound)
        assert rc == abi.RFX_EINVAL and msg.startswith(fn + ":"), (rc, msg)
    for filt in (-1, 5):
        rc, msg = _raw(ctx, fn, good, filt, bound)
        assert rc == abi.RFX_EINVAL and msg.startswith(fn + ":") and "filter" in msg, (rc, msg)
    for n in (bound - 1, bound + 1, W * H * 3):
        rc, msg = _raw(ctx, fn, good, 0, n)
        assert rc == abi.RFX_EINVAL and msg.startswith(fn + ":") and "rfx_png_bound" in msg, (rc, msg)
    for bad in (abi.ExportParams(abi.TEX_DEPTH, abi.EXPORT_U8_SRGB, 3, 0, 1.0), abi.ExportParams(SRC, abi.EXPORT_U8_SRGB, 2, 0, 1.0),
                abi.ExportParams(SRC, abi.EXPORT_U8_SRGB, 3, 2, 1.0), abi.ExportParams(SRC, abi.EXPORT_U8_SRGB, 3, 0, -1.0)):
        assert ctx.lib.rfx_png_bound(ctx._h, C.byref(bad)) == 0
        rc, msg = _raw(ctx, fn, bad, 0, bound)
        assert rc == abi.RFX_EINVAL and msg.startswith(fn + ":"), (rc, msg)
    assert _raw(ctx, fn, good, 0, bound)[0] == abi.RFX_OK
    with pytest.raises(RfxError, match="rfx_png"):
        ctx.png(SRC, 3, filter=7)
    ctx.close()


def test_the_png_encode_is_profiled():
    W, H = 97, 55
    ctx = Context(W, H)
    ctx.upload(SRC, plant(frame(W, H, 3)))
    ctx.profile(True)
    ctx.png(SRC, 3)
    ctx.profile(False)
    prof = ctx.profile_read()
    assert list(prof) == ["k7_export", "k8_png"]
    assert prof["k8_png"][1] == 1 and prof["k8_png"][0] >= 0.0 and prof["k7_export"][1] == 1
    ctx.close()
