"""GPU (-m gpu; also under --hostsim): K8's EXR fragment with run-length matches (rfx_exr_ex / rfx_stage_exr_ex with RFX_ENCODE_MATCHES; the
kernel: csrc/k8_exr.h k8_exr_rows<true>).  For every case of tests/match_cases.py the result buffer, header included, must be byte-identical to the
restatement's (tests/match_device_ref.py) of the halfs ctx.export returns; flags = 0 through the _ex calls must be the old calls' bytes."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import exr_device_ref as E
import match_cases as K
import match_device_ref as M
from rfx_amd import abi, imageio
from rfx_amd.context import Context
from test_gpu_exr_device import SRC, decode, plane_of, same_halfs

pytestmark = pytest.mark.gpu


def encode(ctx, ch, flags):
    """rfx_exr_ex, called for itself: no look at whether the library has it"""
    p = ctx.export_params(SRC, "f16", ch)
    out = np.zeros(ctx.exr_bound(ch), np.uint8)
    rc = ctx.lib.rfx_exr_ex(ctx._h, C.byref(p), flags, out.ctypes.data_as(C.c_void_p), out.nbytes)
    assert rc == abi.RFX_OK, ctx.lib.rfx_last_error(ctx._h).decode()
    return out


def check(ctx, halfs, first_y=0):
    """upload the halfs' plane: matches on against the restatement, flags = 0 and Context.exr(matches=True) against their twins -> the result"""
    ch = halfs.shape[-1]
    ctx.upload(SRC, plane_of(halfs))
    exported = ctx.export(SRC, "f16", ch)
    assert same_halfs(exported, halfs)
    rows, W = exported.shape[:2]
    got = encode(ctx, ch, abi.ENCODE_MATCHES)
    want = M.result_prefix_exr(exported, first_y)
    n = struct.unpack("<Q", got[:8].tobytes())[0]
    assert 32 + n <= got.nbytes == E.bound(W, rows, ch)
    assert got[:32].tobytes() == want[:32], (E.header_of(got), E.header_of(want))
    assert got[:32 + n].tobytes() == want
    nline = 2 * W * ch
    for (y, d), raw in zip(E.chunks_of(got), E.raw_blocks(exported)):  # zlib verifies each chunk's Adler-32
        assert (d if len(d) == nline else imageio._exr_unpredict(zlib.decompress(d))) == raw, y
    off = encode(ctx, ch, 0)
    old = ctx.exr(SRC, ch)
    n0 = struct.unpack("<Q", old[:8].tobytes())[0]
    assert off[:32 + n0].tobytes() == old[:32 + n0].tobytes() == E.result_prefix(exported, first_y) and E.header_of(off)[5] == 0
    assert n <= n0
    assert ctx.exr(SRC, ch, matches=True)[:32 + n].tobytes() == want
    return got


@pytest.mark.parametrize("name", sorted(K.EXR_CASES))
def test_result_buffer_equals_the_restatement(name, tmp_path):
    halfs = K.exr_case(name)
    H, W, ch = halfs.shape
    ctx = Context(W, H)
    got = check(ctx, halfs)
    ctx.close()
    assert same_halfs(decode(tmp_path, W, H, ch, [got]), halfs)


def test_three_row_tiles_stitch(tmp_path):
    W, H, ch, halo = 97, 55, 4, 2
    halfs = K.exr_case("half_flat_97x55")
    results = []
    for (tile, first_y), rank in zip(E.tiles_top_first(halfs, 3), (2, 1, 0)):
        y0, n = Context.split_rows(H, 3, rank)
        t = Context(W, H, tile_y0=y0, tile_rows=n, halo_rows=halo)
        r0, rn = t.held_rows(SRC)
        t.upload(SRC, plane_of(halfs)[r0:r0 + rn])
        p = t.export_params(SRC, "f16", ch)
        out = np.zeros(t.exr_bound(ch), np.uint8)
        assert t.lib.rfx_exr_ex(t._h, C.byref(p), abi.ENCODE_MATCHES, out.ctypes.data_as(C.c_void_p), out.nbytes) == abi.RFX_OK
        want = M.result_prefix_exr(halfs[y0:y0 + n], first_y)
        assert out[:len(want)].tobytes() == want
        results.append(out)
        t.close()
    whole = M.result_prefix_exr(halfs, 0)
    assert b"".join(r[32:32 + E.header_of(r)[0]].tobytes() for r in results) == whole[32:]  # no state across scanlines
    assert sum(E.header_of(r)[5] for r in results) == E.header_of(whole)[5] > 0
    assert same_halfs(decode(tmp_path, W, H, ch, results), halfs)


def test_refusals():
    W, H = 16, 8
    ctx = Context(W, H)
    ctx.upload(SRC, np.zeros((H, W, 4), np.float32))
    p = ctx.export_params(SRC, "f16", 4)
    bound = ctx.exr_bound(4)
    buf = np.zeros(bound, np.uint8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    t = C.c_int(0)
    for flags in (2, 3, 0x80000000):
        assert ctx.lib.rfx_exr_ex(ctx._h, C.byref(p), flags, ptr, bound) == abi.RFX_EINVAL
        msg = ctx.lib.rfx_last_error(ctx._h).decode()
        assert msg.startswith("rfx_exr_ex:") and "flags" in msg, msg
        assert ctx.lib.rfx_stage_exr_ex(ctx._h, C.byref(p), flags, ptr, bound, C.byref(t)) == abi.RFX_EINVAL
        assert ctx.lib.rfx_last_error(ctx._h).decode().startswith("rfx_stage_exr_ex:")
    assert ctx.lib.rfx_exr_ex(ctx._h, C.byref(p), 1, ptr, bound + 1) == abi.RFX_EINVAL and "rfx_exr_bound" in ctx.lib.rfx_last_error(ctx._h).decode()
    assert ctx.lib.rfx_stage_exr_ex(ctx._h, C.byref(p), 1, ptr, bound, None) == abi.RFX_EINVAL
    u8 = ctx.export_params(SRC, "u8_srgb", 4)
    assert ctx.lib.rfx_exr_ex(ctx._h, C.byref(u8), 1, ptr, bound) == abi.RFX_EINVAL
    assert ctx.lib.rfx_exr_ex(ctx._h, C.byref(p), 1, ptr, bound) == abi.RFX_OK
    ctx.close()


def test_the_match_encode_is_profiled():
    halfs = K.exr_case("half_flat_97x55")
    ctx = Context(97, 55)
    ctx.upload(SRC, plane_of(halfs))
    ctx.profile(True)
    ctx.exr(SRC, 4, matches=True)
    ctx.profile(False)
    prof = ctx.profile_read()
    assert list(prof) == ["k7_export", "k8_png"]
    assert prof["k8_png"][1] == 1 and prof["k8_png"][0] >= 0.0 and prof["k7_export"][1] == 1
    ctx.close()
