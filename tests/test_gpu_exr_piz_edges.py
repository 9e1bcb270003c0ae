"""rfx.h "EXR blocks with PIZ" at the edges of the format and of the decode (k9_exr_import.hip's k9_piz_huf with its wave-wide IO, k9_piz_planes;
csrc/k9_piz.h): blocks written by tests/piz_cases.py, not by the library's writer — code lengths to 58 bits, codes that all miss the primary
table, a single code, bitmaps that are supersets, full, padded or empty, padded framing fields, run escapes planted at the positions where the
wave's output buffer changes state, and block shapes whose cells are clipped on both axes or have no wavelet level.  A frame reaches the C ABI as
a descriptor built here: the blocks' bytes one behind the other and an imageio.ExrAovLayout.  The expected frame is known by construction: the
planes the blocks were made from, through Context.stage_aov on a second context (tests/test_piz_cases_cpu.py has shown on the host that two
decoders return exactly those planes from these blocks).  Every comparison is equality of the bytes of DEPTH, GBUFFER, VELOCITY and
DIRECT_LIGHT.  Runs on the device (-m gpu) and on the host simulator (--hostsim)."""
import ctypes as C
import struct

import numpy as np
import pytest

import piz_cases as PC
import test_gpu_exr_import as T

pytestmark = pytest.mark.gpu

K9_E_PIZ_LENGTHS, K9_E_PIZ_RUN = 19, 21  # csrc/k9_piz.h


def staged(frame, planes=None, ctx_args=(), bands=((None, None),)):
    """the four slots after the frame went in band by band: through the device decode of its blocks, or — planes given — through stage_aov.
    -> (the downloads, the status of the last band or None)"""
    from rfx_amd.context import Context
    c = Context(frame.W, frame.H, *ctx_args)
    status = None
    if planes is None:
        assert c.has_exr_piz
        data, lay = frame.descriptor()
    for row0, rows in bands:
        if planes is None:
            want = int(lay.band_blocks(row0, rows)["packed_bytes"].sum())
            assert c.exr_blocks_stage_bytes(data, lay, row0, rows) == want > 0
            c.stage_exr_blocks(data, lay, row0, rows)
            status = c.exr_aov_status()
            assert status[0] == 0 or len(bands) == 1
        elif row0 is None:
            c.stage_aov(planes)
        else:
            c.stage_aov({k: v[row0:row0 + rows] for k, v in planes.items()}, row0, rows)
    c.stage_flip()
    out = [c.download(t) for t in T._slots()]
    c.close()
    return out, status


def check(frame, what, **kw):
    got, status = staged(frame, **kw)
    assert status == (0, -1, 0), what
    want, _ = staged(frame, frame.aov_planes(), **kw)
    T.assert_same(got, want, what)


@pytest.mark.parametrize("name", PC.STREAM_CASES)
def test_stream_forms(name):
    """70 x 33: per part a scanline block of 32 rows and one of 1 row, which has no wavelet level; what each case's blocks hold is asserted from
    their bytes by tests/test_piz_cases_cpu.py"""
    frame, claims = PC.stream_case(name)
    assert (frame.W, frame.H) == (70, 33) and claims
    check(frame, name)


def test_last_word_alone_in_its_group():
    """65 words: the flush at position 63 stores a full group, the final one the 65th word alone (tests/piz_cases.py)"""
    check(PC.last_word_alone_in_its_group(), "65 words")


@pytest.mark.parametrize("w14", [True, False], ids=["14bit", "16bit"])
@pytest.mark.parametrize("cols,rows", PC.SHAPES, ids=lambda v: str(v))
def test_block_shapes(cols, rows, w14):
    """one block per part, a HALF part and a FLOAT part, in 14-bit arithmetic and — the full bitmap — modulo 2^16.  1 x 1 is larger packed than raw;
    1 x 40 and 40 x 1 have no level; 63 x 65 .. 129 x 127 clip their cells on both axes (65 x 127 .. 129 x 127 with Q = 64); 257 x 32 has five
    cells per word plane in x: more turns than workgroups share a block"""
    frame = PC.shape_case(cols, rows, w14)
    assert len(frame.blocks) == 2 and all(r[3:] == (cols, rows) for r in frame.rects)
    check(frame, "%d x %d" % (cols, rows))


def test_tiles_of_127_x_129_whole_and_in_bands_that_cut_them():
    """200 x 140 in tiles of 127 x 129: 127 x 129, 73 x 129, 127 x 11, 73 x 11 per part.  Then a context of tile rows 48 .. 103 with a halo of 3:
    its band needs the tiles of 129 rows alone (frame rows 11 .. 139), the band below all four, the band above again the upper two."""
    from rfx_amd import abi
    from rfx_amd.context import Context
    frame = PC.tiled_case()
    data, lay = frame.descriptor()
    assert sorted((int(b["cols"]), int(b["rows"])) for b in lay.blocks[lay.blocks["part"] == 0]) == [(73, 11), (73, 129), (127, 11), (127, 129)]
    check(frame, "whole")
    tall = int(lay.blocks["packed_bytes"][lay.blocks["rows"] == 129].sum())
    everything = int(lay.blocks["packed_bytes"].sum())
    c = Context(PC.TW, PC.TH, 0, 48, 56, 3)
    assert c.held_rows(abi.TEX_GBUFFER) == (45, 62)
    assert c.exr_blocks_stage_bytes(data, lay, 48, 56) == tall and c.exr_blocks_stage_bytes(data, lay, 104, 36) == tall < everything
    assert c.exr_blocks_stage_bytes(data, lay, 0, 48) == everything and c.exr_blocks_stage_bytes(data, lay, 0, 11) == everything - tall
    c.close()
    check(frame, "bands", ctx_args=(0, 48, 56, 3), bands=((48, 56), (0, 48), (104, 36)))


def test_the_limit_of_128_x_128():
    """a block of 128 x 128 is refused by the plan, before anything is staged: another frame staged just before, not yet flipped, is what the
    flip publishes.  128 x 127 decodes; 127 x 4096 is planned (its bytes are never looked at)."""
    from rfx_amd import abi
    from rfx_amd.context import Context
    one = lambda W, H: [(p, 0, 0, W, H) for p in range(2)]  # noqa: E731
    big = PC.Frame(128, 128, PC.SPLIT, one(128, 128), PC.content(128, 128, 51, values=7, palette=7))
    data, lay = big.descriptor()
    c = Context(128, 128)
    other = PC.Frame(128, 128, PC.SPLIT, one(128, 128), PC.content(128, 128, 52), lambda k, r: b"")  # (its planes alone are used)
    c.stage_aov(big.aov_planes())
    c.stage_flip()
    c.stage_aov(other.aov_planes())  # in the back buffers when the refused call comes: what it would overwrite if it stored after all
    f, keep = c._exr_block_frame(data, lay)
    assert c.exr_blocks_stage_bytes(data, lay) == 0
    assert c.lib.rfx_stage_exr_blocks_piz(c._h, C.byref(f), 0, 128) == abi.RFX_EINVAL
    assert "a PIZ block of 128 x 128 texels or more" in c.lib.rfx_last_error(c._h).decode()
    c.stage_flip()
    got = [c.download(t) for t in T._slots()]
    c.close()
    want, _ = staged(other, other.aov_planes())
    T.assert_same(got, want, "after the refused call")
    refused, _ = staged(big, big.aov_planes())
    assert any(g.tobytes() != r.tobytes() for g, r in zip(got, refused))  # (the two frames differ in the slots)
    check(PC.Frame(128, 127, PC.SPLIT, one(128, 127), PC.content(128, 127, 53)), "128 x 127")
    long_ = PC.Frame(127, 4096, PC.SPLIT, one(127, 4096), {}, lambda k, r: b"\0" * (1000 + k))
    data, lay = long_.descriptor()
    c = Context(127, 4096)
    assert c.exr_blocks_stage_bytes(data, lay) == 2001
    c.close()


def test_status_with_two_bad_blocks_among_four():
    """3 x 12, depth alone in a HALF part of four blocks of 3 x 3 — nine words each — and every other channel in a second part: block 1 is the
    `run_past_nwords` stream and block 3 the `over_subscribed` one of tests/test_piz_core_cpu.py (refused before any store, and run under the
    sanitizers there), behind an empty bitmap.  Two bad blocks, the first one's index and code; their depth reads as not covered, every other
    texel is the clean frame's."""
    W, H = 3, 12
    rest = [c for c in PC.MIXED_PART if c[0] != "depth.Z"]
    parts = [[("depth.Z", PC.HALF)], rest]
    rects = [(0, 0, y, 3, 3) for y in (0, 3, 6, 9)] + [(1, 0, 0, W, H)]
    ch = PC.content(W, H, 61)
    ch["depth.Z"] = np.random.default_rng(62).integers(2, 12, (H, W)).astype(np.float32)  # (never 1: covered)
    wrap = lambda huf: struct.pack("<HHi", 8191, 0, len(huf)) + huf  # noqa: E731
    bad = {1: wrap(PC.huffman_block(PC.GAPS, 0, 300, [0, ("run", 9)])), 3: wrap(PC.huffman_block({0: 1, 1: 1, 2: 1}, 0, 2, [0]))}
    frame = PC.Frame(W, H, parts, rects, ch, lambda k, r: bad.get(k, {}))
    assert all(len(b) != frame.raw_bytes(k) for k, b in enumerate(frame.blocks))
    got, status = staged(frame)
    assert status == (2, 1, K9_E_PIZ_RUN)
    holes = dict(ch)
    holes["depth.Z"] = ch["depth.Z"].copy()
    for k in bad:
        y = rects[k][2]
        holes["depth.Z"][y:y + 3] = 1.0
    want, _ = staged(frame, frame.aov_planes(holes))
    T.assert_same(got, want)
    clean, _ = staged(frame, frame.aov_planes())
    keep = np.ones((H, W), bool)
    for k in bad:
        y = rects[k][2]
        keep[H - y - 3:H - y] = False  # scanline y is frame row H - 1 - y
    for g, w in zip(got, clean):
        assert g[keep].tobytes() == w[keep].tobytes()
    assert (got[0][~keep] == 1.0).all() and (clean[0][~keep] != 1.0).any()
    # each bad block alone gives its own code
    alone = PC.Frame(W, H, parts, rects, ch, lambda k, r: bad[3] if k == 3 else {})
    assert staged(alone)[1] == (1, 3, K9_E_PIZ_LENGTHS)
