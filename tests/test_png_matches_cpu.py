"""CPU (-m "not gpu"): the match form of include/rfx.h "Match form" for PNG fragments without a device — the restatement
(tests/match_device_ref.py) over tests/match_cases.py: the token rule against a run-length decoder, every chunk through zlib and through the
project's own inflater (csrc/k9_inflate.h), whole files through imageio.read_png, row tiles, the form choice, match_form_chunks, the hosts'
wrap, the premises of the cases, the FrameExporter's call order and refusals with matches=True, and the size against zlib's Z_RLE coding."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import match_cases as K
import match_device_ref as M
import png_device_ref as R
from rfx_amd import abi, frames, imageio
from test_inflate_core_cpu import K9_OK, driver, run  # noqa: F401  (driver: the fixture that builds tests/inflate_core_driver.cpp)
from test_png_device_cpu import tiles_top_first

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")

NAMES = sorted(K.PNG_CASES)


def test_token_rule():
    rng = np.random.default_rng(4)
    for trial in range(200):
        n = int(rng.integers(1, 900))
        d = rng.integers(0, 3, n).astype(np.uint8) if trial % 2 else np.repeat(rng.integers(0, 256, 40), rng.integers(1, 600, 40))[:n].astype(np.uint8)
        pos, tok = M.tokens_at(d)
        assert np.array_equal(M.expand(tok), d)
        lengths = tok[tok >= 256] - 256
        assert ((lengths >= 3) & (lengths <= 258)).all() and (np.diff(pos) > 0).all()
        # a literal is a non-repeating position or one of the last 1 or 2 of its interval's pieces; what a match covers is repeating throughout
        rep = set(K.repeating(d).tolist())
        for p, t in zip(pos, tok):
            if t >= 256:
                assert all(q in rep for q in range(p - (t - 256) + 1, p + 1))
    assert M.tokens(np.zeros(1 + 258 + 258 + 2, np.uint8)).tolist() == [0, 256 + 258, 256 + 258, 0, 0]
    assert M.tokens(np.zeros(1 + 258 + 3, np.uint8)).tolist() == [0, 256 + 258, 256 + 3]
    assert M.tokens(np.array([5, 5, 5], np.uint8)).tolist() == [5, 5, 5] and M.tokens(np.array([5, 5, 5, 5], np.uint8)).tolist() == [5, 256 + 3]
    assert [M.length_symbol(l) for l in (3, 10, 11, 12, 13, 18, 19, 257, 258)] == [
        (257, 0, 0), (264, 0, 0), (265, 1, 0), (265, 1, 1), (266, 1, 0), (268, 1, 1), (269, 2, 0), (284, 5, 30), (285, 0, 0)]


def test_the_cases_reach_their_edges():
    for m in K.RUN_LENGTHS:
        d = K.png_line("run_%d" % m)
        lengths = sorted((M.tokens(d)[M.tokens(d) >= 256] - 256).tolist())
        want = [] if m < 3 else [m] * 10 if m <= 4 else [m] if m <= 258 else [m - 258, 258] if m - 258 >= 3 and m < 516 else [258] if m < 516 else \
            [258, 258] if m - 516 < 3 else [m - 516, 258, 258]
        assert lengths == sorted(want), (m, lengths)
        assert K.repeating(d).size == m * len(K.run_starts(m))
    assert {s % 4 for s in K.run_starts(3)} == {0, 1, 2, 3}  # the short runs end on every one of a lane's four positions
    d = K.png_line("run_from_d1")
    assert d[0] == d[1] and K.repeating(d)[0] == 1
    d = K.png_line("run_to_last_byte")
    assert K.repeating(d)[-1] == d.size - 1
    one, two = K.repeating(K.png_line("run_across_one_step")), K.repeating(K.png_line("run_across_two_steps"))
    assert one[0] < 256 <= one[-1] < 512 and two[0] < 256 and two[-1] >= 512
    d = K.png_line("constant_row")
    assert (d == d[0]).all()
    assert K.repeating(K.png_line("no_repeat")).size == 0
    d = K.png_line("only_match_loses")
    c, a = M.png_payload_c(d), R.compressed_payload(d)
    assert c is not None and len(c) >= len(a) and len(a) <= len(R.stored_payload(d)) and M.png_payload(d) == (a, False)
    d = K.png_line("stored_row")
    assert M.png_payload_c(d) is not None and M.png_payload(d) == (R.stored_payload(d), False)
    assert K.png_line("long_scanline").size == 65545
    for name in ("half_flat_97x55", "half_flat_rgba_paeth_128x72", "ramp_97x55", "constant_5x3"):
        img, filt = K.png_case(name)
        assert 0 < sum(c for _, c in M.png_chunks(img, filt))


@pytest.mark.parametrize("name", ["lane_over_64_bits", "window_edge"])
def test_the_accumulator_and_the_window_are_filled(name):
    """one lane packs the most four positions can hold, 66 bits, and its step comes within a few per cent of the 3877 bits a step can put into
    the window (the literal form's edge case stands at 3700 of 3871)"""
    d = K.png_line(name)
    assert M.png_payload(d)[1]  # form (c) is taken: the sweep below is what the kernel emits
    w = K.sweep_model(d)
    print("%s: fullest step %d of %d bits, max nb %d of %d, %d lanes over 64 bits, %d matches" % (name, max(w.steps), K.WINDOW_BITS, w.max_nb, K.LANE_BITS, w.over64, w.matches))
    assert w.max_nb == K.LANE_BITS == 66 and w.over64 >= 1
    assert 3800 <= max(w.steps) <= K.WINDOW_BITS == 3877
    assert int(np.argmax(w.steps)) == (2 if name == "lane_over_64_bits" else 1)  # the step behind the planted match


@pytest.mark.parametrize("name", NAMES)
def test_chunks_decode_and_never_grow(name, driver, tmp_path):
    img, filt = K.png_case(name)
    H, W, ch = img.shape
    lines = R.filtered_rows(img, filt)
    on, off = M.png_chunks(img, filt, True), M.png_chunks(img, filt, False)
    records = []
    for line, (p, c), (q, c0) in zip(lines, on, off):
        assert zlib.decompressobj(-15).decompress(p) == line.tobytes()
        assert not c0 and q == R.payload(line)
        assert len(p) <= len(q) and (len(p) < len(q)) == c and (c or p == q)  # equality implies identical bytes
        if c:  # the project's own inflater takes a whole zlib stream: the wrap's first and last chunk around this one payload
            records.append((b"\x78\x01" + p + b"\x03\x00" + struct.pack(">I", zlib.adler32(line.tobytes()) & 0xFFFFFFFF), line.size))
    for (s, n), line, (code, _, got) in zip(records, [l for l, (_, c) in zip(lines, on) if c], run(driver, tmp_path, records) if records else []):
        assert code == K9_OK and got == line.tobytes()
    want = M.result_prefix_png(img, filt)
    assert M.png_header_of(want)[4:] == (sum(c for _, c in on), 0) and M.png_payloads_of(want) == [p for p, _ in on]
    assert M.result_prefix_png(img, filt, False) == R.result_prefix(img, filt)  # matches off: the bytes of today, the count zero
    assert len(want) <= R.bound(W, H, ch)


@pytest.mark.parametrize("name", ["half_flat_97x55", "half_flat_rgba_paeth_128x72", "ramp_97x55", "constant_5x3", "run_519"])
def test_files_round_trip_and_tiles_wrap_alike(name, tmp_path):
    img, filt = K.png_case(name)
    H, W, ch = img.shape
    for ntiles in (1, 3) if H >= 3 else (1,):
        tiles = tiles_top_first(img, ntiles)
        results = [M.result_prefix_png(t, filt) for t in tiles]
        data = imageio.png_from_fragments(W, H, ch, results)  # the wrap needs no change: a decoder does not care which form a chunk took
        assert data == R.png_file(W, H, ch, results)
        path = tmp_path / ("t%d.png" % ntiles)
        path.write_bytes(data)
        assert np.array_equal(imageio.read_png(str(path)), img)
        if filt in (1, 2):  # no filter looks at the row above: the tiles' fragments are the whole frame's
            assert b"".join(r[32:] for r in results) == M.result_prefix_png(img, filt)[32:]
    if H >= 3 and filt in (1, 2):
        return
    # the identical file from 1 and 3 tiles where the filters of the tiles' first scanlines agree with the whole frame's: forced Sub
    whole = M.result_prefix_png(img, 2)
    parts = [M.result_prefix_png(t, 2) for t in tiles_top_first(img, 3 if H >= 3 else 1)]
    assert imageio.png_from_fragments(W, H, ch, parts) == imageio.png_from_fragments(W, H, ch, [whole])
    assert sum(M.png_header_of(p)[4] for p in parts) == M.png_header_of(whole)[4]


NODE_WRAP = r"""
const fs = require("fs")
const io = require(process.argv[1] + "/imageio")
const [W, H, ch, n] = process.argv.slice(3, 7).map(Number)
const frags = []
for (let k = 0; k < n; k++) frags.push(new Uint8Array(fs.readFileSync(process.argv[2] + "/frag" + k + ".bin")))
fs.writeFileSync(process.argv[2] + "/node.png", io.pngFromFragments(W, H, ch, frags))
"""


@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_wrap_equals_python(tmp_path):
    img, filt = K.png_case("half_flat_97x55")
    H, W, ch = img.shape
    results = [M.result_prefix_png(t, filt) + b"\x55" * 5 for t in tiles_top_first(img, 3)]
    assert sum(M.png_header_of(r)[4] for r in results) > 0
    for k, r in enumerate(results):
        (tmp_path / ("frag%d.bin" % k)).write_bytes(r)
    subprocess.check_call([node, "-e", NODE_WRAP, JS, str(tmp_path), str(W), str(H), str(ch), "3"])
    assert (tmp_path / "node.png").read_bytes() == imageio.png_from_fragments(W, H, ch, results)


# ---------------------------------------------------------------- ABI
def test_match_abi_matches_header(tmp_path):
    proto = tmp_path / "proto.c"  # the prototypes, as the hosts call them (compiled, not linked)
    proto.write_text('#include "rfx.h"\n'
                     "int (*a)(rfx_ctx *, const rfx_export_params *, int, unsigned, void *, size_t, int *) = rfx_stage_png_ex;\n"
                     "int (*b)(rfx_ctx *, const rfx_export_params *, int, unsigned, void *, size_t) = rfx_png_ex;\n"
                     "int (*c)(rfx_ctx *, const rfx_export_params *, unsigned, void *, size_t, int *) = rfx_stage_exr_ex;\n"
                     "int (*d)(rfx_ctx *, const rfx_export_params *, unsigned, void *, size_t) = rfx_exr_ex;\n"
                     "int flag[RFX_ENCODE_MATCHES == 1u ? 1 : -1]; int abi[RFX_ABI_VERSION == %d ? 1 : -1];\n" % abi.RFX_ABI_VERSION)
    subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    lib = abi.load_library()
    for name in ("rfx_stage_png_ex", "rfx_png_ex", "rfx_stage_exr_ex", "rfx_exr_ex"):
        assert name in abi.EXPORTS and hasattr(lib, name)
    assert abi.ENCODE_MATCHES == 1


# ---------------------------------------------------------------- FrameExporter(encode="device", matches=True)
class Recorder:
    """stands in for a Context: records the calls, fills the staged buffer with the restatement's result when the ticket is waited for"""
    W, tile_rows = 16, 8
    has_export_matches = True

    def __init__(self):
        self.calls, self.staged = [], {}

    def png_bound(self, channels=3):
        return R.bound(self.W, self.tile_rows, channels)

    def host_alloc(self, shape, dtype):
        self.calls.append(("host_alloc", tuple(shape), np.dtype(dtype).name))
        return np.zeros(shape, dtype)

    def stage_png(self, source, channels, tonemap, exposure, filter, *, out, matches=False):
        t = len(self.staged) + 1
        self.staged[t] = (out, M.result_prefix_png(K.half_flat_bytes(self.W, self.tile_rows, channels, seed=t), abi.PNG_FILTERS.get(filter, filter), matches))
        self.calls.append(("stage_png", source, channels, filter, matches, t))
        return t

    def export_wait(self, t):
        out, res = self.staged[t]
        out[:len(res)] = np.frombuffer(res, np.uint8)
        self.calls.append(("export_wait", t))


def test_python_frame_exporter_with_matches(tmp_path):
    ctx = Recorder()
    fx = frames.FrameExporter(ctx, str(tmp_path), "png", tonemap="linear", encode="device", matches=True)
    for _ in range(3):
        fx.submit(abi.TEX_FINAL)
    fx.finish()
    n = R.bound(16, 8, 3)
    assert ctx.calls == [("host_alloc", (n,), "uint8")] * 2 + [
        ("stage_png", abi.TEX_FINAL, 3, "adaptive", True, 1), ("stage_png", abi.TEX_FINAL, 3, "adaptive", True, 2), ("export_wait", 1),
        ("stage_png", abi.TEX_FINAL, 3, "adaptive", True, 3), ("export_wait", 2), ("export_wait", 3)]
    for i in range(3):
        assert np.array_equal(imageio.read_png(str(tmp_path / ("frame_%05d.png" % i))), K.half_flat_bytes(16, 8, 3, seed=i + 1))
    with pytest.raises(ValueError, match="matches"):
        frames.FrameExporter(ctx, str(tmp_path), "png", matches=True)  # the host encoder has no such form
    with pytest.raises(ValueError, match="matches"):
        frames.FrameExporter(ctx, str(tmp_path), "exr", matches=True)
    with pytest.raises(ValueError, match="matches"):
        frames.FrameExporter(ctx, str(tmp_path), "pfm", matches=True)
    old = Recorder()
    old.has_export_matches = False  # a library without the symbol
    with pytest.raises(ValueError, match="rfx_stage_png_ex"):
        frames.FrameExporter(old, str(tmp_path), "png", encode="device", matches=True)
    off = frames.FrameExporter(old, str(tmp_path), "png", encode="device")
    assert off.matches is False
    off.submit(abi.TEX_FINAL)
    off.finish()
    assert old.calls[2] == ("stage_png", abi.TEX_FINAL, 3, "adaptive", False, 1)  # the default: the call as it was


# ---------------------------------------------------------------- size
# The match form against zlib's run-length coding (Z_RLE: matches of distance 1 only; one Z_SYNC_FLUSH per scanline, as the Huffman-only test
# of tests/test_png_device_cpu.py frames it) of the same filtered rows: payload bytes / zlib's bytes - 1, at 256 x 144.  Measured (the coder is
# deterministic, so there is no further headroom): right half flat -0.18 % (29 412 bytes against 29 466), lower half a clean ramp +1.15 % (28 150
# against 27 830) — the worse, rounded up to the next
# whole percent.  (zlib's lazy evaluation and its choice among block types find a little more in the ramp's short runs.)
MAX_EXCESS = 0.02


def _size_inputs():
    yield "half_flat-256x144", K.half_flat_bytes(256, 144, 3)
    yield "ramp-256x144", K.ramp_bytes(256, 144, 3)


@pytest.mark.parametrize("name,img", list(_size_inputs()), ids=[n for n, _ in _size_inputs()])
def test_size_against_zlib_rle(name, img):
    lines = R.filtered_rows(img, 0)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    theirs = sum(len(co.compress(l.tobytes()) + co.flush(zlib.Z_SYNC_FLUSH)) for l in lines)
    ours = sum(len(M.png_payload(l)[0]) for l in lines)
    off = sum(len(R.payload(l)) for l in lines)
    print("%s: %d bytes against zlib's %d: excess %+.2f %%; %d without matches; %.3f of raw" % (name, ours, theirs, 100.0 * (ours / theirs - 1.0), off, ours / img.size))
    assert ours <= theirs * (1.0 + MAX_EXCESS)


def test_constant_frame_against_the_literal_form():
    """The constant frame stays out of the comparison with zlib: there zlib switches to fixed-Huffman blocks, which this coder does not have, and
    the dynamic header of every chunk dominates what is left (3 027 bytes against zlib's 2 019 at 256 x 144).  What matches must still do for
    it: at most a quarter of the literal-only size."""
    img = np.full((144, 256, 3), 77, np.uint8)
    lines = R.filtered_rows(img, 0)
    ours, off = sum(len(M.png_payload(l)[0]) for l in lines), sum(len(R.payload(l)) for l in lines)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    theirs = sum(len(co.compress(l.tobytes()) + co.flush(zlib.Z_SYNC_FLUSH)) for l in lines)
    print("constant 256x144: %d bytes with matches, %d without, zlib's Z_RLE %d" % (ours, off, theirs))
    assert 4 * ours <= off
