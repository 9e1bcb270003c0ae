"""CPU (-m "not gpu"): the match form of include/rfx.h "Match form" for EXR fragments without a device — the restatement
(tests/match_device_ref.py) over tests/match_cases.py: every chunk through zlib and through the project's own inflater (csrc/k9_inflate.h),
whole files through imageio.read_exr bit for bit, row tiles, the form choice, match_form_chunks, the hosts' wrap, the premises of the cases,
the FrameExporter's call order and refusals with matches=True, and the size against zlib's Z_RLE coding."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import exr_device_ref as E
import match_cases as K
import match_device_ref as M
from rfx_amd import abi, frames, imageio
from test_exr_device_cpu import NODE_WRAP, read_back, same_halfs
from test_inflate_core_cpu import K9_OK, driver, run  # noqa: F401  (driver: the fixture that builds tests/inflate_core_driver.cpp)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")

NAMES = sorted(K.EXR_CASES)


def test_the_cases_reach_their_edges():
    for m in K.RUN_LENGTHS:
        halfs = K.exr_case("run_%d" % m)
        assert halfs.shape == (1, 300, 4)
        d = K.exr_line("run_%d" % m)
        planted = K.planted(1200, [(s, m, 3) for s in K.run_starts(m)], m)
        assert np.array_equal(d[:1200], planted)  # the low bytes carry the planted sequence; behind it the high bytes' 128s
        assert (d[1201:] == 128).all() and K.repeating(d)[-1] == d.size - 1
        assert K.repeating(d[:1200]).size == m * len(K.run_starts(m))
    d = K.exr_line("run_from_d1")
    assert d[0] == d[1] and K.repeating(d)[0] == 1
    one, two = K.repeating(K.exr_line("run_across_one_step")[:1200]), K.repeating(K.exr_line("run_across_two_steps")[:1200])
    assert one[0] < 256 <= one[-1] < 512 and two[0] < 256 and two[-1] >= 512
    d = K.exr_line("constant_row")
    assert K.repeating(d).size >= d.size - 4  # the low and the high half: two long runs
    assert K.repeating(K.exr_line("no_repeat")).size == 0
    d = K.exr_line("only_match_loses")
    raw = E.raw_blocks(K.exr_case("only_match_loses"))[0]
    c, a = M.exr_data_c(d), E.zlib_stream(d)
    assert c is not None and len(c) >= len(a) and len(a) < len(raw) and M.exr_data(raw) == (a, False)
    raw = E.raw_blocks(K.exr_case("raw_row"))[0]
    assert len(raw) == 8 and M.exr_data_c(E.predict(raw)) is not None and M.exr_data(raw) == (raw, False)
    assert K.exr_line("long_scanline").size == 65544
    for name in ("half_flat_97x55", "half_flat_rgb_128x72", "smooth_97x55"):
        assert 0 < sum(c for _, c in M.exr_chunks(K.exr_case(name)))


@pytest.mark.parametrize("name", ["lane_over_64_bits", "window_edge"])
def test_the_accumulator_and_the_window_are_filled(name):
    d = K.exr_line(name)
    assert M.exr_data(E.raw_blocks(K.exr_case(name))[0])[1]  # form (c) is taken: the sweep below is what the kernel emits
    w = K.sweep_model(d)
    print("%s: fullest step %d of %d bits, max nb %d of %d, %d lanes over 64 bits, %d matches" % (name, max(w.steps), K.WINDOW_BITS, w.max_nb, K.LANE_BITS, w.over64, w.matches))
    assert w.max_nb == K.LANE_BITS == 66 and w.over64 >= 1
    assert 3800 <= max(w.steps) <= K.WINDOW_BITS == 3877
    assert int(np.argmax(w.steps)) == (2 if name == "lane_over_64_bits" else 1)  # the step behind the planted match


@pytest.mark.parametrize("name", NAMES)
def test_chunks_decode_and_never_grow(name, driver, tmp_path):
    halfs = K.exr_case(name)
    H, W, ch = halfs.shape
    n = 2 * W * ch
    raws = E.raw_blocks(halfs)
    on, off = M.exr_chunks(halfs, True), M.exr_chunks(halfs, False)
    records = []
    for raw, (p, c), (q, c0) in zip(raws, on, off):
        assert (p if len(p) == n and not c else imageio._exr_unpredict(zlib.decompress(p))) == raw
        assert not c0 and q == E.data(raw)
        assert len(p) <= len(q) and (len(p) < len(q)) == c and (c or p == q)  # equality implies identical bytes
        assert not c or len(p) < n  # a reader still tells the raw form by size == n
        if c:
            records.append((p, n))
    for (s, _), raw, (code, _, got) in zip(records, [r for r, (_, c) in zip(raws, on) if c], run(driver, tmp_path, records) if records else []):
        assert code == K9_OK and imageio._exr_unpredict(got) == raw  # the project's own inflater
    want = M.result_prefix_exr(halfs, 3)
    head = E.header_of(want)
    assert head[1:4] == (H, 3, H * n) and head[4] == sum(1 for d, c in on if not c and len(d) == n) and head[5] == sum(c for _, c in on)
    assert [d for _, d in E.chunks_of(want)] == [p for p, _ in on]
    assert M.result_prefix_exr(halfs, 3, False) == E.result_prefix(halfs, 3)  # matches off: the bytes of today, the count zero
    assert len(want) <= E.bound(W, H, ch)


@pytest.mark.parametrize("name", ["half_flat_97x55", "half_flat_rgb_128x72", "smooth_97x55", "half_flat_5x3", "run_519"])
def test_files_round_trip_and_tiles_give_the_identical_file(name, tmp_path):
    halfs = K.exr_case(name)
    H, W, ch = halfs.shape
    files = []
    for ntiles in (1, 3) if H >= 3 else (1,):
        results = [M.result_prefix_exr(t, y) for t, y in E.tiles_top_first(halfs, ntiles)]
        files.append(imageio.exr_from_fragments(W, H, ch, results))  # the wrap needs no change: a reader does not care which form a chunk took
        path = tmp_path / ("t%d.exr" % ntiles)
        path.write_bytes(files[-1])
        assert same_halfs(read_back(path, ch), halfs)
    assert all(f == files[0] for f in files)
    off = imageio.exr_from_fragments(W, H, ch, [M.result_prefix_exr(halfs, 0, False)])
    assert len(files[0]) <= len(off)


@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_wrap_equals_python(tmp_path):
    halfs = K.exr_case("half_flat_97x55")
    H, W, ch = halfs.shape
    results = [M.result_prefix_exr(t, y) + b"\x55" * 5 for t, y in E.tiles_top_first(halfs, 3)]
    assert sum(E.header_of(r)[5] for r in results) > 0
    for k, r in enumerate(results):
        (tmp_path / ("frag%d.bin" % k)).write_bytes(r)
    subprocess.check_call([node, "-e", NODE_WRAP, JS, str(tmp_path), str(W), str(H), str(ch), "3"], stdout=subprocess.DEVNULL)
    assert (tmp_path / "node.exr").read_bytes() == imageio.exr_from_fragments(W, H, ch, results)


# ---------------------------------------------------------------- FrameExporter(compression="zips", matches=True)
class Recorder:
    """stands in for a Context: records the calls, fills the staged buffer with the restatement's result when the ticket is waited for"""
    W, tile_rows = 16, 8
    has_export_matches = True

    def __init__(self):
        self.calls, self.staged = [], {}

    def exr_bound(self, channels=4):
        return E.bound(self.W, self.tile_rows, channels)

    def host_alloc(self, shape, dtype):
        self.calls.append(("host_alloc", tuple(shape), np.dtype(dtype).name))
        return np.zeros(shape, dtype)

    def stage_exr(self, source, channels, *, out, matches=False):
        t = len(self.staged) + 1
        self.staged[t] = (out, M.result_prefix_exr(K.half_flat_halfs(self.W, self.tile_rows, channels, seed=t), 0, matches))
        self.calls.append(("stage_exr", source, channels, matches, t))
        return t

    def export_wait(self, t):
        out, res = self.staged[t]
        out[:len(res)] = np.frombuffer(res, np.uint8)
        self.calls.append(("export_wait", t))


def test_python_frame_exporter_with_matches(tmp_path):
    ctx = Recorder()
    fx = frames.FrameExporter(ctx, str(tmp_path), "exr", compression="zips", matches=True)
    for _ in range(3):
        fx.submit(abi.TEX_FINAL)
    fx.finish()
    n = E.bound(16, 8, 4)
    assert ctx.calls == [("host_alloc", (n,), "uint8")] * 2 + [
        ("stage_exr", abi.TEX_FINAL, 4, True, 1), ("stage_exr", abi.TEX_FINAL, 4, True, 2), ("export_wait", 1),
        ("stage_exr", abi.TEX_FINAL, 4, True, 3), ("export_wait", 2), ("export_wait", 3)]
    for i in range(3):
        assert same_halfs(read_back(tmp_path / ("frame_%05d.exr" % i), 4), K.half_flat_halfs(16, 8, 4, seed=i + 1))
    with pytest.raises(ValueError, match="matches"):
        frames.FrameExporter(ctx, str(tmp_path), "exr", matches=True)  # the uncompressed file has no such form
    old = Recorder()
    old.has_export_matches = False  # a library without the symbol
    with pytest.raises(ValueError, match="rfx_stage_png_ex"):
        frames.FrameExporter(old, str(tmp_path), "exr", compression="zips", matches=True)
    off = frames.FrameExporter(old, str(tmp_path), "exr", compression="zips")
    off.submit(abi.TEX_FINAL)
    off.finish()
    assert old.calls[2] == ("stage_exr", abi.TEX_FINAL, 4, False, 1)  # the default: the call as it was


# ---------------------------------------------------------------- size
# The match form against zlib's run-length coding (Z_RLE: matches of distance 1 only; window 15, one one-shot stream per scanline, as the
# Huffman-only test of tests/test_exr_device_cpu.py frames it) of the same predicted scanline, each side storing the raw block when its stream is
# not smaller: stored bytes / zlib's stored bytes - 1, at 256 x 144 x 4.  Measured (the coder is deterministic, so there is no further headroom):
# right half flat +0.23 % (81 186 bytes against 80 997), smooth_noisy_halfs +0.08 % (148 833 against 148 715) — the worse, rounded up to the next
# whole percent.
MAX_EXCESS = 0.01


def _size_inputs():
    yield "half_flat-256x144x4", K.half_flat_halfs(256, 144, 4)
    yield "smooth-256x144x4", E.smooth_noisy_halfs(256, 144, 4)


@pytest.mark.parametrize("name,img", list(_size_inputs()), ids=[n for n, _ in _size_inputs()])
def test_size_against_zlib_rle(name, img):
    ours = theirs = off = 0
    for raw in E.raw_blocks(img):
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        z = co.compress(imageio._exr_predict(raw)) + co.flush()
        theirs += min(len(z), len(raw))
        ours += len(M.exr_data(raw)[0])
        off += len(E.data(raw))
    print("%s: %d bytes against zlib's %d: excess %+.2f %%; %d without matches; %.3f of raw" % (name, ours, theirs, 100.0 * (ours / theirs - 1.0), off, ours / img.nbytes))
    assert ours <= theirs * (1.0 + MAX_EXCESS)


def test_constant_frame_against_the_literal_form():
    """The constant frame stays out of the comparison with zlib: there zlib switches to fixed-Huffman blocks, which this coder does not have, and
    the dynamic header of every chunk dominates what is left.  What matches must still do for it: at most a quarter of the literal-only size."""
    img = np.full((144, 256, 4), 0.5, np.float16)
    ours = sum(len(M.exr_data(raw)[0]) for raw in E.raw_blocks(img))
    off = sum(len(E.data(raw)) for raw in E.raw_blocks(img))
    print("constant 256x144x4: %d bytes with matches, %d without" % (ours, off))
    assert 4 * ours <= off
