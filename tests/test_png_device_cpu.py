"""CPU (-m "not gpu"): the PNG fragment format of include/rfx.h "PNG fragments" without a device — the restatement (tests/png_device_ref.py)
decoded by zlib and imageio.read_png, its chunks' CRCs, the bound, the stored form, stitched tiles, the hosts' wrap (Python and Node) against
the restatement's, the header's constants against rfx_amd/abi.py, the FrameExporter's call order with encode="device", and the size of the
literal-only coding against zlib's Huffman-only coding of the same filtered rows."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import export_cases as X
import png_device_ref as R
from rfx_amd import abi, frames, imageio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")

CASES = ((5, 3, 3), (97, 55, 4), (128, 72, 3), (97, 55, 3))


def chunks(data):
    """the chunks of a fragment or a file body -> [(tag, payload, stored crc)]"""
    out, pos = [], 0
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        out.append((tag, data[pos + 8:pos + 8 + n], struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]))
        pos += 12 + n
    assert pos == len(data)
    return out


def tiles_top_first(img, n):
    H = img.shape[0]
    edges = [H * k // n for k in range(n + 1)]
    return [img[edges[k]:edges[k + 1]] for k in reversed(range(n))]


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d" % c)
def test_restatement_decodes_to_the_input(case, filt, tmp_path):
    W, H, ch = case
    img = R.noisy_frame(W, H, ch)
    for ntiles in (1, 3):
        tiles = tiles_top_first(img, ntiles)
        results = [R.result_prefix(t, filt) for t in tiles]
        data = R.png_file(W, H, ch, results)
        body = chunks(data[8:])
        assert [c[0] for c in body] == [b"IHDR"] + [b"IDAT"] * (H + 2) + [b"IEND"]  # one chunk per scanline between the two the host adds
        for tag, payload, crc in body:
            assert crc == zlib.crc32(tag + payload) & 0xFFFFFFFF
        # zlib.decompress verifies the combined Adler-32; the stream is the filtered rows, top tile first
        raw = zlib.decompress(b"".join(c[1] for c in body if c[0] == b"IDAT"))
        assert raw == b"".join(l.tobytes() for t in tiles for l in R.filtered_rows(t, filt))
        path = tmp_path / ("t%d.png" % ntiles)
        path.write_bytes(data)
        assert np.array_equal(imageio.read_png(str(path)), img)  # the filters undone
        for t, r in zip(tiles, results):
            assert len(r) <= R.bound(W, t.shape[0], ch)
            n, a, b, rawn, zero = struct.unpack("<QIIQQ", r[:32])
            assert n == len(r) - 32 and rawn == t.shape[0] * (1 + W * ch) and zero == 0
            assert (b << 16) | a == zlib.adler32(b"".join(l.tobytes() for l in R.filtered_rows(t, filt))) & 0xFFFFFFFF
        assert imageio.png_from_fragments(W, H, ch, results) == data  # the Python host's wrap
        assert imageio.png_from_fragments(W, H, ch, [np.frombuffer(r + b"\xee" * 7, np.uint8) for r in results]) == data  # slack after the fragment


def test_forced_filters_and_the_first_scanline():
    img = R.noisy_frame(97, 55, 3)
    for filt, want in ((1, {0}), (2, {1}), (3, {2}), (4, {4})):
        types = [int(l[0]) for l in R.filtered_rows(img, filt)]
        assert types[0] == (1 if filt >= 3 else types[1]) and set(types[1:]) == want
    types = [int(l[0]) for l in R.filtered_rows(img, 0)]
    assert types[0] in (0, 1) and set(types) >= {1, 2, 4}
    flat = np.zeros((4, 8, 3), np.uint8)  # every filter costs 0: the tie goes to None
    assert [int(l[0]) for l in R.filtered_rows(flat, 0)] == [0, 0, 0, 0]


def test_random_bytes_take_the_stored_form_and_the_bound_is_tight():
    rng = np.random.default_rng(3)
    for (W, H, ch) in ((300, 2, 3), (16385, 1, 4)):
        img = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
        frag, _, _, _, payloads = R.fragment(img, 0)
        n = 1 + W * ch
        blocks = (n + 65534) // 65535
        for p in payloads:
            assert len(p) == n + 5 * blocks and p[0] == 0 and struct.unpack("<HH", p[1:5]) == (min(n, 65535), min(n, 65535) ^ 0xFFFF)
        assert 32 + len(frag) == R.bound(W, H, ch)
        assert zlib.decompress(b"\x78\x01" + b"".join(payloads) + b"\x03\x00" + struct.pack(">I", zlib.adler32(
            b"".join(l.tobytes() for l in R.filtered_rows(img, 0))))) == b"".join(l.tobytes() for l in R.filtered_rows(img, 0))


def test_no_payload_exceeds_its_stored_form():
    for img in (R.noisy_frame(128, 72, 3), np.zeros((3, 5, 4), np.uint8), np.random.default_rng(1).integers(0, 256, (6, 40, 3), dtype=np.uint8)):
        n = 1 + img.shape[1] * img.shape[2]
        for filt in range(5):
            for p in R.fragment(img, filt)[4]:
                assert len(p) <= n + 5 * ((n + 65534) // 65535)
                assert len(p) == min(len(R.compressed_payload(np.frombuffer(zlib.decompress(p + b"\x03\x00", -15), np.uint8))), n + 5)


def test_code_lengths_are_optimal_limited_and_complete():
    import heapq
    rng = np.random.default_rng(9)
    for trial in range(60):
        f = rng.integers(0, 40, 257) * (rng.random(257) < rng.random())
        f[256] = 1
        f[0] += 1
        lens = R.code_lengths(f, 15)
        heap = [int(x) for x in f if x]
        heapq.heapify(heap)
        best = 0
        while len(heap) > 1:
            s = heapq.heappop(heap) + heapq.heappop(heap)
            best += s
            heapq.heappush(heap, s)
        assert sum(int(x) * l for x, l in zip(f, lens)) == best  # (none of these is deep enough to meet the limit)
        assert sum(2.0 ** -l for l in lens if l) == 1.0
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for limit in (15, 7):
        lens = R.code_lengths(fib, limit)
        assert max(lens) == limit and min(lens) >= 1 and sum(2.0 ** -l for l in lens) == 1.0
        assert all(lens[i] >= lens[i + 1] for i in range(len(lens) - 1))  # a more frequent symbol never gets the longer code
    assert max(R.code_lengths(fib, 99)) == 29


# ---------------------------------------------------------------- ABI
def test_png_abi_matches_header(tmp_path):
    c = tmp_path / "abi_png.c"
    c.write_text('#include <stdio.h>\n#include "rfx.h"\nint main(){printf("%d %d %d %d %d\\n",(int)RFX_PROF_K7,(int)RFX_PROF_COUNT,(int)RFX_PROF_K8,'
                 "(int)RFX_PROF_COUNT_ALL,RFX_ABI_VERSION);return 0;}\n")
    exe = tmp_path / "abi_png"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    proto = tmp_path / "proto.c"  # the prototypes, as the hosts call them (compiled, not linked)
    proto.write_text('#include "rfx.h"\n'
                     "size_t (*a)(const rfx_ctx *, const rfx_export_params *) = rfx_png_bound;\n"
                     "int (*b)(rfx_ctx *, const rfx_export_params *, int, void *, size_t, int *) = rfx_stage_png;\n"
                     "int (*d)(rfx_ctx *, const rfx_export_params *, int, void *, size_t) = rfx_png;\n"
                     "int (*e)(rfx_ctx *, float *, int *, int) = rfx_profile_read_n;\n")
    subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [abi.PROF_KINDS.index("k7_export"), len(abi.PROF_KINDS), abi.PROF_KINDS_ALL.index("k8_png"), len(abi.PROF_KINDS_ALL), abi.RFX_ABI_VERSION]
    assert got[2] == got[1] and got[3] == got[2] + 1  # appended behind RFX_PROF_COUNT: no earlier kind moved, rfx_profile_read's arrays did not grow
    assert abi.PROF_KINDS_ALL[:len(abi.PROF_KINDS)] == abi.PROF_KINDS
    assert abi.PNG_FILTERS == {"adaptive": 0, "none": 1, "sub": 2, "up": 3, "paeth": 4} and abi.PNG_HEADER_BYTES == R.HEADER_BYTES == 32
    lib = abi.load_library()
    for name in ("rfx_png_bound", "rfx_stage_png", "rfx_png", "rfx_profile_read_n"):
        assert name in abi.EXPORTS and hasattr(lib, name)


NODE_WRAP = r"""
const fs = require("fs")
const r = require(process.argv[1] + "/Renderer")
const io = require(process.argv[1] + "/imageio")
const [W, H, ch, n] = process.argv.slice(3, 7).map(Number)
const frags = []
for (let k = 0; k < n; k++) frags.push(new Uint8Array(fs.readFileSync(process.argv[2] + "/frag" + k + ".bin")))
fs.writeFileSync(process.argv[2] + "/node.png", io.pngFromFragments(W, H, ch, frags))
console.log(JSON.stringify({ filters: r.PNG_FILTERS, all: r.PROF_KINDS_ALL, kinds: r.PROF_KINDS }))
"""


@pytest.mark.skipif(node is None, reason="node not installed")
@pytest.mark.parametrize("case", [(97, 55, 3, 3), (5, 3, 4, 1)], ids=lambda c: "%dx%dx%d-%dtiles" % c)
def test_node_wrap_equals_python(case, tmp_path):
    W, H, ch, ntiles = case
    img = R.noisy_frame(W, H, ch)
    results = [R.result_prefix(t, 0) + b"\x55" * 5 for t in tiles_top_first(img, ntiles)]
    for k, r in enumerate(results):
        (tmp_path / ("frag%d.bin" % k)).write_bytes(r)
    got = json.loads(subprocess.check_output([node, "-e", NODE_WRAP, JS, str(tmp_path), str(W), str(H), str(ch), str(ntiles)], text=True).strip().splitlines()[-1])
    assert (tmp_path / "node.png").read_bytes() == R.png_file(W, H, ch, results)
    assert got["filters"] == abi.PNG_FILTERS and got["all"] == list(abi.PROF_KINDS_ALL) and got["kinds"] == list(abi.PROF_KINDS)


# ---------------------------------------------------------------- FrameExporter(encode="device")
class Recorder:
    """stands in for a Context: records the calls, fills the staged buffer with the restatement's result when the ticket is waited for"""
    W, tile_rows = 16, 8

    def __init__(self):
        self.calls, self.staged = [], {}

    def png_bound(self, channels=3):
        return R.bound(self.W, self.tile_rows, channels)

    def host_alloc(self, shape, dtype):
        self.calls.append(("host_alloc", tuple(shape), np.dtype(dtype).name))
        return np.zeros(shape, dtype)

    def stage_png(self, source, channels, tonemap, exposure, filter, *, out):
        t = len(self.staged) + 1
        self.staged[t] = (out, R.result_prefix(R.noisy_frame(self.W, self.tile_rows, channels, seed=t), abi.PNG_FILTERS.get(filter, filter)))
        self.calls.append(("stage_png", source, channels, tonemap, exposure, filter, t))
        return t

    def export_wait(self, t):
        out, res = self.staged[t]
        out[:len(res)] = np.frombuffer(res, np.uint8)
        self.calls.append(("export_wait", t))


def test_python_frame_exporter_device_encode(tmp_path):
    ctx = Recorder()
    fx = frames.FrameExporter(ctx, str(tmp_path), "png", tonemap="linear", exposure=0.5, encode="device")
    for _ in range(3):
        fx.submit(abi.TEX_FINAL)
    fx.finish()
    n = R.bound(16, 8, 3)
    assert ctx.calls == [("host_alloc", (n,), "uint8")] * 2 + [
        ("stage_png", abi.TEX_FINAL, 3, "linear", 0.5, "adaptive", 1), ("stage_png", abi.TEX_FINAL, 3, "linear", 0.5, "adaptive", 2), ("export_wait", 1),
        ("stage_png", abi.TEX_FINAL, 3, "linear", 0.5, "adaptive", 3), ("export_wait", 2), ("export_wait", 3)]
    for i in range(3):
        assert np.array_equal(imageio.read_png(str(tmp_path / ("frame_%05d.png" % i))), R.noisy_frame(16, 8, 3, seed=i + 1))
    with pytest.raises(ValueError, match="png"):
        frames.FrameExporter(ctx, str(tmp_path), "exr", encode="device")
    with pytest.raises(ValueError, match="encode"):
        frames.FrameExporter(ctx, str(tmp_path), "png", encode="gpu")
    assert frames.FrameExporter(ctx, str(tmp_path)).encode == "host"  # the default stays the host encoder


# ---------------------------------------------------------------- size
# The literal-only coding against zlib's own Huffman-only coding (Z_HUFFMAN_ONLY, one Z_SYNC_FLUSH per scanline) of the same filtered rows:
# payload bytes / zlib's bytes - 1.  Measured (the coder is deterministic, so there is no further headroom): noisy 512x288 -0.27 %,
# lognormal 128x72 -1.27 %, uniform_1p2 -1.27 %, uniform_0p01 -0.86 % — the worst, -0.27 %, rounded up to the next whole percent.
MAX_EXCESS = 0.00


def _size_inputs():
    yield "noisy-512x288", R.noisy_frame(512, 288)
    for fam in X.FAMILIES:
        yield fam + "-128x72", imageio.tonemap(X.linear_input(128, 72, fam), "aces", 1.0)


@pytest.mark.parametrize("name,img", list(_size_inputs()), ids=[n for n, _ in _size_inputs()])
def test_size_against_zlib_huffman_only(name, img):
    lines = R.filtered_rows(img, 0)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    theirs = sum(len(co.compress(l.tobytes()) + co.flush(zlib.Z_SYNC_FLUSH)) for l in lines)
    ours = sum(len(R.payload(l)) for l in lines)
    print("%s: %d bytes against zlib's %d: excess %+.2f %%, %.3f of raw" % (name, ours, theirs, 100.0 * (ours / theirs - 1.0), ours / img.size))
    assert ours <= theirs * (1.0 + MAX_EXCESS)
