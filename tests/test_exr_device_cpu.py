"""CPU (-m "not gpu"): the EXR fragment format of include/rfx.h "EXR fragments" without a device — the restatement (tests/exr_device_ref.py)
decoded chunk by chunk by zlib and as a file by imageio.read_exr, the two data forms and the bound, stitched tiles, the hosts' wrap (Python and
Node) against each other, the prototypes, the FrameExporter's call order with compression="zips", and the size of the literal-only coding
against zlib's Huffman-only coding of the same predicted scanlines."""
import functools
import json
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import exr_device_ref as E
import export_cases as X
from rfx_amd import abi, frames, imageio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")


def to_halfs(a, channels):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(a)[..., :channels]).astype(np.float16)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (H, W, channels) float16, read-only"""
    if name == "smooth-97x55x4":
        a = E.smooth_noisy_halfs(97, 55, 4)
    elif name == "smooth-128x72x3":
        a = E.smooth_noisy_halfs(128, 72, 3, seed=2)
    elif name == "random-64x4x4":
        a = E.random_halfs(64, 4, 4, seed=4)
    elif name == "lognormal-128x72x4":
        a = to_halfs(X.linear_input(128, 72, "lognormal"), 4)
    elif name == "specials-97x55x3":
        a = to_halfs(X.f16_input(97, 55), 3)
    elif name == "tiny-5x3x3":
        a = to_halfs(X.f16_edge_input(5, 3), 3)
    else:
        raise ValueError(name)
    a.setflags(write=False)
    return a


CASES = ("smooth-97x55x4", "smooth-128x72x3", "random-64x4x4", "lognormal-128x72x4", "specials-97x55x3", "tiny-5x3x3")


def same_halfs(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


def read_back(path, ch):
    planes = imageio.read_exr(str(path))
    assert sorted(planes) == sorted("RGBA"[:ch]) and set(imageio.exr_channel_types(str(path)).values()) == {"half"}
    return np.stack([planes[c] for c in "RGBA"[:ch]], -1).astype(np.float16)


@pytest.mark.parametrize("name", CASES)
def test_restatement_decodes_to_the_input(name, tmp_path):
    img = case(name)
    H, W, ch = img.shape
    n = 2 * W * ch
    files = []
    for ntiles in (1, 3):
        tiles = E.tiles_top_first(img, ntiles)
        results = [E.result_prefix(t, y) for t, y in tiles]
        y = 0
        for (t, first_y), r in zip(tiles, results):
            nbytes, chunks, fy, raw, raw_chunks, zero = E.header_of(r)
            assert nbytes == len(r) - 32 and chunks == t.shape[0] and fy == first_y == y and raw == chunks * n and zero == 0
            assert len(r) <= E.bound(W, t.shape[0], ch)
            got = E.chunks_of(r)
            assert [c[0] for c in got] == list(range(y, y + chunks))  # one chunk per scanline, top first
            assert raw_chunks == sum(1 for _, d in got if len(d) == n)
            for (_, d), block in zip(got, E.raw_blocks(t)):
                assert len(d) <= n  # no chunk's size exceeds n
                if len(d) == n:
                    assert d == block  # form (b): the raw block itself
                else:
                    assert d[:2] == b"\x78\x01"
                    assert zlib.decompress(d) == imageio._exr_predict(block)  # form (a): zlib verifies the Adler-32
                    assert E.predict(block).tobytes() == imageio._exr_predict(block)
            y += chunks
        data = imageio.exr_from_fragments(W, H, ch, results)
        assert data == imageio.exr_from_fragments(W, H, ch, [np.frombuffer(r + b"\xee" * 7, np.uint8) for r in results])  # slack after the fragment
        path = tmp_path / ("t%d.exr" % ntiles)
        path.write_bytes(data)
        assert same_halfs(read_back(path, ch), img)  # bit for bit, NaNs included
        files.append(data)
    assert files[0] == files[1]  # stitched tilings of 1 and 3 tiles give the identical file


def test_the_case_set_holds_every_form():
    forms = {}
    for name in CASES:
        img = case(name)
        n = 2 * img.shape[1] * img.shape[2]
        r = E.result_prefix(img)
        raw_chunks, chunks = E.header_of(r)[4], E.header_of(r)[1]
        forms[name] = "a" if raw_chunks == 0 else "b" if raw_chunks == chunks else "mixed"
        if forms[name] == "b":
            assert len(r) == E.bound(img.shape[1], img.shape[0], img.shape[2])  # exactly the bound
        assert all(len(d) <= n for _, d in E.chunks_of(r))
    assert forms["smooth-97x55x4"] == "a" and forms["random-64x4x4"] == "b" and forms["lognormal-128x72x4"] == "mixed", forms


def test_a_stream_of_exactly_n_bytes_is_not_taken():
    """form (a) only when STRICTLY smaller: a reader tells the forms apart by size == n"""
    img = case("lognormal-128x72x4")
    for raw in E.raw_blocks(img):
        a = E.zlib_stream(E.predict(raw))
        assert E.data(raw) == (a if len(a) < len(raw) else raw)


def test_file_equals_the_host_writer_for_raw_chunks(tmp_path):
    """every chunk raw: the wrapped file is byte for byte what write_exr(compression="zips") writes when nothing shrinks"""
    img = case("random-64x4x4")
    H, W, ch = img.shape
    path = tmp_path / "host.exr"
    imageio.write_exr(str(path), {n: img[..., k] for k, n in enumerate("RGBA")}, compression="zips", half=True)
    assert path.read_bytes() == imageio.exr_from_fragments(W, H, ch, [E.result_prefix(img)])


def test_wrap_refuses_damaged_fragments():
    img = case("smooth-97x55x4")
    H, W, ch = img.shape
    r = E.result_prefix(img)
    with pytest.raises(ValueError, match="scanlines"):
        imageio.exr_from_fragments(W, H + 1, ch, [r])
    with pytest.raises(ValueError, match="buffer holds"):
        imageio.exr_from_fragments(W, H, ch, [r[:-1]])
    top, bottom = [E.result_prefix(t, y) for t, y in E.tiles_top_first(img, 2)]
    with pytest.raises(ValueError, match="is due"):
        imageio.exr_from_fragments(W, H, ch, [bottom, top])  # top tile first
    with pytest.raises(ValueError, match="channels"):
        imageio.exr_from_fragments(W, H, 2, [r])


# ---------------------------------------------------------------- ABI
def test_exr_prototypes_compile_from_the_header(tmp_path):
    proto = tmp_path / "proto.c"  # the prototypes, as the hosts call them (compiled, not linked)
    proto.write_text('#include "rfx.h"\n'
                     "size_t (*a)(const rfx_ctx *, const rfx_export_params *) = rfx_exr_bound;\n"
                     "int (*b)(rfx_ctx *, const rfx_export_params *, void *, size_t, int *) = rfx_stage_exr;\n"
                     "int (*d)(rfx_ctx *, const rfx_export_params *, void *, size_t) = rfx_exr;\n"
                     "int kinds[RFX_PROF_COUNT_ALL == RFX_PROF_K8 + 1 ? 1 : -1];\n")  # no new profile kind
    subprocess.check_call(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    assert abi.EXR_HEADER_BYTES == E.HEADER_BYTES == 32
    lib = abi.load_library()
    for name in ("rfx_exr_bound", "rfx_stage_exr", "rfx_exr"):
        assert name in abi.EXPORTS and hasattr(lib, name)


NODE_WRAP = r"""
const fs = require("fs")
const io = require(process.argv[1] + "/imageio")
const [W, H, ch, n] = process.argv.slice(3, 7).map(Number)
const frags = []
for (let k = 0; k < n; k++) frags.push(new Uint8Array(fs.readFileSync(process.argv[2] + "/frag" + k + ".bin")))
fs.writeFileSync(process.argv[2] + "/node.exr", io.exrFromFragments(W, H, ch, frags))
let refused = ""
try { io.exrFromFragments(W, H + 1, ch, frags) } catch (e) { refused = String(e.message) }
console.log(JSON.stringify({ refused }))
"""


@pytest.mark.skipif(node is None, reason="node not installed")
@pytest.mark.parametrize("name,ntiles", [("lognormal-128x72x4", 3), ("specials-97x55x3", 1), ("tiny-5x3x3", 1)])
def test_node_wrap_equals_python(name, ntiles, tmp_path):
    img = case(name)
    H, W, ch = img.shape
    results = [E.result_prefix(t, y) + b"\x55" * 5 for t, y in E.tiles_top_first(img, ntiles)]  # slack bytes after the fragment
    for k, r in enumerate(results):
        (tmp_path / ("frag%d.bin" % k)).write_bytes(r)
    got = json.loads(subprocess.check_output([node, "-e", NODE_WRAP, JS, str(tmp_path), str(W), str(H), str(ch), str(ntiles)], text=True).strip().splitlines()[-1])
    assert (tmp_path / "node.exr").read_bytes() == imageio.exr_from_fragments(W, H, ch, results)
    assert "scanlines" in got["refused"]


# ---------------------------------------------------------------- FrameExporter(compression="zips")
class Recorder:
    """stands in for a Context: records the calls, fills the staged buffer with the restatement's result when the ticket is waited for"""
    W, tile_rows = 16, 8

    def __init__(self):
        self.calls, self.staged = [], {}

    def exr_bound(self, channels=4):
        return E.bound(self.W, self.tile_rows, channels)

    def host_alloc(self, shape, dtype):
        self.calls.append(("host_alloc", tuple(shape), np.dtype(dtype).name))
        return np.zeros(shape, dtype)

    def stage_exr(self, source, channels, *, out):
        t = len(self.staged) + 1
        self.staged[t] = (out, E.result_prefix(E.smooth_noisy_halfs(self.W, self.tile_rows, channels, seed=t)))
        self.calls.append(("stage_exr", source, channels, t))
        return t

    def export_wait(self, t):
        out, res = self.staged[t]
        out[:len(res)] = np.frombuffer(res, np.uint8)
        self.calls.append(("export_wait", t))


def test_python_frame_exporter_zips(tmp_path):
    ctx = Recorder()
    fx = frames.FrameExporter(ctx, str(tmp_path), "exr", compression="zips")
    for _ in range(3):
        fx.submit(abi.TEX_FINAL)
    fx.finish()
    n = E.bound(16, 8, 4)
    assert ctx.calls == [("host_alloc", (n,), "uint8")] * 2 + [
        ("stage_exr", abi.TEX_FINAL, 4, 1), ("stage_exr", abi.TEX_FINAL, 4, 2), ("export_wait", 1),
        ("stage_exr", abi.TEX_FINAL, 4, 3), ("export_wait", 2), ("export_wait", 3)]
    for i in range(3):
        assert same_halfs(read_back(tmp_path / ("frame_%05d.exr" % i), 4), E.smooth_noisy_halfs(16, 8, 4, seed=i + 1))
    for fmt in ("png", "pfm"):
        with pytest.raises(ValueError, match="exr"):
            frames.FrameExporter(ctx, str(tmp_path), fmt, compression="zips")
    with pytest.raises(ValueError, match="compression"):
        frames.FrameExporter(ctx, str(tmp_path), "exr", compression="zip")
    with pytest.raises(ValueError, match="png"):
        frames.FrameExporter(ctx, str(tmp_path), "exr", encode="device")  # (stays refused: the switch is `compression`)

    class Plain(Recorder):
        def host_alloc(self, shape, dtype):
            return np.zeros(shape, dtype)

    assert frames.FrameExporter(Plain(), str(tmp_path), "exr").compression == "none"  # the default stays the uncompressed file


# ---------------------------------------------------------------- size
# The literal-only coding against zlib's own Huffman-only coding (Z_HUFFMAN_ONLY, window 15, one one-shot stream per scanline) of the same
# predicted scanline, each side storing the raw block when its stream is not smaller: stored bytes / zlib's stored bytes - 1.  Measured (the
# coder is deterministic, so there is no further headroom): smooth 512x288x4 +0.003 % (658 501 bytes against 658 483; 0.558 of raw), lognormal
# 128x72x4 -0.12 %, uniform_1p2 -0.31 %, uniform_0p01 -0.28 % — the worst, +0.003 %, rounded up to the next whole percent.
MAX_EXCESS = 0.01


def _size_inputs():
    yield "smooth-512x288x4", E.smooth_noisy_halfs(512, 288, 4)
    for fam in X.FAMILIES:
        yield fam + "-128x72x4", to_halfs(X.linear_input(128, 72, fam), 4)


@pytest.mark.parametrize("name,img", list(_size_inputs()), ids=[n for n, _ in _size_inputs()])
def test_size_against_zlib_huffman_only(name, img):
    ours = theirs = 0
    for raw in E.raw_blocks(img):
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        z = co.compress(imageio._exr_predict(raw)) + co.flush()
        theirs += min(len(z), len(raw))
        ours += len(E.data(raw))
    excess = 100.0 * (ours / theirs - 1.0)
    print("%s: %d bytes against zlib's %d: excess %+.2f %%, %.3f of raw" % (name, ours, theirs, excess, ours / img.nbytes))
    assert ours <= theirs * (1.0 + MAX_EXCESS)
