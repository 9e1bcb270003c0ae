"""rfx.h "EXR blocks with PIZ" (rfx_stage_exr_blocks_piz / rfx_exr_blocks_piz_stage_bytes; the kernels: k9_exr_import.hip's k9_piz_huf and
k9_piz_planes on csrc/k9_piz.h): PIZ parts decoded on the device, on request.  The reference everywhere is the host decode of the same file —
imageio.exr_to_typed_planes + stage_aov on a second context — and the check is equality of bytes of DEPTH, GBUFFER, VELOCITY and DIRECT_LIGHT:
integer work on both sides, nothing to tolerate.  Every file is written by the library's own writers, once per module; the tests assert from the
files themselves that they hold what they are meant to: blocks smaller than raw, a block in either wavelet arithmetic, a run escape and a code
longer than the primary table's bits.  Runs on the device (-m gpu) and on the host simulator (--hostsim)."""
import ctypes as C
import struct

import numpy as np
import pytest

import exr_import_cases as X
import test_gpu_exr_import as T

pytestmark = pytest.mark.gpu

K9_E_PIZ_TRUNCATED = 23  # csrc/k9_piz.h
FAST_BITS = 12           # csrc/k9_piz.h K9_PIZ_FAST_BITS
_files = {}


def ramps(W, H):
    """every channel an integer ramp read as a half's bits, (7 i + 9000 k) mod 0x7c00 — finite, non-negative halves —: more than 16384 distinct
    words in a block of 32 rows"""
    from rfx_amd import imageio
    i = np.arange(W * H, dtype=np.int64).reshape(H, W)
    names = [n for v in imageio.AOV_LAYOUT.values() for n in v]
    return {n: ((7 * i + 9000 * k) % 0x7c00).astype(np.uint16).view(np.float16).astype(np.float32) for k, n in enumerate(names)}


def piz_file(tmp_path_factory, key):
    """(path, W, H) of one of the module's files, written on first use"""
    from rfx_amd import imageio
    if key in _files:
        return _files[key]
    W, H, multi, types, tiles, content = {
        "scanline": (97, 70, False, "mixed", None, "standard"),
        "multipart": (33, 17, True, "half", None, "standard"),
        "tiled": (70, 70, False, "float", (64, 64), "standard"),
        "ramps": (97, 70, False, "half", None, "ramps"),
        "band": (97, 55, False, "mixed", None, "standard"),
        "constant": (97, 70, False, "half", None, "constant"),  # every channel one value: run escapes of 255 and nothing else
    }[key]
    path = str(tmp_path_factory.mktemp("piz") / (key + ".exr"))
    ch = ramps(W, H) if content == "ramps" else X.channels(W, H, 7)
    if content == "constant":
        ch = {n: np.full_like(v, v[3, 5] if n != "depth.Z" else 0.25) for n, v in ch.items()}
    if multi:
        imageio.write_exr_multipart(path, X.as_parts(ch), "piz", half=types == "half", tiles=tiles)
    else:
        half = {"half": True, "float": False, "mixed": {c for c in ch if c.split(".")[0] in T.HALF_LAYERS_MIXED}}[types]
        imageio.write_exr(path, ch, "piz", half=half, tiles=tiles)
    _files[key] = (path, W, H)
    return _files[key]


def raw_sizes(lay):
    texel = np.array([sum(2 if pt == 1 else 4 for pt, _, _ in chans) for _, chans in lay.parts])
    b = lay.blocks
    return b["rows"].astype(np.int64) * b["cols"] * texel[b["part"]]


def block_facts(data, lay):
    """per compressed PIZ block of the file: (mx, the longest code, whether a run escape occurs) read from its bytes.  A run escape: the code
    bits are fewer than the words times the shortest code, so some words cost no code of their own."""
    out = []
    for b, raw in zip(lay.blocks, raw_sizes(lay)):
        if lay.parts[int(b["part"])][0] != 4 or int(b["packed_bytes"]) == int(raw):
            continue
        blk = bytes(data[int(b["offset"]):int(b["offset"] + b["packed_bytes"])])
        mn, mxb = struct.unpack_from("<HH", blk, 0)
        bitmap = np.zeros(8192, np.uint8)
        pos = 4
        if mn <= mxb:
            bitmap[mn:mxb + 1] = np.frombuffer(blk, np.uint8, mxb - mn + 1, 4)
            pos += mxb - mn + 1
        bits = np.unpackbits(bitmap)
        mx = int(bits.sum()) - int(bitmap[0] & 1) + 1 - 1  # (value 0 counts whether its bit is set or not)
        im, iM, tlen, nbits, _ = struct.unpack_from("<IIIII", blk, pos + 4)
        tb = int.from_bytes(blk[pos + 24:pos + 24 + tlen], "big")
        at, i, lengths = 8 * tlen, im, []
        while i <= iM:
            at -= 6
            ln = (tb >> at) & 63
            if ln == 63:
                at -= 8
                i += ((tb >> at) & 255) + 6
            elif ln >= 59:
                i += ln - 57
            else:
                lengths += [ln] if ln else []
                i += 1
        out.append((mx, max(lengths), nbits < (int(raw) // 2) * min(lengths)))
    return out


def piz_slots(W, H, path, ctx_args=()):
    from rfx_amd import imageio
    from rfx_amd.context import Context
    c = Context(W, H, *ctx_args)
    assert c.has_exr_piz
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data, forms="blocks", piz=True)
    assert c.exr_blocks_stage_bytes(data, lay) == int(lay.band_blocks()["packed_bytes"].sum())
    c.stage_exr_blocks(data, lay)
    c.stage_flip()
    out = [c.download(t) for t in T._slots()], c.exr_aov_status(), lay, data
    c.close()
    return out


@pytest.mark.parametrize("key", ["scanline", "multipart", "tiled", "ramps", "constant"])
def test_piz_decode_equals_host_decode(tmp_path_factory, key):
    from rfx_amd import imageio
    path, W, H = piz_file(tmp_path_factory, key)
    with pytest.raises(imageio.ExrNotStreamable, match="PIZ"):
        imageio.exr_aov_layout(path, forms="blocks")  # the default refuses what it refused
    got, status, lay, data = piz_slots(W, H, path)
    assert all(comp == 4 for comp, _ in lay.parts)
    packed, raw = lay.blocks["packed_bytes"].astype(np.int64), raw_sizes(lay)
    assert (packed <= raw).all() and (packed < raw).any()
    facts = block_facts(data, lay)
    if key == "scanline":
        assert [int(r) for r in lay.blocks["rows"]] == [32, 32, 6] and (lay.blocks["cols"] == W).all()
        assert all(mx < 16384 for mx, _, _ in facts) and any(longest > FAST_BITS for _, longest, _ in facts)
    if key == "constant":
        assert len(facts) == 3 and all(run for _, _, run in facts)
    if key == "multipart":
        assert len(lay.parts) == 8 and len(lay.blocks) == 8 and (lay.blocks["rows"] == 17).all()
    if key == "tiled":  # the 6 x 6 corner tile cannot shrink: the writer stores it raw, the other three are PIZ streams
        sizes = sorted((int(b["cols"]), int(b["rows"]), bool(p < r)) for b, p, r in zip(lay.blocks, packed, raw))
        assert sizes == [(6, 6, False), (6, 64, True), (64, 6, True), (64, 64, True)]
    if key == "ramps":
        assert any(mx >= 16384 for mx, _, _ in facts), [mx for mx, _, _ in facts]
    assert status == (0, -1, 0)
    T.assert_same(got, T.host_slots(W, H, path), key)


def test_moved_data_window(tmp_path_factory, tmp_path):
    """the frame is the data window: a scanline block states its y in the window's coordinates, so those move with it"""
    from rfx_amd import imageio
    src, W, H = piz_file(tmp_path_factory, "multipart")
    want = T.host_slots(W, H, src)
    d = bytearray(open(src, "rb").read())
    lay = imageio.exr_aov_layout(bytes(d), forms="blocks", piz=True)
    key, at = b"dataWindow\0box2i\0", 0
    for _ in lay.parts:
        at = d.index(key, at) + len(key) + 4
        d[at:at + 16] = struct.pack("<iiii", 4, 2, W - 1 + 4, H - 1 + 2)
    for b in lay.blocks:
        o = int(b["offset"]) - 8
        d[o:o + 4] = struct.pack("<i", int(b["y"]) + 2)
    path = str(tmp_path / "moved.exr")
    open(path, "wb").write(bytes(d))
    got, status, lay2, _ = piz_slots(W, H, path)
    assert (lay2.width, lay2.height) == (W, H) and int(lay2.blocks["y"].min()) == 0 and status == (0, -1, 0)
    T.assert_same(got, want)
    T.assert_same(got, T.host_slots(W, H, path), "host decode of the moved file")


def test_piz_parts_and_zip_parts_in_one_call(tmp_path_factory, tmp_path):
    """The library's writers give a file one compression, so the mix is made in the descriptor, which is all the C ABI sees: the same parts written
    twice, as PIZ and as ZIP, the two files' bytes one behind the other in one buffer, and every other part's compression and blocks taken from
    the PIZ file (their offsets moved behind the ZIP file's bytes)."""
    from rfx_amd import imageio
    from rfx_amd.context import Context
    src, W, H = piz_file(tmp_path_factory, "multipart")
    zpath = str(tmp_path / "zip.exr")
    imageio.write_exr_multipart(zpath, X.as_parts(X.channels(W, H, 7)), "zip", half=True)
    z, p = open(zpath, "rb").read(), open(src, "rb").read()
    zl, pl = imageio.exr_aov_layout(z, forms="blocks"), imageio.exr_aov_layout(p, forms="blocks", piz=True)
    assert [ch for _, ch in zl.parts] == [ch for _, ch in pl.parts]
    odd = [k for k in range(len(zl.parts)) if k & 1]
    moved = pl.blocks[np.isin(pl.blocks["part"], odd)].copy()
    moved["offset"] += len(z)
    blocks = np.concatenate([zl.blocks[~np.isin(zl.blocks["part"], odd)], moved])
    parts = [(4 if k in odd else 3, ch) for k, (_, ch) in enumerate(zl.parts)]
    lay = imageio.ExrAovLayout(W, H, len(z) + len(p), parts, None, zl.planes, blocks)
    assert (moved["packed_bytes"] < raw_sizes(pl)[np.isin(pl.blocks["part"], odd)]).any()
    c = Context(W, H)
    data = np.frombuffer(z + p, np.uint8)
    assert c.exr_blocks_stage_bytes(data, lay) == int(blocks["packed_bytes"].sum())
    c.stage_exr_blocks(data, lay)
    c.stage_flip()
    got, status = [c.download(t) for t in T._slots()], c.exr_aov_status()
    # the same descriptor through the entry point without PIZ: refused, nothing staged
    f, keep = c._exr_block_frame(data, lay)
    assert c.lib.rfx_exr_blocks_stage_bytes(c._h, C.byref(f), 0, H) == 0
    from rfx_amd import abi
    assert c.lib.rfx_stage_exr_blocks(c._h, C.byref(f), 0, H) == abi.RFX_EINVAL
    c.close()
    assert status == (0, -1, 0)
    T.assert_same(got, T.host_slots(W, H, src))


def test_band_that_cuts_a_block_of_32_rows(tmp_path_factory):
    """tile rows 16 .. 39 of 97 x 55 with a halo of 3: the band's scanlines 15 .. 38 cut both PIZ blocks (scanlines 0 .. 31 and 32 .. 54); the bottom
    band needs the second block alone.  Exactly the blocks with a row inside the band are copied; the rest of the frame is staged by two more calls."""
    from rfx_amd import abi, imageio
    from rfx_amd.context import Context
    path, W, H = piz_file(tmp_path_factory, "band")
    args = (0, 16, 24, 3)
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data, forms="blocks", piz=True)
    assert [(int(b["y"]), int(b["rows"])) for b in lay.blocks] == [(0, 32), (32, 23)]
    assert (lay.blocks["packed_bytes"] < raw_sizes(lay)).all()
    a, b = Context(W, H, *args), Context(W, H, *args)
    assert a.held_rows(abi.TEX_GBUFFER) == (13, 30)
    assert a.exr_blocks_stage_bytes(data, lay, 16, 24) == int(lay.band_blocks(16, 24)["packed_bytes"].sum()) == int(lay.blocks["packed_bytes"].sum())
    assert a.exr_blocks_stage_bytes(data, lay, 0, 16) == int(lay.band_blocks(0, 16)["packed_bytes"].sum()) == int(lay.blocks["packed_bytes"][1])
    assert a.exr_blocks_stage_bytes(data, lay, 40, 15) == int(lay.blocks["packed_bytes"][0])
    planes = T.host_planes(path)
    for row0, rows in ((16, 24), (0, 16), (40, 15)):
        a.stage_exr_blocks(data, lay, row0, rows)
        assert a.exr_aov_status()[0] == 0
        b.stage_aov({k: v[row0:row0 + rows] for k, v in planes.items()}, row0, rows)
    a.stage_flip(); b.stage_flip()
    T.assert_same([a.download(t) for t in T._slots()], [b.download(t) for t in T._slots()])
    a.close(); b.close()


def test_status_reports_the_tile_whose_stream_ends_inside_a_code(tmp_path_factory):
    """the one corrupt input sent to a device: hlen of the 64 x 64 tile lowered by two bytes, so that its code bits end before nBits — the
    decoder's bounded "input ends inside a code" end, which tests/test_piz_core_cpu.py runs under the sanitizers first.  That tile's rectangle
    reads as not covered (what stage_aov makes of depth 1 and zeros there), every other texel is the clean frame's."""
    from rfx_amd import imageio
    from rfx_amd.context import Context
    path, W, H = piz_file(tmp_path_factory, "tiled")
    data = bytearray(open(path, "rb").read())
    lay = imageio.exr_aov_layout(bytes(data), forms="blocks", piz=True)
    b = lay.blocks
    victim = int(np.flatnonzero((b["cols"] == 64) & (b["rows"] == 64))[0])
    assert (int(b["x"][victim]), int(b["y"][victim])) == (0, 0) and int(b["packed_bytes"][victim]) < int(raw_sizes(lay)[victim])
    o = int(b["offset"][victim])
    mn, mxb = struct.unpack_from("<HH", data, o)
    at = o + 4 + (mxb - mn + 1 if mn <= mxb else 0)
    (hlen,) = struct.unpack_from("<i", data, at)
    assert at + 4 + hlen == o + int(b["packed_bytes"][victim])
    struct.pack_into("<i", data, at, hlen - 2)
    c = Context(W, H)
    c.stage_exr_blocks(bytes(data), lay)
    c.stage_flip()
    got, status = [c.download(t) for t in T._slots()], c.exr_aov_status()
    c.close()
    assert status == (1, victim, K9_E_PIZ_TRUNCATED)
    planes = {k: v.copy() for k, v in T.host_planes(path).items()}
    for k, v in planes.items():
        v[H - 64:H, 0:64] = 1.0 if k == "depth" else 0.0  # scanlines 0 .. 63 are frame rows H - 64 .. H - 1
    c = Context(W, H)
    c.stage_aov(planes)
    c.stage_flip()
    want = [c.download(t) for t in T._slots()]
    c.close()
    T.assert_same(got, want)
    clean = T.host_slots(W, H, path)
    keep = np.ones((H, W), bool)
    keep[H - 64:H, 0:64] = False
    for g, w in zip(got, clean):
        assert g[keep].tobytes() == w[keep].tobytes()
    assert (got[0][H - 64:H, 0:64] == 1.0).all()


def test_sequence_and_whole_file_entry_points(tmp_path_factory, tmp_path):
    """stage_exr_frame(decode="device", piz=True) and ExrSequence(piz=True) take a PIZ file on the device; the defaults keep it on the host"""
    import shutil
    from rfx_amd import frames
    from rfx_amd.context import Context
    src, W, H = piz_file(tmp_path_factory, "multipart")
    d = tmp_path / "seq"
    d.mkdir()
    shutil.copy(src, str(d / "f00.exr"))
    want = T.host_slots(W, H, src)
    c = Context(W, H)
    assert c.has_exr_piz
    for kw, way in ((dict(), "host"), (dict(piz=False), "host"), (dict(piz=True), "device")):
        assert c.stage_exr_frame(src, decode="device", **kw) == way
        c.stage_flip()
        T.assert_same([c.download(t) for t in T._slots()], want, "stage_exr_frame %r" % kw)
        seq = frames.ExrSequence(c, str(d), **kw)
        assert seq.stage(0) == way
        c.stage_flip()
        if way == "device":
            assert c.exr_aov_status() == (0, -1, 0)
        T.assert_same([c.download(t) for t in T._slots()], want, "ExrSequence %r" % kw)
    assert c.stage_exr_frame(src, piz=True) == "host"  # (decode="host" is the default)
    c.close()
