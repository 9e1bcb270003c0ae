"""rfx.h "EXR blocks" (rfx_stage_exr_blocks / rfx_exr_blocks_stage_bytes; the kernels: k9_exr_import.hip with k9_rle.h and k9_pxr24.h): tiled parts,
RLE and PXR24, a moved data window.  The reference everywhere is the host decode of the same file — imageio.exr_to_typed_planes + stage_aov on a
second context — and the check is equality of bytes of DEPTH, GBUFFER, VELOCITY and DIRECT_LIGHT: integer work on both sides, nothing to
tolerate.  Every file is written by the library's own writers; each case also asserts, from the packed sizes in the file, that the form it is
named for — compressed blocks, raw blocks, or both — is really in it.  Runs on the device (-m gpu) and on the host simulator (--hostsim)."""
import ctypes as C
import struct

import numpy as np
import pytest

import exr_import_cases as X
import test_gpu_exr_import as T

pytestmark = pytest.mark.gpu

K9_E_RLE_SHORT = 14  # csrc/k9_rle.h


def write_file(tmp_path, W, H, comp, types="half", multi=False, tiles=None, seed=3, noise=False, name="f.exr"):
    """the library writer's file of exr_import_cases.channels -> its path.  types as test_gpu_exr_import.write_base's (multi: "half" | "float")"""
    from rfx_amd import imageio
    ch = X.channels(W, H, seed, noise=noise)
    path = str(tmp_path / name)
    if multi:
        assert types in ("half", "float")
        imageio.write_exr_multipart(path, X.as_parts(ch), comp, half=types == "half", tiles=tiles)
    else:
        half = {"half": True, "float": False, "mixed": {c for c in ch if c.split(".")[0] in T.HALF_LAYERS_MIXED}}[types]
        imageio.write_exr(path, ch, comp, half=half, tiles=tiles)
    return path


def block_slots(W, H, path, ctx_args=()):
    from rfx_amd import imageio
    from rfx_amd.context import Context
    c = Context(W, H, *ctx_args)
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data, forms="blocks")
    c.stage_exr_blocks(data, lay)
    c.stage_flip()
    out = [c.download(t) for t in T._slots()], c.exr_aov_status(), lay
    c.close()
    return out


def raw_sizes(lay):
    texel = np.array([sum(2 if pt == 1 else 4 for pt, _, _ in chans) for _, chans in lay.parts])
    b = lay.blocks
    return b["rows"].astype(np.int64) * b["cols"] * texel[b["part"]]


def forms_in(lay):
    """{"compressed", "raw"}: what the file's blocks are, by OpenEXR's rule (a block whose packed size is its raw size is the raw block)"""
    raw = raw_sizes(lay)
    packed = lay.blocks["packed_bytes"].astype(np.int64)
    assert (packed <= raw).all()  # (the writers never store a stream that is not smaller)
    return ({"raw"} if (packed == raw).any() else set()) | ({"compressed"} if (packed < raw).any() else set())


WANT = {"compressed": {"compressed"}, "raw": {"raw"}, "both": {"compressed", "raw"}}
# (W, H, compression, channel types, multi-part, tiles, noise, the forms that must be in the file)
FILES = [
    (97, 55, "rle", "half", False, (16, 16), False, "both"),       # RLE leaves a few narrow edge tiles raw
    (97, 55, "rle", "mixed", False, None, False, "compressed"),
    (97, 55, "rle", "float", True, (32, 8), False, "compressed"),
    (97, 55, "pxr24", "half", False, (16, 16), False, "compressed"),
    (97, 55, "pxr24", "float", False, None, False, "compressed"),  # 24-bit values: the inflate must give 3 bytes per sample; rows of 97: a carry
    (97, 55, "pxr24", "mixed", False, (32, 8), False, "compressed"),
    (97, 55, "pxr24", "float", True, (64, 64), False, "compressed"),
    (97, 55, "zip", "half", True, (16, 16), False, "compressed"),
    (97, 55, "zip", "mixed", False, (64, 64), False, "compressed"),
    (97, 55, "zips", "float", False, (32, 8), False, "compressed"),
    (97, 55, "none", "mixed", False, (16, 16), False, "raw"),
    (97, 55, "none", "half", True, (32, 8), False, "raw"),
    (33, 17, "rle", "half", True, None, False, "compressed"),
    (33, 17, "rle", "mixed", False, (64, 64), False, "compressed"),  # one tile larger than the frame
    (33, 17, "pxr24", "mixed", False, (16, 16), False, "compressed"),
    (33, 17, "pxr24", "half", True, (32, 8), False, "compressed"),
    (33, 17, "zips", "half", False, (16, 16), False, "compressed"),
    (33, 17, "zip", "float", True, (64, 64), False, "compressed"),
    (33, 17, "rle", "half", False, (16, 16), True, "raw"),           # noise: no RLE stream is smaller
    (33, 17, "pxr24", "float", True, (16, 16), True, "both"),        # noise at 3 of 4 bytes still shrinks; the 1 x 1 corner tiles do not
    (33, 17, "pxr24", "half", True, (16, 16), True, "raw"),
    (1, 1, "rle", "half", False, None, False, "raw"),
    (1, 1, "pxr24", "float", True, None, False, "raw"),
    (1, 1, "zip", "half", False, (16, 16), False, "raw"),
    (64, 1, "rle", "half", False, (32, 8), False, "compressed"),
    (64, 1, "pxr24", "mixed", False, None, False, "compressed"),
    (1, 40, "rle", "float", False, (16, 16), False, "compressed"),
    (1, 40, "pxr24", "half", True, None, False, "compressed"),
    (1, 40, "zips", "mixed", False, (32, 8), False, "compressed"),
]


@pytest.mark.parametrize("W,H,comp,types,multi,tiles,noise,want", FILES, ids=lambda v: str(v).replace(" ", ""))
def test_blocks_decode_equals_host_decode(tmp_path, W, H, comp, types, multi, tiles, noise, want):
    from rfx_amd import imageio
    path = write_file(tmp_path, W, H, comp, types, multi, tiles, noise=noise)
    with pytest.raises(imageio.ExrNotStreamable) if (tiles or comp in ("rle", "pxr24")) else _no_raise():
        imageio.exr_aov_layout(path)  # the scanline form refuses what it refused
    got, status, lay = block_slots(W, H, path)
    assert WANT[want] <= forms_in(lay), "the file holds %s blocks only" % sorted(forms_in(lay))
    if tiles:
        tw, th = tiles
        nparts = len(lay.parts)
        assert len(lay.blocks) == nparts * ((W + tw - 1) // tw) * ((H + th - 1) // th)
        assert {int(v) for v in lay.blocks["cols"]} == {min(tw, W - x) for x in range(0, W, tw)}  # edge tiles are narrower
        assert {int(v) for v in lay.blocks["rows"]} == {min(th, H - y) for y in range(0, H, th)}  # ... and shorter
    assert status == (0, -1, 0)
    T.assert_same(got, T.host_slots(W, H, path), "%dx%d %s" % (W, H, comp))


class _no_raise:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_pxr24_float_blocks_compressed_and_raw(tmp_path):
    """FLOAT channels whose 32 bits are all seeded noise, one part per layer, tiles of 16 x 16 on 33 x 17.  A compressed block holds the floats cut
    to 24 bits, 3 bytes per sample — that, not the raw size, is what its stream must inflate to; a block the writer left raw (the 1 x 1 corner
    tile of every part: 3 n + a zlib frame is not below 4 n bytes) holds whole floats, low byte included."""
    from rfx_amd import imageio
    W, H = 33, 17
    rng = np.random.default_rng(23)
    ch = X.channels(W, H, 6)
    for n in ch:
        bits = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
        bits[(bits & 0x7f800000) == 0x7f800000] ^= 0x00800000  # (no infinity, no NaN)
        ch[n] = bits.view(np.float32)
    ch["depth.Z"] = np.abs(ch["depth.Z"])
    path = str(tmp_path / "f.exr")
    imageio.write_exr_multipart(path, X.as_parts(ch), "pxr24", half=False, tiles=(16, 16))
    got, status, lay = block_slots(W, H, path)
    raw, packed = raw_sizes(lay), lay.blocks["packed_bytes"].astype(np.int64)
    corner = (lay.blocks["cols"] == 1) & (lay.blocks["rows"] == 1)
    assert (packed[corner] == raw[corner]).all() and corner.sum() == len(lay.parts) and (packed[~corner] < raw[~corner]).all()
    kept = imageio.read_exr(path)
    assert any((kept[n][0, W - 1].view(np.uint32) & 255) != 0 for n in kept)  # a raw corner sample (bottom right) with a low byte
    assert all(((kept[n][H - 1, 0].view(np.uint32)) & 255) == 0 for n in kept)  # ... and a compressed one without
    assert status == (0, -1, 0)
    T.assert_same(got, T.host_slots(W, H, path))


def test_multi_part_file_of_tiled_and_scanline_parts(tmp_path):
    from rfx_amd import imageio
    W, H = 97, 55
    ch = X.channels(W, H, 5)
    path = str(tmp_path / "m.exr")
    for comp in ("zip", "rle", "pxr24"):
        imageio.write_exr_multipart(path, X.as_parts(ch), comp, half={"diffuse", "normal", "roughness", "direct"},
                                    tiles={"diffuse": (16, 16), "depth": (32, 8), "velocity": (64, 64), "emissive": (16, 16)})
        got, status, lay = block_slots(W, H, path)
        order = list(X.as_parts(ch))
        whole = lay.blocks["cols"] == W
        assert set(lay.blocks["part"][~whole]) == {order.index(k) for k in ("diffuse", "depth", "velocity", "emissive")}  # (64 < 97: every tiled part has narrow blocks)
        assert "compressed" in forms_in(lay) and status == (0, -1, 0)
        T.assert_same(got, T.host_slots(W, H, path), comp)


def move_data_window(path, dx, dy, W, H):
    """the file with its dataWindow moved by (dx, dy) inside a larger displayWindow-to-be (the box patched as test_what_stays_on_the_host does);
    a scanline chunk states its y in the window's coordinates, so those move with it — a tile's coordinates are relative already"""
    from rfx_amd import imageio
    d = bytearray(open(path, "rb").read())
    lay = imageio.exr_aov_layout(bytes(d), forms="blocks")
    key = b"dataWindow\0box2i\0"
    at = d.index(key) + len(key) + 4
    d[at:at + 16] = struct.pack("<iiii", dx, dy, W - 1 + dx, H - 1 + dy)
    if not struct.unpack("<i", d[4:8])[0] & 0x200:
        for b in lay.blocks:
            o = int(b["offset"]) - 8
            d[o:o + 4] = struct.pack("<i", int(b["y"]) + dy)
    open(path, "wb").write(bytes(d))


@pytest.mark.parametrize("comp,tiles", [("zip", None), ("zip", (16, 16)), ("rle", None), ("pxr24", None), ("pxr24", (32, 8))])
def test_moved_data_window(tmp_path, comp, tiles):
    """the frame is the data window, read_exr's rule: the context has the window's size, block y counts from the window's top"""
    from rfx_amd import imageio
    W, H = 33, 17
    path = write_file(tmp_path, W, H, comp, "mixed", tiles=tiles)
    want = T.host_slots(W, H, path)
    move_data_window(path, 4, 2, W, H)
    with pytest.raises(imageio.ExrNotStreamable, match="dataWindow" if (comp, tiles) == ("zip", None) else None):
        imageio.exr_aov_layout(path)
    got, status, lay = block_slots(W, H, path)
    assert (lay.width, lay.height) == (W, H) and int(lay.blocks["y"].min()) == 0 and status == (0, -1, 0)
    T.assert_same(got, want)
    T.assert_same(got, T.host_slots(W, H, path), "host decode of the moved file")


def test_band_that_cuts_tiles_at_both_edges(tmp_path):
    """tile rows 16 .. 39 of 97 x 55 with a halo of 3: the band's scanlines 15 .. 38 take one row of the tile row 8 .. 15 and seven of 32 .. 39.
    Exactly the blocks with a row inside the band are copied; the rest of the frame is staged by two more calls."""
    from rfx_amd import abi, imageio
    from rfx_amd.context import Context
    W, H, args = 97, 55, (0, 16, 24, 3)
    path = write_file(tmp_path, W, H, "pxr24", "mixed", tiles=(32, 8))
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data, forms="blocks")
    a, b = Context(W, H, *args), Context(W, H, *args)
    assert a.held_rows(abi.TEX_GBUFFER) == (13, 30)
    need = lay.band_blocks(16, 24)
    restated = [i for i, q in enumerate(lay.blocks) if any(16 <= H - 1 - y < 40 for y in range(int(q["y"]), int(q["y"] + q["rows"])))]
    assert need.tobytes() == lay.blocks[restated].tobytes() and sorted(set(int(y) for y in need["y"])) == [8, 16, 24, 32]
    assert a.exr_blocks_stage_bytes(data, lay, 16, 24) == int(need["packed_bytes"].sum()) < int(lay.blocks["packed_bytes"].sum())
    assert a.exr_blocks_stage_bytes(data, lay) == int(lay.blocks["packed_bytes"].sum())
    planes = T.host_planes(path)
    for row0, rows in ((16, 24), (0, 16), (40, 15)):
        a.stage_exr_blocks(data, lay, row0, rows)
        assert a.exr_aov_status()[0] == 0
        b.stage_aov({k: v[row0:row0 + rows] for k, v in planes.items()}, row0, rows)
    a.stage_flip(); b.stage_flip()
    T.assert_same([a.download(t) for t in T._slots()], [b.download(t) for t in T._slots()])
    a.close(); b.close()


def test_tiled_and_scanline_frames_alternate_and_the_areas_grow(tmp_path):
    from rfx_amd import imageio
    from rfx_amd.context import Context
    W, H = 33, 17
    small = write_file(tmp_path, W, H, "zip", "half", tiles=(16, 16), seed=1, name="small.exr")
    large = write_file(tmp_path, W, H, "none", "float", multi=True, seed=2, name="large.exr")
    rle = write_file(tmp_path, W, H, "rle", "mixed", seed=4, name="rle.exr")
    paths = [small, large, rle]
    want = [T.host_slots(W, H, p) for p in paths]
    files = [open(p, "rb").read() for p in paths]
    lays = [imageio.exr_aov_layout(f, forms="blocks") for f in files]
    c = Context(W, H)
    assert c.exr_blocks_stage_bytes(files[0], lays[0]) < c.exr_blocks_stage_bytes(files[1], lays[1])
    for k in range(7):
        c.stage_exr_blocks(files[k % 3], lays[k % 3])
        c.stage_flip()
        assert c.exr_aov_status() == (0, -1, 0)
        T.assert_same([c.download(t) for t in T._slots()], want[k % 3], "flip %d" % k)
    c.close()


def test_old_and_new_entry_points_give_the_same_slots(tmp_path):
    from rfx_amd import imageio
    W, H = 97, 55
    for comp in ("zip", "zips", "none"):
        path = write_file(tmp_path, W, H, comp, "mixed")
        old, status, lay = T.device_slots(W, H, path)
        new, status2, blay = block_slots(W, H, path)
        assert status == status2 == (0, -1, 0)
        assert len(lay.chunks) == len(blay.blocks) and (blay.blocks["x"] == 0).all() and (blay.blocks["cols"] == W).all()
        for f in ("part", "y", "rows", "offset", "packed_bytes"):
            assert (lay.chunks[f] == blay.blocks[f]).all()
        T.assert_same(new, old, comp)


def test_refusals(tmp_path):
    """host-side only: nothing is launched"""
    from rfx_amd import abi, imageio
    from rfx_amd.context import Context
    W, H = 33, 17
    data = open(write_file(tmp_path, W, H, "zip", "half", multi=True, tiles=(16, 16)), "rb").read()
    none = open(write_file(tmp_path, W, H, "none", "half", tiles=(16, 16), name="none.exr"), "rb").read()
    c = Context(W, H)

    def rc(mutate, d=data, row0=0, rows=H):
        lay = imageio.exr_aov_layout(d, forms="blocks")
        mutate(lay)
        f, keep = c._exr_block_frame(d, lay)
        assert c.lib.rfx_exr_blocks_stage_bytes(c._h, C.byref(f), row0, rows) == 0
        r = c.lib.rfx_stage_exr_blocks(c._h, C.byref(f), row0, rows)
        assert r != 0 and b"rfx_stage_exr_blocks" in c.lib.rfx_last_error(c._h)
        return r

    def put(field, k, v):
        return lambda l: l.blocks[field].__setitem__(k, v)

    def drop(k):
        def m(l):
            l.blocks = np.delete(l.blocks, k)
        return m
    E = abi.RFX_EINVAL
    lay = imageio.exr_aov_layout(data, forms="blocks")
    assert c.exr_blocks_stage_bytes(data, lay) > 0 and [int(x) for x in lay.blocks["x"][:3]] == [0, 16, 32]
    assert rc(put("x", 1, 8)) == E                                                   # two overlapping blocks (and a hole behind them)
    assert rc(drop(1)) == E                                                          # a hole in the band
    assert rc(put("x", 2, 32 + 1)) == E                                              # a block past the frame's right edge
    assert rc(lambda l: l.parts.__setitem__(0, (4, l.parts[0][1]))) == E             # compression 4 (PIZ)
    assert rc(put("cols", 0, 0)) == E                                                # cols = 0
    assert rc(put("rows", 0, 0)) == E
    assert rc(put("y", 0, -1)) == E
    assert rc(put("part", 0, 99)) == E
    assert rc(put("offset", 3, len(data) - 2)) == E                                  # a block outside the file bytes
    assert rc(put("packed_bytes", 0, 0)) == E
    assert rc(lambda l: l.blocks["packed_bytes"].__setitem__(0, int(l.blocks["packed_bytes"][0]) - 1), d=none) == E  # NONE: packed size is not the raw size
    assert rc(lambda l: None, rows=H + 1) == E                                       # a band outside DEPTH's rows
    # a hole OUTSIDE the band is no reason to refuse: tile (16, 0) of part 0 covers scanlines 0 .. 15, the band below is scanline 16 alone
    lay = imageio.exr_aov_layout(data, forms="blocks")
    lay.blocks = np.delete(lay.blocks, 1)
    assert c.exr_blocks_stage_bytes(data, lay, 0, 1) == int(lay.band_blocks(0, 1)["packed_bytes"].sum()) > 0
    c.close()


def rle_ops(stream):
    """[(offset, size)] of the runs and literals of an RLE stream"""
    ops, i = [], 0
    while i < len(stream):
        n = 2 if stream[i] < 128 else 1 + 256 - stream[i]
        ops.append((i, n))
        i += n
    assert i == len(stream)
    return ops


def test_status_reports_the_rle_block_whose_last_run_is_cut_off(tmp_path):
    """the one corrupt input sent to a device: a tile's RLE stream without its last run — the expander's bounded "fewer bytes than the block
    holds" end, which tests/test_exr_cores_cpu.py runs under the sanitizers first.  That tile's rectangle reads as not covered, every other texel
    is the clean frame's."""
    from rfx_amd import imageio
    from rfx_amd.context import Context
    W, H = 97, 55
    path = write_file(tmp_path, W, H, "rle", "half", multi=True, tiles=(32, 8))
    clean, status, lay = block_slots(W, H, path)
    assert status == (0, -1, 0)
    data = open(path, "rb").read()
    layers = list(X.as_parts(X.channels(W, H)))
    b = lay.blocks
    victim = int(np.flatnonzero((b["part"] == layers.index("emissive")) & (b["x"] == 32) & (b["y"] == 16))[0])
    assert int(b["packed_bytes"][victim]) < int(raw_sizes(lay)[victim])  # an RLE stream, not a raw block
    stream = data[int(b["offset"][victim]):int(b["offset"][victim] + b["packed_bytes"][victim])]
    lay.blocks["packed_bytes"][victim] = rle_ops(stream)[-1][0]  # the stream ends in front of its last run
    c = Context(W, H)
    c.stage_exr_blocks(data, lay)
    c.stage_flip()
    got, status = [c.download(t) for t in T._slots()], c.exr_aov_status()
    c.close()
    assert status == (1, victim, K9_E_RLE_SHORT)
    rows, cols = slice(H - 24, H - 16), slice(32, 64)  # frame rows of scanlines 16 .. 23
    depth, gbuffer, velocity, direct = got
    assert (depth[rows, cols] == 1.0).all()
    assert (gbuffer[rows, cols].reshape(-1, 4).view(np.uint32) == np.array([0, 0, 0, 0x3f800000], np.uint32)).all()
    assert (velocity[rows, cols].reshape(-1, 4).view(np.uint32) == np.array([0, 0, 0, 0x3f800000], np.uint32)).all()
    keep = np.ones((H, W), bool)
    keep[rows, cols] = False
    for g, w in zip(got, clean):
        assert g[keep].tobytes() == w[keep].tobytes()
    assert direct.tobytes() == clean[3].tobytes()  # (the direct part decoded: its samples are staged as they are)


def test_sequence_and_whole_file_entry_points(tmp_path):
    """Context.stage_exr_frame(decode="device") and frames.ExrSequence take tiled, RLE and PXR24 files on the device now; PIZ stays on the host"""
    from rfx_amd import frames, imageio
    from rfx_amd.context import Context
    W, H = 33, 17
    d = tmp_path / "seq"
    d.mkdir()
    kinds = (("zip", (16, 16)), ("rle", None), ("pxr24", None), ("piz", None), ("pxr24", (32, 8)), ("zips", None))
    half = {c for c in X.channels(1, 1) if c.split(".")[0] in T.HALF_LAYERS_MIXED}
    for i, (comp, tiles) in enumerate(kinds):
        imageio.write_exr(str(d / ("f%02d.exr" % i)), X.channels(W, H, 30 + i), comp, half=half, tiles=tiles)
    c = Context(W, H)
    assert c.has_exr_blocks
    seq = frames.ExrSequence(c, str(d))
    for i in range(len(seq)):
        assert seq.stage(i) == ("host" if kinds[i][0] == "piz" else "device")
        c.stage_flip()
        assert c.exr_aov_status()[0] == 0
        T.assert_same([c.download(t) for t in T._slots()], T.host_slots(W, H, seq.paths[i]), "frame %d" % i)
    for i in (0, 1, 2, 3):
        assert c.stage_exr_frame(seq.paths[i], decode="device") == ("host" if kinds[i][0] == "piz" else "device")
        c.stage_flip()
        T.assert_same([c.download(t) for t in T._slots()], T.host_slots(W, H, seq.paths[i]), "file %d" % i)
    c.close()
