"""CPU (-m "not gpu") side of the EXR blocks (include/rfx.h rfx_stage_exr_blocks): the header against the ctypes mirror, imageio.exr_aov_layout(...,
forms="blocks") on tiled, RLE, PXR24 and moved-data-window files the library's writers produce — every block's rectangle against the fields the
file states in front of it —, level 0 of a mip-mapped part, the scanline default still refusing each of them, the band arithmetic, and a run of
tests/test_gpu_exr_blocks.py on the host simulator, so that the entry point and the kernels' logic are exercised where there is no device."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import exr_import_cases as X
from launch_plans import needs_hostsim
from rfx_amd import abi, imageio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = 33, 17


def test_header_and_ctypes_mirror_agree(tmp_path):
    items = ["sizeof(rfx_exr_block)", "offsetof(rfx_exr_block, x)", "offsetof(rfx_exr_block, y)", "offsetof(rfx_exr_block, cols)", "offsetof(rfx_exr_block, rows)",
             "offsetof(rfx_exr_block, offset)", "offsetof(rfx_exr_block, packed_bytes)", "sizeof(rfx_exr_block_frame)", "offsetof(rfx_exr_block_frame, bytes)",
             "offsetof(rfx_exr_block_frame, parts)", "offsetof(rfx_exr_block_frame, blocks)", "offsetof(rfx_exr_block_frame, part)", "offsetof(rfx_exr_block_frame, block)",
             "(size_t)RFX_EXR_RLE", "(size_t)RFX_EXR_PXR24", "(size_t)RFX_ABI_VERSION", "(size_t)RFX_PROF_COUNT"]
    c = tmp_path / "blocks.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rfx.h"\nint main(){size_t v[] = {%s};\n'
                 'for (unsigned i = 0; i < sizeof v / sizeof v[0]; i++) printf("%%zu ", v[i]);\nreturn 0;}\n' % ", ".join(items))
    exe = tmp_path / "blocks"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    B, F = abi.ExrBlock, abi.ExrBlockFrame
    want = [C.sizeof(B), B.x.offset, B.y.offset, B.cols.offset, B.rows.offset, B.offset.offset, B.packed_bytes.offset, C.sizeof(F), F.bytes.offset, F.parts.offset,
            F.blocks.offset, F.part.offset, F.block.offset, abi.EXR_RLE, abi.EXR_PXR24, 21, 10]  # still ABI 21, no new profile kind
    assert got == want
    assert abi.EXR_BLOCK_DTYPE.itemsize == C.sizeof(B) and [abi.EXR_BLOCK_DTYPE.fields[n][1] for n in abi.EXR_BLOCK_DTYPE.names] == [
        getattr(B, n).offset for n in abi.EXR_BLOCK_DTYPE.names]
    assert (abi.EXR_RLE, abi.EXR_PXR24) == (imageio._COMP_RLE, imageio._COMP_PXR24)  # OpenEXR's own numbers
    lib = abi.load_library()
    for name in ("rfx_stage_exr_blocks", "rfx_exr_blocks_stage_bytes"):
        assert name in abi.EXPORTS and hasattr(lib, name)
    assert abi.RFX_ABI_VERSION == 21 and lib.rfx_abi_version() == 21


def fields_in_front(data, rec, multipart, tiled):
    """what the file states in front of the packed data a record points at: (part, tile x, tile y, level x, level y, size) or (part, y, size)"""
    o = int(rec["offset"])
    n = (5 if tiled else 2) + (1 if multipart else 0)
    v = struct.unpack("<%di" % n, data[o - 4 * n:o])
    return v if multipart else (0,) + v


@pytest.mark.parametrize("comp", ["none", "rle", "zips", "zip", "pxr24"])
@pytest.mark.parametrize("tiles", [(16, 16), (32, 8), (64, 64)])
def test_layout_of_a_tiled_file(tmp_path, comp, tiles):
    ch = X.channels(W, H)
    path = str(tmp_path / "t.exr")
    half = {c for c in ch if not c.startswith(("velocity", "depth"))}
    imageio.write_exr(path, ch, comp, half=half, tiles=tiles)
    with pytest.raises(imageio.ExrNotStreamable):
        imageio.exr_aov_layout(path)
    with pytest.raises(imageio.ExrNotStreamable):
        imageio.exr_aov_layout(path, forms="scanline")
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(path, forms="blocks")
    assert lay.chunks is None and (lay.width, lay.height, lay.file_bytes) == (W, H, len(data))
    assert lay.parts[0][0] == {"none": 0, "rle": 1, "zips": 2, "zip": 3, "pxr24": 5}[comp]
    assert lay.planes == {k: (len(v), "float" if k in ("velocity", "depth") else "half") for k, v in imageio.AOV_LAYOUT.items()}
    tw, th = tiles
    ntx, nty = (W + tw - 1) // tw, (H + th - 1) // th
    assert len(lay.blocks) == ntx * nty
    texel = sum(2 if n in half else 4 for n in ch)
    for b in lay.blocks:
        _, tx, ty, lx, ly, size = fields_in_front(data, b, False, True)
        assert (lx, ly) == (0, 0) and (int(b["x"]), int(b["y"])) == (tx * tw, ty * th) and size == int(b["packed_bytes"])
        assert (int(b["cols"]), int(b["rows"])) == (min(tw, W - tx * tw), min(th, H - ty * th))  # edge tiles are narrower and shorter
        assert size <= int(b["cols"]) * int(b["rows"]) * texel
    cover = np.zeros((H, W), int)
    for b in lay.blocks:
        cover[b["y"]:b["y"] + b["rows"], b["x"]:b["x"] + b["cols"]] += 1
    assert (cover == 1).all()
    assert imageio.exr_aov_layout(data, forms="blocks").blocks.tobytes() == lay.blocks.tobytes()  # a path or the bytes


@pytest.mark.parametrize("comp,per", [("rle", 1), ("pxr24", 16), ("zip", 16)])
def test_layout_of_scanline_parts_as_blocks(tmp_path, comp, per):
    ch = X.channels(W, H)
    path = str(tmp_path / "m.exr")
    imageio.write_exr_multipart(path, X.as_parts(ch), comp, half={"diffuse", "normal"})
    if comp != "zip":
        with pytest.raises(imageio.ExrNotStreamable, match=comp.upper()):
            imageio.exr_aov_layout(path)
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data, forms="blocks")
    n = (H + per - 1) // per
    assert len(lay.blocks) == n * len(lay.parts) and (lay.blocks["x"] == 0).all() and (lay.blocks["cols"] == W).all()
    for b in lay.blocks:
        part, y, size = fields_in_front(data, b, True, False)
        assert (part, y, size) == (int(b["part"]), int(b["y"]), int(b["packed_bytes"])) and int(b["rows"]) == min(per, H - y)
    if comp == "zip":  # the same records as the scanline form's
        old = imageio.exr_aov_layout(data)
        assert all((old.chunks[f] == lay.blocks[f]).all() for f in ("part", "y", "rows", "offset", "packed_bytes")) and old.planes == lay.planes


def test_layout_of_a_multi_part_file_of_tiled_and_scanline_parts(tmp_path):
    ch = X.channels(W, H)
    parts = X.as_parts(ch)
    path = str(tmp_path / "m.exr")
    imageio.write_exr_multipart(path, parts, "zip", half=True, tiles={"normal": (16, 16), "depth": (32, 8)})
    with pytest.raises(imageio.ExrNotStreamable, match="tiledimage"):
        imageio.exr_aov_layout(path)
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data, forms="blocks")
    order = list(parts)
    for k, name in enumerate(order):
        mine = lay.blocks[lay.blocks["part"] == k]
        tile = {"normal": (16, 16), "depth": (32, 8)}.get(name)
        assert len(mine) == (((W + tile[0] - 1) // tile[0]) * ((H + tile[1] - 1) // tile[1]) if tile else (H + 15) // 16)
        for b in mine:
            v = fields_in_front(data, b, True, bool(tile))
            assert v[0] == k and v[-1] == int(b["packed_bytes"])
            assert (int(b["x"]), int(b["y"])) == ((v[1] * tile[0], v[2] * tile[1]) if tile else (0, v[1]))
    want = imageio.read_exr(path)  # (the host reader takes the same file)
    assert sorted(want) == sorted(ch)


def mip_mapped(data):
    """a ONE_LEVEL tiled single-part file -> the same with tile mode MIPMAP_LEVELS (round down): the header's mode byte, the longer offset table,
    and one tile of zeros for every tile of the levels above 0 behind the level-0 tiles"""
    attrs, table_pos = imageio._exr_parse_header(data, 8)
    lay = imageio._exr_part_layout("t", attrs, True)
    n0 = lay["level0_chunks"]
    at = data.index(b"tiles\0tiledesc\0") + len(b"tiles\0tiledesc\0") + 4 + 8
    assert data[at] == 0
    head = data[:at] + b"\x01" + data[at + 1:table_pos]
    attrs2, _ = imageio._exr_parse_header(head + b"\0", 8)
    total = imageio._exr_part_layout("t", attrs2, True)["chunks"]
    assert total > n0
    offs = [o + 8 * (total - n0) for o in struct.unpack("<%dQ" % n0, data[table_pos:table_pos + 8 * n0])]
    body, extra, pos = data[table_pos + 8 * n0:], b"", len(data) + 8 * (total - n0)
    w, h, level = lay["W"], lay["H"], 0
    while not (w == 1 and h == 1):
        w, h, level = max(1, w // 2), max(1, h // 2), level + 1
        for ty in range((h + lay["th"] - 1) // lay["th"]):
            for tx in range((w + lay["tw"] - 1) // lay["tw"]):
                offs.append(pos + len(extra))
                extra += struct.pack("<iiiii", tx, ty, level, level, 4) + b"\0\0\0\0"
    assert len(offs) == total
    return head + struct.pack("<%dQ" % total, *offs) + body + extra, n0


def test_level_0_of_a_mip_mapped_file(tmp_path):
    ch = X.channels(W, H)
    path = str(tmp_path / "t.exr")
    imageio.write_exr(path, ch, "zip", half=True, tiles=(16, 16))
    one = open(path, "rb").read()
    mip, n0 = mip_mapped(one)
    a, b = imageio.exr_aov_layout(one, forms="blocks"), imageio.exr_aov_layout(mip, forms="blocks")
    assert len(b.blocks) == n0 == len(a.blocks) and b.file_bytes == len(mip) > len(one)
    for f in ("part", "x", "y", "cols", "rows", "packed_bytes"):
        assert (a.blocks[f] == b.blocks[f]).all()
    assert all(mip[int(q["offset"]):int(q["offset"] + q["packed_bytes"])] == one[int(p["offset"]):int(p["offset"] + p["packed_bytes"])] for p, q in zip(a.blocks, b.blocks))
    mpath = str(tmp_path / "mip.exr")
    open(mpath, "wb").write(mip)
    want, got = imageio.read_exr(path), imageio.read_exr(mpath)
    assert all(want[k].tobytes() == got[k].tobytes() for k in want)
    # a table whose first entries are not level 0 is refused, as the host reader refuses it
    o = int(b.blocks["offset"][1])
    bad = mip[:o - 12] + struct.pack("<ii", 1, 1) + mip[o - 4:]
    with pytest.raises(ValueError, match="level 0"):
        imageio.exr_aov_layout(bad, forms="blocks")
    # rip-maps stay refused as on the host
    at = mip.index(b"tiles\0tiledesc\0") + len(b"tiles\0tiledesc\0") + 4 + 8
    with pytest.raises(ValueError, match="rip-mapped"):
        imageio.exr_aov_layout(mip[:at] + b"\x02" + mip[at + 1:], forms="blocks")


def test_moved_data_window_and_what_still_stays_on_the_host(tmp_path):
    ch = X.channels(W, H)
    path = str(tmp_path / "a.exr")
    imageio.write_exr(path, ch, "zip", half=True, tiles=(16, 16))
    d = open(path, "rb").read()
    at = d.index(b"dataWindow\0box2i\0") + len(b"dataWindow\0box2i\0") + 4
    moved = d[:at] + struct.pack("<iiii", 4, 2, W + 3, H + 1) + d[at + 16:]  # the same size, offset inside a larger display
    a, b = imageio.exr_aov_layout(d, forms="blocks"), imageio.exr_aov_layout(moved, forms="blocks")
    assert (b.width, b.height) == (W, H) and a.blocks.tobytes() == b.blocks.tobytes()  # tiles are relative to the window's origin
    imageio.write_exr(path, ch, "zip", half=True)
    d = open(path, "rb").read()
    moved = d[:at] + struct.pack("<iiii", 4, 2, W + 3, H + 1) + d[at + 16:]
    with pytest.raises(imageio.ExrNotStreamable, match="dataWindow"):
        imageio.exr_aov_layout(moved)
    b = imageio.exr_aov_layout(moved, forms="blocks")
    assert [int(y) for y in b.blocks["y"]] == [-2, 14]  # a scanline chunk's y is the file's, relative to dataWindow.y0 (this patched file did not move its chunks)
    # PIZ, UINT channels, deep data, parts of different data windows: ExrNotStreamable in either form
    imageio.write_exr(path, ch, "piz", half=True)
    for forms in ("scanline", "blocks"):
        with pytest.raises(imageio.ExrNotStreamable, match="PIZ"):
            imageio.exr_aov_layout(path, forms=forms)
    imageio.write_exr(path, ch, "zip", half=True)
    d = open(path, "rb").read()
    k = d.index(b"depth.Z\0") + 8
    with pytest.raises(imageio.ExrNotStreamable, match="UINT"):
        imageio.exr_aov_layout(d[:k] + struct.pack("<i", 0) + d[k + 4:], forms="blocks")
    with pytest.raises(imageio.ExrNotStreamable, match="deep"):
        imageio.exr_aov_layout(d[:4] + struct.pack("<i", 2 | 0x800) + d[8:], forms="blocks")
    imageio.write_exr_multipart(path, X.as_parts(ch), "zip", half=True)
    d = open(path, "rb").read()
    at = d.index(b"dataWindow\0box2i\0", d.index(b"dataWindow\0box2i\0") + 1) + len(b"dataWindow\0box2i\0") + 4  # the second part's
    with pytest.raises(imageio.ExrNotStreamable, match="different data windows"):
        imageio.exr_aov_layout(d[:at] + struct.pack("<iiii", 4, 2, W + 3, H + 1) + d[at + 16:], forms="blocks")
    with pytest.raises(ValueError, match="forms"):
        imageio.exr_aov_layout(d, forms="tiles")


def test_band_arithmetic(tmp_path):
    """band_blocks — what rfx_exr_blocks_stage_bytes sums, as the device tests check on the library itself — against the row rule restated: a
    block is needed when one of its rows y has its frame row H - 1 - y inside the band, and its part feeds a plane"""
    ch = X.channels(97, 55)
    parts = X.as_parts(ch)
    parts["beauty"] = {"R": ch["direct.R"]}
    path = str(tmp_path / "m.exr")
    for comp, tiles in (("zip", (32, 8)), ("rle", {"diffuse": (16, 16), "beauty": (16, 16)}), ("pxr24", None)):
        imageio.write_exr_multipart(path, parts, comp, half=True, tiles=tiles)
        lay = imageio.exr_aov_layout(path, forms="blocks")
        beauty = list(parts).index("beauty")
        for row0, rows in ((0, 55), (16, 24), (0, 1), (54, 1), (7, 16), (38, 17)):
            want = [i for i, c in enumerate(lay.blocks) if c["part"] != beauty and any(row0 <= 55 - 1 - y < row0 + rows for y in range(int(c["y"]), int(c["y"] + c["rows"])))]
            got = lay.band_blocks(row0, rows)
            assert got.tobytes() == lay.blocks[want].tobytes()
            assert int(got["packed_bytes"].sum()) == sum(int(lay.blocks[i]["packed_bytes"]) for i in want) > 0
        assert lay.band_blocks().tobytes() == lay.band_blocks(0, 55).tobytes()


def test_multipart_writer_tiles_round_trip(tmp_path):
    """write_exr_multipart(tiles=): the host reader gives back the pixels, for every compression"""
    ch = X.channels(W, H)
    path = str(tmp_path / "m.exr")
    for comp in ("none", "rle", "zips", "zip", "piz", "pxr24"):
        imageio.write_exr_multipart(path, X.as_parts(ch), comp, half=True, tiles=(16, 16))
        got = imageio.read_exr(path)
        assert all(got[k].tobytes() == ch[k].astype(np.float16).astype(np.float32).tobytes() for k in ch), comp


@needs_hostsim
def test_gpu_file_on_the_host_simulator():
    """tests/test_gpu_exr_blocks.py with the host simulator's library in place of the device's: the entry point's checks and coverage rule, K9's
    inflate, RLE expander, PXR24 scan, scatter with geometry and status, the pack launches behind them and the Python host, executed here"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    env = {k: v for k, v in os.environ.items() if k not in ("RFX_HOSTSIM", "RFX_TEST_LIB")}
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--hostsim", "-p", "no:cacheprovider", os.path.join(HERE, "test_gpu_exr_blocks.py")],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert " passed" in p.stdout and "skipped" not in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]
