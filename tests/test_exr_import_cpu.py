"""CPU (-m "not gpu") side of the streamed EXR frames (include/rfx.h rfx_stage_exr_aov): imageio.exr_aov_layout on files the library's writers
produce (chunk table, channel -> plane map, the F16 / F32 rule, the missing-alpha rule), what it leaves to the host (ExrNotStreamable), the band
arithmetic of the staged bytes, the header against the ctypes mirror, and a run of tests/test_gpu_exr_import.py on the host simulator, so that
the entry point and the kernels' logic are exercised where there is no device."""
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
    items = ["sizeof(rfx_exr_channel)", "sizeof(rfx_exr_part)", "offsetof(rfx_exr_part, channel)", "sizeof(rfx_exr_chunk)", "offsetof(rfx_exr_chunk, offset)",
             "offsetof(rfx_exr_chunk, packed_bytes)", "sizeof(rfx_exr_frame)", "offsetof(rfx_exr_frame, bytes)", "offsetof(rfx_exr_frame, parts)",
             "offsetof(rfx_exr_frame, chunks)", "offsetof(rfx_exr_frame, part)", "offsetof(rfx_exr_frame, chunk)", "(size_t)RFX_EXR_NONE", "(size_t)RFX_EXR_ZIPS",
             "(size_t)RFX_EXR_ZIP", "(size_t)RFX_EXR_HALF", "(size_t)RFX_EXR_FLOAT", "(size_t)RFX_EXR_PLANE_DEPTH", "(size_t)RFX_EXR_PLANE_DIRECT", "(size_t)RFX_ABI_VERSION",
             "(size_t)RFX_PROF_COUNT", "(size_t)RFX_PROF_K8", "(size_t)RFX_PROF_COUNT_ALL", "(size_t)(RFX_EXR_SKIP + 1)"]
    c = tmp_path / "exr.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rfx.h"\nint main(){size_t v[] = {%s};\n'
                 'for (unsigned i = 0; i < sizeof v / sizeof v[0]; i++) printf("%%zu ", v[i]);\nreturn 0;}\n' % ", ".join(items))
    exe = tmp_path / "exr"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(abi.ExrChannel), C.sizeof(abi.ExrPart), abi.ExrPart.channel.offset, C.sizeof(abi.ExrChunk), abi.ExrChunk.offset.offset,
            abi.ExrChunk.packed_bytes.offset, C.sizeof(abi.ExrFrame), abi.ExrFrame.bytes.offset, abi.ExrFrame.parts.offset, abi.ExrFrame.chunks.offset,
            abi.ExrFrame.part.offset, abi.ExrFrame.chunk.offset, abi.EXR_NONE, abi.EXR_ZIPS, abi.EXR_ZIP, abi.EXR_HALF, abi.EXR_FLOAT,
            abi.AOV_PLANES.index("depth"), abi.AOV_PLANES.index("direct"), 21, 10, 10, 11, abi.EXR_SKIP + 1]  # ABI 21, no new profile kind
    assert got == want
    assert abi.EXR_CHUNK_DTYPE.itemsize == C.sizeof(abi.ExrChunk) and [abi.EXR_CHUNK_DTYPE.fields[n][1] for n in abi.EXR_CHUNK_DTYPE.names] == [
        getattr(abi.ExrChunk, n).offset for n in abi.EXR_CHUNK_DTYPE.names]
    assert (abi.EXR_NONE, abi.EXR_ZIPS, abi.EXR_ZIP) == (imageio._COMP_NONE, imageio._COMP_ZIPS, imageio._COMP_ZIP)  # OpenEXR's own numbers
    assert (abi.EXR_HALF, abi.EXR_FLOAT) == (imageio._PT_HALF, imageio._PT_FLOAT) and tuple(imageio.AOV_LAYOUT) == abi.AOV_PLANES
    lib = abi.load_library()
    for name in ("rfx_stage_exr_aov", "rfx_exr_aov_stage_bytes", "rfx_exr_aov_status"):
        assert name in abi.EXPORTS and hasattr(lib, name)
    assert abi.RFX_ABI_VERSION == 21


def chunk_fields(data, rec, multipart):
    """(part, y, size) as the file states them in front of the packed data the record points at"""
    o = int(rec["offset"])
    if multipart:
        return struct.unpack("<iii", data[o - 12:o])
    return (0,) + struct.unpack("<ii", data[o - 8:o])


@pytest.mark.parametrize("comp,per", [("none", 1), ("zips", 1), ("zip", 16)])
def test_layout_of_a_single_part_file(tmp_path, comp, per):
    ch = X.channels(W, H)
    path = str(tmp_path / "a.exr")
    half = {c for c in ch if not c.startswith(("velocity", "depth"))} - {"emissive.G"}
    imageio.write_exr(path, ch, comp, half=half)
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(path)
    assert (lay.width, lay.height, lay.file_bytes) == (W, H, len(data)) and len(lay.parts) == 1
    code, chans = lay.parts[0]
    assert code == {"none": 0, "zips": 2, "zip": 3}[comp]
    names = sorted(ch)  # the file's channel order
    feeds = {cn: (pi, j) for pi, key in enumerate(imageio.AOV_LAYOUT) for j, cn in enumerate(imageio.AOV_LAYOUT[key])}
    assert chans == [((1 if n in half else 2),) + feeds[n] for n in names]
    # F16 iff every channel of the plane is HALF: the one float channel widens emissive
    assert lay.planes == {k: (len(v), "float" if k in ("velocity", "depth", "emissive") else "half") for k, v in imageio.AOV_LAYOUT.items()}
    ys = list(range(0, H, per))
    assert [int(c["y"]) for c in lay.chunks] == ys and [int(c["rows"]) for c in lay.chunks] == [min(per, H - y) for y in ys]
    for c in lay.chunks:
        part, y, size = chunk_fields(data, c, False)
        assert (part, y, size) == (0, int(c["y"]), int(c["packed_bytes"]))
    row_bytes = sum(W * (2 if n in half else 4) for n in names)
    raw = np.array([int(c["rows"]) * row_bytes for c in lay.chunks])
    assert (lay.chunks["packed_bytes"] == raw).all() if comp == "none" else (lay.chunks["packed_bytes"] < raw).all()
    assert imageio.exr_aov_layout(data).chunks.tobytes() == lay.chunks.tobytes()  # a path or the bytes


def test_layout_of_a_multi_part_file_with_other_names(tmp_path):
    ch = X.channels(W, H)
    parts = X.as_parts(ch)
    del parts["diffuse"]["A"], parts["direct"]["A"], parts["velocity"]
    parts["beauty"] = {c: ch["direct." + c] for c in "RGB"}  # a part no plane names
    parts["depth"] = {"V": ch["depth.Z"]}
    path = str(tmp_path / "m.exr")
    imageio.write_exr_multipart(path, parts, "zip", half={"diffuse", "normal", "beauty"})
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data, {"depth": ("depth.V",)})
    assert [code for code, _ in lay.parts] == [3] * len(parts)
    order = list(parts)
    assert lay.planes == dict(diffuse=(3, "half"), normal=(3, "half"), roughness=(1, "float"), metalness=(1, "float"), emissive=(3, "float"), depth=(1, "float"),
                              direct=(3, "float"))  # no velocity; a missing alpha: three channels
    assert lay.parts[order.index("beauty")][1] == [(1, -1, 0)] * 3 and lay.parts[order.index("depth")][1] == [(2, 6, 0)]
    assert lay.parts[order.index("diffuse")][1] == [(1, 0, 2), (1, 0, 1), (1, 0, 0)]  # B, G, R in the file
    n = (H + 15) // 16
    assert len(lay.chunks) == n * len(parts) and [int(p) for p in lay.chunks["part"]] == [k for k in range(len(parts)) for _ in range(n)]
    for c in lay.chunks:
        assert chunk_fields(data, c, True) == (int(c["part"]), int(c["y"]), int(c["packed_bytes"]))
    with pytest.raises(KeyError):  # a plane with a hole
        imageio.exr_aov_layout(data, {"depth": ("depth.V",), "normal": ("normal.X", "normal.Y", "normal.W")})


def test_band_arithmetic(tmp_path):
    """band_chunks — what rfx_exr_aov_stage_bytes sums, as the device tests check on the library itself — against the row rule restated: a chunk
    is needed when one of its scanlines y has its frame row H - 1 - y inside the band, and its part feeds a plane"""
    ch = X.channels(97, 55)
    parts = X.as_parts(ch)
    parts["beauty"] = {"R": ch["direct.R"]}
    path = str(tmp_path / "m.exr")
    for comp in ("zip", "zips"):
        imageio.write_exr_multipart(path, parts, comp, half=True)
        lay = imageio.exr_aov_layout(path)
        beauty = list(parts).index("beauty")
        for row0, rows in ((0, 55), (16, 24), (0, 1), (54, 1), (7, 16), (38, 17)):
            want = [i for i, c in enumerate(lay.chunks) if c["part"] != beauty and any(row0 <= 55 - 1 - y < row0 + rows for y in range(int(c["y"]), int(c["y"] + c["rows"])))]
            got = lay.band_chunks(row0, rows)
            assert got.tobytes() == lay.chunks[want].tobytes()
            assert int(got["packed_bytes"].sum()) == sum(int(lay.chunks[i]["packed_bytes"]) for i in want) > 0
        assert lay.band_chunks().tobytes() == lay.band_chunks(0, 55).tobytes()


def test_what_stays_on_the_host(tmp_path):
    ch = X.channels(W, H)
    path = str(tmp_path / "a.exr")
    for comp in ("rle", "piz", "pxr24"):
        imageio.write_exr(path, ch, comp, half=True)
        with pytest.raises(imageio.ExrNotStreamable, match=comp.upper()):
            imageio.exr_aov_layout(path)
    imageio.write_exr(path, ch, "zip", half=True, tiles=(16, 16))
    with pytest.raises(imageio.ExrNotStreamable, match="tiled"):
        imageio.exr_aov_layout(path)
    imageio.write_exr(path, ch, "zip", half=True)
    d = open(path, "rb").read()
    at = d.index(b"dataWindow\0box2i\0") + len(b"dataWindow\0box2i\0") + 4
    moved = d[:at] + struct.pack("<iiii", 4, 2, W + 3, H + 1) + d[at + 16:]  # the same size, offset inside a larger display
    with pytest.raises(imageio.ExrNotStreamable, match="dataWindow"):
        imageio.exr_aov_layout(moved)
    assert issubclass(imageio.ExrNotStreamable, ValueError)
    with pytest.raises(ValueError, match="not an OpenEXR"):
        imageio.exr_aov_layout(b"P6 not an exr file")
    imageio.exr_to_typed_planes(path)  # (the host takes every one of them: what decode="device" falls back to)


@needs_hostsim
def test_gpu_file_on_the_host_simulator():
    """tests/test_gpu_exr_import.py with the host simulator's library in place of the device's: the entry point's checks and layout, K9's decode,
    scan, scatter and status, the pack launches behind them and the Python host, executed here"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    env = {k: v for k, v in os.environ.items() if k not in ("RFX_HOSTSIM", "RFX_TEST_LIB")}
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--hostsim", "-p", "no:cacheprovider", os.path.join(HERE, "test_gpu_exr_import.py")],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert " passed" in p.stdout and "skipped" not in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]
