"""CPU (-m "not gpu") side of the PIZ device decode (include/rfx.h "EXR blocks with PIZ"): the header against the ctypes mirror,
imageio.exr_aov_layout(..., forms="blocks", piz=True) on scanline, tiled and multi-part PIZ files — every block against the fields the file states
in front of it —, the default still refusing them, the band arithmetic, the table-scratch plan as the library computes it, and a run of
tests/test_gpu_exr_piz.py on the host simulator, so that the entry points and the kernels' logic are exercised where there is no device."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import exr_import_cases as X
from launch_plans import needs_hostsim
from rfx_amd import abi, imageio
from test_exr_blocks_cpu import fields_in_front

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = 33, 70


def test_header_and_ctypes_mirror_agree(tmp_path):
    c = tmp_path / "piz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rfx.h"\n'
                 'size_t (*a)(const rfx_ctx *, const rfx_exr_block_frame *, int, int) = rfx_exr_blocks_piz_stage_bytes;\n'
                 'int (*b)(rfx_ctx *, const rfx_exr_block_frame *, int, int) = rfx_stage_exr_blocks_piz;\n'
                 'int main(){printf("%d %d %d", (int)RFX_EXR_PIZ, (int)RFX_ABI_VERSION, a == 0 || b == 0);return 0;}\n')
    obj = tmp_path / "piz.o"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(obj)])  # (the prototypes are the mirror's)
    text = open(os.path.join(ROOT, "include", "rfx.h")).read()
    assert "enum { RFX_EXR_PIZ = 4 };" in text
    assert abi.EXR_PIZ == 4 == imageio._COMP_PIZ and abi.RFX_ABI_VERSION == 21  # OpenEXR's own number; additive to ABI 21
    lib = abi.load_library()
    for name in ("rfx_stage_exr_blocks_piz", "rfx_exr_blocks_piz_stage_bytes"):
        assert name in abi.EXPORTS and hasattr(lib, name)
    assert lib.rfx_exr_blocks_piz_stage_bytes.restype is C.c_size_t
    assert lib.rfx_stage_exr_blocks_piz.argtypes == lib.rfx_stage_exr_blocks.argtypes and lib.rfx_exr_blocks_piz_stage_bytes.argtypes == lib.rfx_exr_blocks_stage_bytes.argtypes
    assert lib.rfx_abi_version() == 21
    codes = dict((n, int(v)) for n, v in re.findall(r"(K9_E_PIZ_\w+) = (\d+)", open(os.path.join(ROOT, "realism-effects_amd", "csrc", "k9_piz.h")).read()))
    assert sorted(codes.values()) == list(range(15, 24))  # numbered after k9_rle.h's 12 .. 14


def piz_files(tmp_path):
    ch = X.channels(W, H, 5)
    half = {c for c in ch if not c.startswith(("velocity", "depth"))}
    paths = {k: str(tmp_path / (k + ".exr")) for k in ("scanline", "tiled", "multipart")}
    imageio.write_exr(paths["scanline"], ch, "piz", half=half)
    imageio.write_exr(paths["tiled"], ch, "piz", half=half, tiles=(64, 64))
    imageio.write_exr_multipart(paths["multipart"], X.as_parts(ch), "piz", half=True)
    return paths, ch, half


def test_piz_layouts_and_the_default(tmp_path):
    paths, ch, half = piz_files(tmp_path)
    for key, path in paths.items():
        for forms in ("scanline", "blocks"):
            with pytest.raises(imageio.ExrNotStreamable, match="tiled" if (key, forms) == ("tiled", "scanline") else "PIZ"):
                imageio.exr_aov_layout(path, forms=forms)
            with pytest.raises(imageio.ExrNotStreamable):
                imageio.exr_aov_layout(path, forms=forms, piz=False)
        with pytest.raises(ValueError, match="blocks"):
            imageio.exr_aov_layout(path, piz=True)
        data = open(path, "rb").read()
        lay = imageio.exr_aov_layout(path, forms="blocks", piz=True)
        assert lay.chunks is None and (lay.width, lay.height, lay.file_bytes) == (W, H, len(data))
        assert all(comp == abi.EXR_PIZ for comp, _ in lay.parts) and len(lay.parts) == (8 if key == "multipart" else 1)
        multi, tiled = key == "multipart", key == "tiled"
        if tiled:
            assert sorted((int(b["x"]), int(b["y"]), int(b["cols"]), int(b["rows"])) for b in lay.blocks) == [(0, 0, 33, 64), (0, 64, 33, 6)]
        else:
            assert [int(r) for r in lay.blocks["rows"]] == [32, 32, 6] * len(lay.parts)  # a PIZ scanline block: 32 rows, the last one what is left
            assert [int(y) for y in lay.blocks["y"]] == [0, 32, 64] * len(lay.parts) and (lay.blocks["x"] == 0).all() and (lay.blocks["cols"] == W).all()
        texel = [sum(2 if pt == imageio._PT_HALF else 4 for pt, _, _ in chans) for _, chans in lay.parts]
        for b in lay.blocks:
            v = fields_in_front(data, b, multi, tiled)
            assert v[0] == int(b["part"]) and v[-1] == int(b["packed_bytes"]) <= int(b["rows"]) * int(b["cols"]) * texel[int(b["part"])]
            assert (v[1] * 64, v[2] * 64) == (int(b["x"]), int(b["y"])) if tiled else v[1] == int(b["y"])
            # the packed bytes are the block the host decode reads there
            chans = [(None, pt) for pt, _, _ in lay.parts[int(b["part"])][1]]
            blk = data[int(b["offset"]):int(b["offset"] + b["packed_bytes"])]
            raw = int(b["rows"]) * int(b["cols"]) * texel[int(b["part"])]
            assert len(imageio._exr_unpack_block(blk, imageio._COMP_PIZ, chans, int(b["cols"]), int(b["rows"]), raw)) == raw
        assert (lay.blocks["packed_bytes"] < lay.blocks["rows"].astype(np.int64) * lay.blocks["cols"] * np.array(texel)[lay.blocks["part"]]).any()
        assert imageio.exr_aov_layout(data, forms="blocks", piz=True).blocks.tobytes() == lay.blocks.tobytes()  # a path or the bytes
    # a file without a PIZ part: piz=True changes nothing
    z = str(tmp_path / "z.exr")
    imageio.write_exr(z, ch, "zip", half=half, tiles=(16, 16))
    assert imageio.exr_aov_layout(z, forms="blocks", piz=True).blocks.tobytes() == imageio.exr_aov_layout(z, forms="blocks").blocks.tobytes()
    # the limit of rfx.h: tiles of 128 x 128 or more stay on the host
    big = {n: np.zeros((130, 130), np.float32) for n in ch}
    imageio.write_exr(z, big, "piz", half=True, tiles=(128, 128))
    with pytest.raises(imageio.ExrNotStreamable, match="128"):
        imageio.exr_aov_layout(z, forms="blocks", piz=True)
    imageio.write_exr(z, big, "piz", half=True, tiles=(256, 64))
    assert len(imageio.exr_aov_layout(z, forms="blocks", piz=True).blocks) == 3


def test_band_arithmetic(tmp_path):
    """band_blocks — what rfx_exr_blocks_piz_stage_bytes sums, as the device tests check on the library itself — against the row rule restated"""
    paths, _, _ = piz_files(tmp_path)
    for key in ("scanline", "multipart", "tiled"):
        lay = imageio.exr_aov_layout(paths[key], forms="blocks", piz=True)
        for row0, rows in ((0, H), (16, 24), (0, 1), (H - 1, 1), (5, 1), (6, 32), (38, 32)):
            want = [i for i, c in enumerate(lay.blocks) if any(row0 <= H - 1 - y < row0 + rows for y in range(int(c["y"]), int(c["y"] + c["rows"])))]
            got = lay.band_blocks(row0, rows)
            assert got.tobytes() == lay.blocks[want].tobytes()
            assert int(got["packed_bytes"].sum()) == sum(int(lay.blocks[i]["packed_bytes"]) for i in want) > 0
        assert len(lay.band_blocks(0, 6)) == len(lay.parts) and len(lay.band_blocks(0, 7)) == 2 * len(lay.parts)  # scanlines 64 .. 69 are the last block's


_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
class T(ctypes.Structure):
    _fields_ = [(n, ctypes.c_ulonglong) for n in ("rev_bytes", "symbol_bytes", "info_bytes", "slot_bytes", "bytes")]
lib.rfx_internal_exr_piz_tables.argtypes = [ctypes.c_int, ctypes.POINTER(T)]
out = []
for n in json.load(sys.stdin):
    t = T()
    rc = lib.rfx_internal_exr_piz_tables(n, ctypes.byref(t))
    out.append([rc] + [getattr(t, f) for f, _ in T._fields_])
json.dump(out, sys.stdout)
"""


@needs_hostsim
def test_table_scratch_plan_as_built():
    """rfx_launch.h rfx_exr_piz_tables_for as the library computes it: one slot per PIZ stream of the call — 65536 two-byte entries of the reverse
    lookup table, 65537 two-byte sorted symbols rounded up to 256 bytes, 256 bytes of info —, 256-byte aligned; a 4K multi-part frame's 544 blocks"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    from conftest import hostsim_child_env
    env = dict(os.environ, **hostsim_child_env(sim))
    cases = [0, 1, 3, 544, (1 << 23) - 1, 1 << 23, -1]
    p = subprocess.run([sys.executable, "-c", _CHILD, env["RFX_TEST_LIB"]], input=json.dumps(cases), capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    slot = 131072 + 131328 + 256
    for n, (rc, rev, sym, info, per, total) in zip(cases, json.loads(p.stdout)):
        if n < 0 or n >= 1 << 23:
            assert rc != 0
            continue
        assert rc == 0 and (rev, sym, info, per, total) == (131072, 131328, 256, slot, slot * n)
        assert sym >= 2 * 65537 and sym % 256 == 0 and per % 256 == 0
    text = open(os.path.join(ROOT, "realism-effects_amd", "csrc", "k9_exr_import.hip")).read()
    assert "K9_PIZ_TABLE_BYTES" in text  # (what the kernels stride by; k9_piz.h derives it from the same three sizes)


@needs_hostsim
def test_gpu_file_on_the_host_simulator():
    """tests/test_gpu_exr_piz.py with the host simulator's library in place of the device's: the entry points' checks, k9_piz_huf's table build and
    decode wave-wide, k9_piz_planes' cells, the scatter, the status and the Python host, executed here"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    env = {k: v for k, v in os.environ.items() if k not in ("RFX_HOSTSIM", "RFX_TEST_LIB")}
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--hostsim", "-p", "no:cacheprovider", os.path.join(HERE, "test_gpu_exr_piz.py")],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert " passed" in p.stdout and "skipped" not in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]
