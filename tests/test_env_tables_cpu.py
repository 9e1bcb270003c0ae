"""CPU (-m "not gpu") side of the environment kept on the device (include/rfx.h "the environment kept on the device"): the header against the
ctypes mirror, and K10's arithmetic — csrc/k10_env_tables.h, the statements the kernels run — in a stand-alone program built under
AddressSanitizer + UBSan with exact-sized buffers, bit for bit against rfx_amd.envmap.build_importance on every case of tests/env_cases.py and on
the golden MIS frame's environment, whose tables the reference's own worker code produced."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import env_cases as E
import golden_util as G
from launch_plans import needs_hostsim
from rfx_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "realism-effects_amd", "csrc")


def test_header_and_ctypes_mirror_agree(tmp_path):
    c = tmp_path / "env.c"
    c.write_text('#include <stdio.h>\n#include "rfx.h"\n'
                 'int (*a)(rfx_ctx *, const float *, int, int, int, int) = rfx_set_environment_cube;\n'
                 'int (*b)(rfx_ctx *, int) = rfx_build_environment_importance;\n'
                 'int (*d)(rfx_ctx *, float *, float *, double *, float *, float *) = rfx_download_environment_importance;\n'
                 'int main(){printf("%d %d", (int)RFX_ABI_VERSION, a == 0 || b == 0 || d == 0);return 0;}\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "env.o")])
    lib = abi.load_library()
    for name in ("rfx_set_environment_cube", "rfx_build_environment_importance", "rfx_download_environment_importance"):
        assert name in abi.EXPORTS and hasattr(lib, name)
    assert abi.RFX_ABI_VERSION == 21 == lib.rfx_abi_version()  # additive: the number stands
    assert lib.rfx_download_environment_importance.argtypes[3] == C.POINTER(C.c_double)
    mk = open(os.path.join(CSRC, "sources.mk")).read()  # one word in the list, uncontracted: the order of K10's roundings is its contract
    assert "k10_env_tables" in mk.split("RFX_STEMS :=")[1].split("\n\n")[0].split() and "k10_env_tables" not in mk.split("RFX_CONTRACTED :=")[1].split()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k10") / "env_tables_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC, os.path.join(HERE, "env_tables_driver.cpp"), "-o", exe])
    return exe


def run_driver(driver, tmp_path, cases):
    """cases: (stored texels (H, W, 4), flip) -> [(marginal, conditional, total, whole, decimal)], the program run directly, nothing preloaded"""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for t, flip in cases:
            f.write(struct.pack("<3i", t.shape[1], t.shape[0], int(flip)))
            f.write(np.ascontiguousarray(t, "<f4").tobytes())
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    p = subprocess.run([driver, src, dst], capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    raw, at, out = open(dst, "rb").read(), 0, []
    for t, _ in cases:
        H, W = t.shape[:2]
        m = np.frombuffer(raw, "<f4", H, at)
        c = np.frombuffer(raw, "<f4", W * H, at + 4 * H).reshape(H, W)
        at += 4 * H + 4 * W * H
        total, whole, dec = struct.unpack_from("<dff", raw, at)
        at += 16
        out.append((m, c, total, np.float32(whole), np.float32(dec)))
    assert at == len(raw)
    return out


def same_bits(got, want, what):
    for name, g, w in zip(("marginal", "conditional"), got[:2], want[:2]):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %s differs in %d entries" % (what, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()))
    assert struct.pack("<d", got[2]) == struct.pack("<d", want[2]), "%s: totalSumValue %r != %r" % (what, got[2], want[2])
    assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes(), "%s: whole / decimal %r %r != %r %r" % (what, got[3], got[4], want[3], want[4])


@pytest.mark.parametrize("size", E.SIZES, ids=lambda s: "%dx%d" % s)
def test_host_program_equals_build_importance(driver, tmp_path, size):
    W, H = size
    cases = [c for c in E.all_cases() if c[:2] == size]
    assert len(cases) == len(E.CONTENTS) * 4
    got = run_driver(driver, tmp_path, [(E.stored(W, H, content, half), flip) for _, _, content, half, flip in cases])
    for case, g in zip(cases, got):
        same_bits(g, E.reference(*case), "%dx%d %s half=%s flipY=%d" % case)


def test_host_program_on_the_golden_environment(driver, tmp_path):
    """the half-rounded `environment` of the golden MIS frame gives the worker's own marginalWeights, conditionalWeights and totalSumValue"""
    g = G.load(G.GOLDEN_ENVMIS)
    stored = np.ascontiguousarray(g["environment"], np.float32).astype(np.float16).astype(np.float32)
    (m, c, total, _, _), = run_driver(driver, tmp_path, [(stored, 0)])
    assert m.tobytes() == np.ascontiguousarray(g["marginalWeights"], np.float32).tobytes()
    assert c.tobytes() == np.ascontiguousarray(g["conditionalWeights"], np.float32).reshape(c.shape).tobytes()
    assert total == float(g["totalSumValue"])


def test_the_row_map_is_the_workers_unflip():
    """k10_src_row restated: what build_importance(texels[::-1], True) reads, as rows of the stored map"""
    for H in (1, 2, 3, 4, 8, 9):
        rows = np.arange(H)[::-1].copy()  # the array the worker sees: stored order reversed
        for y in range(H):
            rows[H - 1 - y] = rows[y]
        assert [H - 1 - min(r, H - 1 - r) for r in range(H)] == rows.tolist()


@needs_hostsim
def test_gpu_files_on_the_host_simulator():
    """tests/test_gpu_env_device.py, test_gpu_env_effect.py and test_node_env_device.py with the host simulator's library in place of the device's:
    the entry points' state handling, K10's kernels lane by lane and both hosts, executed here"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    env = {k: v for k, v in os.environ.items() if k not in ("RFX_HOSTSIM", "RFX_TEST_LIB")}
    files = [os.path.join(HERE, n) for n in ("test_gpu_env_device.py", "test_gpu_env_effect.py", "test_node_env_device.py")]
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--hostsim", "-p", "no:cacheprovider"] + files, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert " passed" in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]
    assert "skipped" not in p.stdout or shutil.which("node") is None, p.stdout[-2000:]
