"""Test helper (CPU): the launch plans of realism-effects_amd/csrc/rfx_launch.h as the library computes them.  The host-simulator build
(tests/hostsim) exports the two plan functions the launchers and ssgi_draw call — rfx_internal_k1_table, rfx_internal_k3_tile — and a child
process that loads it answers a whole list of cases at once."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
needs_hostsim = pytest.mark.skipif(not os.path.exists(CLANG) or shutil.which("make") is None, reason="no host clang++ / make")

_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
I = ctypes.c_int
class K1(ctypes.Structure):
    _fields_ = [(n, I) for n in ("cell_shift", "cells_w", "cells_h", "pitch", "pitch_log2", "pow2", "vec4")]
class K3(ctypes.Structure):
    _fields_ = [(n, I) for n in ("Rx", "Ry", "LW", "LH", "pitch", "skip")] + [("lds_bytes", ctypes.c_size_t), ("tiled", I)]
lib.rfx_internal_k1_table.argtypes = [I, I, ctypes.POINTER(K1)]
lib.rfx_internal_k3_tile.argtypes = [I, I, ctypes.c_float, I, I, ctypes.POINTER(K3)]
kind, cases = json.load(sys.stdin)
fn, T = (lib.rfx_internal_k1_table, K1) if kind == "k1" else (lib.rfx_internal_k3_tile, K3)
out = []
for case in cases:
    t = T()
    rc = fn(*case, ctypes.byref(t))
    assert rc == 0, (case, rc)
    out.append({n: getattr(t, n) for n, _ in T._fields_})
json.dump(out, sys.stdout)
"""


def _plans(kind, cases):
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    from conftest import hostsim_child_env
    env = dict(os.environ, **hostsim_child_env(sim))
    p = subprocess.run([sys.executable, "-c", _CHILD, env["RFX_TEST_LIB"]], input=json.dumps([kind, cases]), capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout)


def k1_tables(sizes):
    """[(W, H), ...] -> one dict per size: cell_shift, cells_w, cells_h, pitch, pitch_log2, pow2, vec4"""
    return _plans("k1", [list(s) for s in sizes])


def k3_tiles(cases):
    """[(W, H, radius, inputIsTemporal, textureCount), ...] -> one dict per case: Rx, Ry, LW, LH, pitch, skip, lds_bytes, tiled"""
    return _plans("k3", [[W, H, float(r), int(t), tc] for W, H, r, t, tc in cases])
