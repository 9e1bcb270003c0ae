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
if kind == "k3_layouts":  # a sweep: only the (pitch, skip) pairs it selects travel back, each with the first case that selected it
    ws, hs, radii = cases
    seen = {}
    t = K3()
    for W in range(*ws):
        for H in range(*hs):
            for r in radii:
                assert lib.rfx_internal_k3_tile(W, H, r, 1, 2, ctypes.byref(t)) == 0
                if t.tiled and (t.pitch, t.skip) not in seen:
                    seen[(t.pitch, t.skip)] = [W, H, r]
    json.dump([[p, s] + c for (p, s), c in sorted(seen.items())], sys.stdout)
    sys.exit(0)
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


def k3_pass0_layouts(widths, heights, radii):
    """The (pitch, skip) layouts of the staged rectangle that pass 0 with two textures (the only draw that shaves corners) is planned with
    over range(*widths) x range(*heights) x radii, tiled plans only: {(pitch, skip): the first (W, H, radius) that selected it}"""
    return {(p, s): (W, H, r) for p, s, W, H, r in _plans("k3_layouts", [list(widths), list(heights), [float(r) for r in radii]])}
