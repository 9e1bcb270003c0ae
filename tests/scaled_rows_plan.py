"""Test helper (CPU): rfx_launch.h rfx_scaled_rows as the library computes it (the export rfx_internal_scaled_rows of the host-simulator build,
asked by a child process for a whole list of cases at once — the tests/launch_plans.py pattern), and an independent statement of the two vUv
models in numpy's IEEE fp32, for the brute force it is held against."""
import json
import os
import subprocess
import sys

import numpy as np

from launch_plans import ROOT, needs_hostsim  # noqa: F401

_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
I = ctypes.c_int
lib.rfx_internal_scaled_rows.argtypes = [I] * 7 + [ctypes.POINTER(I)] * 2
out = []
for case in json.load(sys.stdin):
    j0, j1 = I(), I()
    assert lib.rfx_internal_scaled_rows(*case, ctypes.byref(j0), ctypes.byref(j1)) == 0, case
    out.append([j0.value, j1.value])
json.dump(out, sys.stdout)
"""


def scaled_rows(cases):
    """[(W, H, Hs, uv_model, y0, y1, apron), ...] -> [(j0, j1), ...]"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    from conftest import hostsim_child_env
    env = dict(os.environ, **hostsim_child_env(sim))
    p = subprocess.run([sys.executable, "-c", _CHILD, env["RFX_TEST_LIB"]], input=json.dumps([list(map(int, c)) for c in cases]), capture_output=True,
                       text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return [tuple(t) for t in json.loads(p.stdout)]


# ---- the two vUv models in numpy: fp32 operations are IEEE there as on the device, one rounding each
UV_IDEAL, UV_REFERENCE_GL = 0, 1
F = np.float32


def frag_v(model, w, h):
    """vUv.y of every row of a w x h render target under `model` (include/rfx.h rfx_set_uv_model), fp32: (i + 0.5) / n, one correctly rounded
    division; or the plane equation v0 + dv * y of the reference GL's rasteriser, ONE fma.  numpy has no fma: dv * y is exact in fp64 (24 + 12
    bits) and so is its sum with v0 (both below 2, the smaller ulp is above 2^-48 for h < 4096), so the single rounding to fp32 is the fma's."""
    assert h < 4096 and w < 16384
    y = np.arange(h)
    if model == UV_IDEAL:
        return (y.astype(F) + F(0.5)) / F(h)
    ooa = F(1.0) / (F(w) * F(h))
    dv = F(w) * ooa
    v0 = F(1.0) - dv * (F(h) - F(0.5))
    assert all(type(t) is np.float32 for t in (ooa, dv, v0))
    return (np.float64(dv) * y.astype(np.float64) + np.float64(v0)).astype(F)


def nearest_idx(u, size: int):
    """NEAREST CLAMP_TO_EDGE: trunc(clamp(fp32(u * size), 0, size - 1))"""
    c = np.asarray(u, F) * F(size)
    return np.clip(c, F(0), F(size - 1)).astype(np.int64)
