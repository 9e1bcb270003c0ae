"""The environments of the K10 tests (tests/test_env_tables_cpu.py, tests/test_gpu_env_device.py): sizes, contents and the host builder's
answer, computed once per case and shared (functools.lru_cache; the arrays are handed out read-only).

Sizes: powers of two only — one and several 64-column tiles / 64-row workgroups in either direction (k10_rows' tile is 64 x 64), the maximum edge in
each, a map taller than wide.  Contents: seeded, finite, |v| < 6e4."""
import functools

import numpy as np

from rfx_amd.envmap import build_importance

SIZES = [(1, 1), (2, 1), (1, 2), (8, 4), (128, 64), (64, 128), (512, 2), (2, 512), (4096, 8), (16384, 1), (1, 16384)]
CONTENTS = ["random", "ones", "black", "black_rows", "last_texel", "negative"]
LIMIT = 6e4


def _random(rs, W, H):
    """values over a dynamic range of 1e-8 .. 6e4"""
    a = (10.0 ** rs.uniform(-8.0, np.log10(LIMIT), (H, W, 4))).astype(np.float32)
    return np.minimum(a, np.float32(5.9e4))


@functools.lru_cache(maxsize=None)
def texels(W, H, content):
    """(H, W, 4) float32, row 0 = bottom: the map as the hosts hand it to set_environment"""
    rs = np.random.RandomState(1000 * CONTENTS.index(content) + 7 * W + H)
    if content == "random":
        a = _random(rs, W, H)
    elif content == "ones":  # every CDF entry equals its target: the probe's `<`
        a = np.ones((H, W, 4), np.float32)
    elif content == "black":
        a = np.zeros((H, W, 4), np.float32)
    elif content == "black_rows":  # black rows among lit ones (a single row stays lit)
        a = _random(rs, W, H)
        a[1::3] = 0
        if H > 4:
            a[H // 2:H // 2 + 2] = 0
    elif content == "last_texel":  # rows lit only in their last texel, among random ones
        a = _random(rs, W, H)
        a[::2, :-1] = 0
        a[::2, -1] = np.float32(3.5)
    else:  # a few negative texels: the CDFs are not monotone
        a = _random(rs, W, H)
        n = max(1, (W * H) // 37)
        ys, xs = rs.randint(0, H, n), rs.randint(0, W, n)
        a[ys, xs, :3] *= np.float32(-1)
    assert np.isfinite(a).all() and np.abs(a).max() < LIMIT
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def stored(W, H, content, half):
    """level 0 as rfx_set_environment stores it (the worker's fromHalfFloat view)"""
    a = texels(W, H, content)
    a = a.astype(np.float16).astype(np.float32) if half else a
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(W, H, content, half, flip):
    """(marginal, conditional, total, whole, decimal) as the hosts compute and split them (effect.keepEnvMapUpdated, Context.set_environment_importance)"""
    t = stored(W, H, content, half)
    m, c, total = build_importance(t[::-1] if flip else t, bool(flip))
    whole = float(int(total))
    for a in (m, c):
        a.setflags(write=False)
    return m, c, float(total), np.float32(whole), np.float32(total - whole)


def all_cases():
    return [(W, H, content, half, flip) for (W, H) in SIZES for content in CONTENTS for half in (True, False) for flip in (0, 1)]
