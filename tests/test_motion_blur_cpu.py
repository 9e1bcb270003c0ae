"""CPU (-m "not gpu"): MotionBlurEffect (K6).  The numpy restatement (tests/motion_blur_ref.py) against the reference's own GLSL on
llvmpipe (tests/golden/motion_blur_*.npz, tests/golden/make_golden_motion_blur.py), the rfx_motion_blur_params layout against
include/rfx.h, and the Python host's option surface (no device calls)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_blur_ref as R
from rfx_amd import abi, effect
from rfx_amd.context import load_blue_noise_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BOUND = 1e-4  # |got - ref| <= BOUND * max(1, |ref|)


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _vel4(v):
    return np.concatenate([v, np.zeros(v.shape[:2] + (2,), np.float32)], -1)


def _within(got, ref):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert (np.isnan(got) == np.isnan(ref)).all()
    ok = np.isnan(ref) | (np.abs(got - ref) <= BOUND * np.maximum(1.0, np.abs(ref)))
    assert ok.all(), (np.nanmax(np.abs(got - ref)), np.argwhere(~ok)[:5])


def _halfs_adjacent(got, ref):
    """half targets: the two stores are the same or adjacent halfs, or within the float bound"""
    g16 = np.asarray(got, np.float32).astype(np.float16).view(np.int16).astype(np.int64)
    r16 = np.asarray(ref, np.float32).astype(np.float16).view(np.int16).astype(np.int64)
    close = np.abs(np.asarray(got, np.float32) - np.asarray(ref, np.float32)) <= BOUND * np.maximum(1.0, np.abs(ref))
    assert ((np.abs(g16 - r16) <= 1) | close).all()


@pytest.mark.parametrize("uv_model", ["reference_gl", "ideal"])
def test_restatement_vs_reference_glsl_float(uv_model):
    g = _load("motion_blur_float_97x55.npz")
    bn = load_blue_noise_table()
    exact = []
    for fi, f in enumerate(g["frames"]):
        for di, dt in enumerate(g["deltaTimes"]):
            got = R.motion_blur(_vel4(g["velocity"]), g["source"], blue_noise=bn, frame=int(f), deltaTime=float(dt), uv_model=uv_model)
            _within(got, g["outputs"][fi, di])
            exact.append((got == g["outputs"][fi, di]).mean())
    if uv_model == "reference_gl":
        assert min(exact) >= 0.97, exact  # measured 0.989


@pytest.mark.parametrize("uv_model", ["reference_gl", "ideal"])
def test_restatement_vs_reference_glsl_options(uv_model):
    g = _load("motion_blur_cases_128x72.npz")
    bn = load_blue_noise_table()
    for c, ref in zip(g["cases"], g["outputs_rgb"]):
        s, i, j, rx, ry, f, dt = c
        got = R.motion_blur(_vel4(g["velocity"]), g["source"], blue_noise=bn, samples=int(s), intensity=i, jitter=j, resolution=(rx, ry),
                            frame=int(f), deltaTime=dt, uv_model=uv_model)
        _within(got[..., :3], ref)


@pytest.mark.parametrize("uv_model", ["reference_gl", "ideal"])
def test_restatement_vs_reference_glsl_half_and_traa_form(uv_model):
    g = _load("motion_blur_half_96x54.npz")
    bn = load_blue_noise_table()
    src, acc = g["source"].astype(np.float32), g["accumulated"].astype(np.float32)
    for k, c in enumerate(g["cases"]):
        s, i, j, rx, ry, f, dt = c
        kw = dict(blue_noise=bn, samples=int(s), intensity=i, jitter=j, resolution=(rx, ry), frame=int(f), deltaTime=dt, uv_model=uv_model,
                  target_half=True)
        own = R.motion_blur(_vel4(g["velocity"]), src, **kw)
        traa = R.motion_blur(_vel4(g["velocity"]), src, center=acc, center_nearest=True, center_alpha_one=True, **kw)
        _halfs_adjacent(own, g["outputs_own"][k])
        _halfs_adjacent(traa, g["outputs_traa"][k])
        if uv_model == "reference_gl":
            assert (own == g["outputs_own"][k].astype(np.float32)).mean() >= 0.999
            assert (traa == g["outputs_traa"][k].astype(np.float32)).mean() >= 0.999


def test_fixture_inputs_cover_the_velocity_edges():
    for name in ("motion_blur_float_97x55.npz", "motion_blur_cases_128x72.npz", "motion_blur_half_96x54.npz"):
        v = _load(name)["velocity"]
        d = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]
        assert (d == 0).any() and ((d > 0) & (d <= 1e-9)).any() and np.isnan(d).any() and (np.abs(v) > 1).any(), name


def test_motion_blur_params_layout_matches_header(tmp_path):
    c = tmp_path / "mb.c"
    fields = [f for f, _ in abi.MotionBlurParams._fields_]
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rfx.h"\nint main(){printf("%zu' + " %zu" * len(fields) + ' %d %d %d %d %d\\n",'
                 "sizeof(rfx_motion_blur_params)," + ",".join("offsetof(rfx_motion_blur_params,%s)" % f for f in fields) +
                 ",(int)RFX_TEX_EFFECT_INPUT,(int)RFX_TEX_MOTION_BLUR,(int)RFX_TEX_COUNT,(int)RFX_PROF_K6,RFX_ABI_VERSION);return 0;}\n")
    exe = tmp_path / "mb"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(abi.MotionBlurParams)] + [getattr(abi.MotionBlurParams, f).offset for f in fields]
    want += [abi.TEX_EFFECT_INPUT, abi.TEX_MOTION_BLUR, abi.TEX_COUNT, abi.PROF_KINDS.index("k6_motion_blur"), abi.RFX_ABI_VERSION]
    assert got == want
    assert abi.TEX_FORMAT[abi.TEX_EFFECT_INPUT] == (np.float32, 4) and abi.TEX_FORMAT[abi.TEX_MOTION_BLUR] == (np.float32, 4)
    assert "rfx_motion_blur" in abi.EXPORTS and hasattr(abi.load_library(), "rfx_motion_blur")


def test_python_option_surface():
    """MotionBlurEffect.js:14,37-45,51-66: defaults, `samples` fixed at construction, intensity / jitter reactive."""
    e = effect.MotionBlurEffect(effect.VelocityDepthNormalPass(None, None))
    assert (e.intensity, e.jitter, e.samples) == (1, 1, 16)
    assert (e.uniforms.intensity, e.uniforms.jitter, e.uniforms.samples) == (1.0, 1.0, 16)
    e.intensity, e.jitter, e.samples = 2.5, 0.0, 4
    assert (e.uniforms.intensity, e.uniforms.jitter, e.uniforms.samples) == (2.5, 0.0, 16)  # the define keeps its constructed value
    assert e.samples == 4
    e2 = effect.MotionBlurEffect(None, {"samples": 7, "intensity": -1})
    assert (e2.uniforms.samples, e2.uniforms.intensity, e2.uniforms.jitter) == (7, -1.0, 1.0)


class _Recorder:
    W, H = 8, 4

    def __init__(self):
        self.calls = []

    def upload(self, tex, a):
        self.calls.append(("upload", tex, a.shape, a.dtype))

    def motion_blur(self, p):
        self.calls.append(("motion_blur", p.source, p.center, p.centerAlphaOne, p.frame, p.deltaTime, tuple(p.resolution), p.targetHalf))


def test_python_update_uniforms():
    """:85-101: deltaTime = max(1/1000, dt), frame % 4096 (default: the updates so far), resolution (default: the frame), input sources."""
    e, r = effect.MotionBlurEffect(None), _Recorder()
    e.update(r, abi.TEX_FINAL, 0.0)
    assert e.mainImage(r) == abi.TEX_MOTION_BLUR
    assert r.calls[-1] == ("motion_blur", abi.TEX_FINAL, -1, 0, 0, np.float32(1 / 1000), (8.0, 4.0), 0)
    e.update(r, abi.TEX_FINAL, 1 / 60)
    e.mainImage(r)
    assert r.calls[-1][4] == 1 and r.calls[-1][5] == np.float32(1 / 60)
    e.frame, e.resolution = 4097, (1920, 1080)
    e.update(r, {"data": np.ones((4, 8, 4), np.float32), "texture": {"type": effect.HalfFloatType}}, 1 / 30)
    e.mainImage(r)
    assert r.calls[-2][:2] == ("upload", abi.TEX_EFFECT_INPUT)
    assert r.calls[-1] == ("motion_blur", abi.TEX_EFFECT_INPUT, -1, 0, 1, np.float32(1 / 30), (1920.0, 1080.0), 1)
    traa = effect.TRAAEffect(None, None, None)
    traa.uniforms["accumulatedTexture"] = abi.TEX_TEMPORAL0
    e.shareEffectPass(traa)
    e.update(r, None, 1 / 60)
    e.mainImage(r)
    assert r.calls[-1][1:4] == (abi.TEX_SSGI, abi.TEX_TEMPORAL0, 1)
