"""Checkpoint and resume of the temporal state on the device (rfx_amd/state.py, js/state.js): N frames straight on one context against
k frames, save, a FRESH context with fresh effects, load, N - k more.  After every frame past the cut every stage output is compared
byte for byte — no tolerance anywhere.  Small frames, so the file also runs under --hostsim."""
import json
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from rfx_amd import abi, effect, state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")

W, H, N, K = 200, 132, 8, 3
STAGES = (abi.TEX_SSGI, abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1, abi.TEX_DENOISE_A0, abi.TEX_DENOISE_A1, abi.TEX_DENOISE_B0, abi.TEX_DENOISE_B1,
          abi.TEX_COMPOSE, abi.TEX_FINAL)

# kind, options, scene.environment, MotionBlurEffect chained
CASES = {
    "default_chain_2_iterations": ("ssgi", dict(denoiseIterations=2), False, True),
    "denoise_mode_temporal": ("ssgi", dict(denoiseMode="temporal"), False, False),
    "ssr": ("ssr", dict(), False, False),
    "environment_importance_sampling": ("ssgi", dict(importanceSampling=True), True, False),
    "traa_half": ("traa", dict(fullAccumulate=True), False, True),
    "resolution_scale_half": ("ssgi", dict(resolutionScale=0.5), False, False),
}


def _frames(n=N):
    from rfx_amd.scene import synthetic_frame
    return [synthetic_frame(W, H, i) for i in range(n)]


class Run:
    """Fresh effects of a case on `renderer`; frames() records every stage output after each frame."""

    def __init__(self, case, renderer, seeds=None):
        kind, options, env, with_mb = CASES[case] if isinstance(case, str) else case
        self.kind, self.r = kind, renderer
        self.scene = types.SimpleNamespace(frame=None)
        if env:  # an input, not state: the caller sets it again after a resume
            from rfx_amd.scene import synthetic_environment
            self.scene.environment = dict(data=synthetic_environment(64, 32))
        self.cam = None
        self.options, self.seeds, self.with_mb = options, seeds, with_mb
        self.fx = self.mb = None
        self.outputs = []

    def _build(self, camera):
        self.cam = types.SimpleNamespace(**vars(camera))
        if self.kind == "traa":
            vel = effect.VelocityDepthNormalPass(self.scene, self.cam)
            self.fx = effect.TRAAEffect(self.scene, self.cam, vel, dict(self.options), half_store_rtz=True)
        else:
            cls = effect.SSREffect if self.kind == "ssr" else effect.SSGIEffect
            self.fx = cls(None, self.scene, self.cam, dict(self.options, width=W, height=H, steps=8, refineSteps=2), seeds=self.seeds, half_store_rtz=True)
            vel = self.fx.denoiser.velocityDepthNormalPass
        if self.with_mb:
            self.mb = effect.MotionBlurEffect(vel, dict(samples=8), half_store_rtz=True)
            if self.kind == "traa":
                self.mb.shareEffectPass(self.fx)
        self.effects = [self.fx] + ([self.mb] if self.mb else [])
        return self

    def frames(self, frames, record=True):
        if self.fx is None:
            self._build(frames[0].camera)
        for f in frames:
            self.scene.frame = f
            for k, v in vars(f.camera).items():
                setattr(self.cam, k, v)
            out = {}
            if self.kind == "traa":
                self.fx.update(self.r, dict(texture=dict(type=effect.HalfFloatType), width=W, height=H, data=f.direct))
                if self.mb:
                    self.mb.update(self.r, None, 1 / 60)
                    self.mb.mainImage(self.r)
                if record:
                    out["traa"] = self.fx.output(self.r).tobytes()
                    stages = (abi.TEX_TEMPORAL0, abi.TEX_FBCOPY_F16)
            else:
                self.fx.update(self.r, None)
                self.fx.mainImage(self.r)
                if self.mb:
                    self.mb.update(self.r, abi.TEX_FINAL, 1 / 60)
                    self.mb.mainImage(self.r)
                stages = STAGES
            if record:
                for t in stages + ((abi.TEX_MOTION_BLUR,) if self.mb else ()):
                    out[abi.TEX_NAMES[t]] = self.r.download(t).tobytes()
                self.outputs.append(out)
        return self


def _assert_same_outputs(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w)
        for name in sorted(w):
            assert g[name] == w[name], "%s: %s differs %d frame(s) after the resume" % (what, name, i + 1)


@pytest.mark.parametrize("case", sorted(CASES))
def test_resumed_run_is_byte_identical_on_the_device(tmp_path, case):
    from rfx_amd.context import Context
    frames = _frames()
    ctx = Context(W, H)
    straight = Run(case, ctx, seeds=dict(ssgi=31, denoise=32)).frames(frames[:K], record=False).frames(frames[K:])
    ctx.close()
    ctx = Context(W, H)
    first = Run(case, ctx, seeds=dict(ssgi=31, denoise=32)).frames(frames[:K], record=False)
    header = state.save_state(str(tmp_path / "ck"), ctx, first.effects)
    ctx.close()
    assert {p["slot"] for p in header["planes"]} == {abi.TEX_NAMES[t] for t in state.state_slots(first.effects)}
    ctx = Context(W, H)  # a fresh context, fresh effects with random blue-noise starts
    resumed = Run(case, ctx)._build(frames[K].camera)
    state.load_state(str(tmp_path / "ck"), ctx, resumed.effects)
    resumed.frames(frames[K:])
    assert ctx.halo_violations() == 0
    ctx.close()
    _assert_same_outputs(resumed.outputs, straight.outputs, case)
    # what the comparison is able to see: the same resume without the planes is a different run
    ctx = Context(W, H)
    blind = Run(case, ctx)._build(frames[K].camera)
    for e, s in zip(blind.effects, header["effects"]):
        e.set_state(s)
    blind.frames(frames[K:K + 1])
    ctx.close()
    assert any(blind.outputs[0][k] != straight.outputs[0][k] for k in straight.outputs[0])


def _local_tiles(ntiles, halo):
    from test_gpu_parity import _LocalTiles

    class Tiles(_LocalTiles):
        def sync(self):
            for c in self.ctxs:
                c.sync()

        def final_compose(self, p):
            for c in self.ctxs:
                c.final_compose(p)

        def close(self):
            for c in self.ctxs:
                c.close()

    return Tiles(W, H, ntiles, halo)


@pytest.mark.parametrize("ntiles", [2, 3])
def test_checkpoints_are_independent_of_the_row_tiling(tmp_path, ntiles):
    """Saved whole-frame, resumed on 2 / 3 row tiles (each takes the rows it holds, halo included; no exchange after the load), and the
    reverse: the gathered outputs equal the single-context run's, and no tile read outside its halo."""
    from rfx_amd import tiling
    from rfx_amd.context import Context
    frames = _frames()
    vmax = max(float(np.abs(f.velocity[..., 1].view(np.float32)).max()) for f in frames)
    halo = tiling.required_halo(3.0, vmax, H, W)
    tiled = ("ssgi", dict(denoiseIterations=2), False, False)  # the default chain without motion blur (a streak can reach anywhere: whole-frame runs only)
    stages = (abi.TEX_SSGI, abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1, abi.TEX_DENOISE_B0, abi.TEX_DENOISE_B1, abi.TEX_COMPOSE)

    def gathered(run):
        return {abi.TEX_NAMES[t]: run.r.download(t).tobytes() for t in stages}

    single = Context(W, H)
    straight = Run(tiled, single, seeds=dict(ssgi=3, denoise=4)).frames(frames[:K], record=False)
    whole_dir, tiled_dir = str(tmp_path / "whole"), str(tmp_path / "tiled")
    whole_header = state.save_state(whole_dir, single, straight.effects)
    straight.frames(frames[K:], record=False)
    want = gathered(straight)
    single.close()
    # whole-frame checkpoint -> tiles
    tiles = _local_tiles(ntiles, halo)
    resumed = Run(tiled, tiles)._build(frames[K].camera)
    state.load_state(whole_dir, tiles, resumed.effects)
    resumed.frames(frames[K:], record=False)
    assert gathered(resumed) == want
    assert all(c.halo_violations() == 0 for c in tiles.ctxs)
    tiles.close()
    # tiles -> checkpoint (the same files) -> whole frame
    tiles = _local_tiles(ntiles, halo)
    first = Run(tiled, tiles, seeds=dict(ssgi=3, denoise=4)).frames(frames[:K], record=False)
    tiled_header = state.save_state(tiled_dir, tiles, first.effects)
    tiles.close()
    assert tiled_header == whole_header
    for p in whole_header["planes"]:
        assert open(os.path.join(whole_dir, p["file"]), "rb").read() == open(os.path.join(tiled_dir, p["file"]), "rb").read(), p["slot"]
    single = Context(W, H)
    resumed = Run(tiled, single)._build(frames[K].camera)
    state.load_state(tiled_dir, single, resumed.effects)
    resumed.frames(frames[K:], record=False)
    assert gathered(resumed) == want and single.halo_violations() == 0
    single.close()


def _dumps(tmp_path, n, w=160, h=96):
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    dirs = []
    for i in range(n):
        d = str(tmp_path / ("dump%d" % i))
        write_dump(d, synthetic_frame(w, h, i))
        dirs.append(d)
    return dirs


def _run_dump(dirs, out, *extra, env=None):
    res = subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--steps", "12", "--refineSteps", "3"] + list(extra),
                                  text=True, env=env, timeout=900)
    return json.loads(res.strip().splitlines()[-1])


def _bins(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.endswith(".bin")}


@pytest.mark.skipif(node is None, reason="node not installed")
@pytest.mark.parametrize("flags", [(), ("--motionBlur", '{"samples":8}'), ("--traa", '"half"'), ("--stream", "true")], ids=["plain", "motion_blur", "traa", "stream"])
def test_run_dump_resumes_byte_identically(tmp_path, flags):
    """run_dump.js over 6 dumps == run_dump.js over 3 with --saveState, then run_dump.js --loadState over the other 3: every .bin it writes.
    The Python host resumed from the same (Node-written) checkpoint writes the same bytes too."""
    dirs = _dumps(tmp_path, 6)
    whole, a, b, ck = (str(tmp_path / n) for n in ("whole", "a", "b", "ck"))
    _run_dump(dirs, whole, *flags)
    assert _run_dump(dirs[:3], a, "--saveState", ck, "--saveEvery", "2", *flags)["frames"] == 3
    assert _run_dump(dirs[3:], b, "--loadState", ck, *flags)["haloViolations"] == 0
    want, got = _bins(whole), _bins(b)
    assert want and sorted(want) == sorted(got)
    for name in want:
        assert want[name] == got[name], name
    assert _bins(a) != want
    if flags and flags[0] in ("--traa", "--motionBlur"):
        return
    # the Python host from the Node host's checkpoint
    from rfx_amd.context import Context
    from rfx_amd.dump import read_dump
    W2, H2 = 160, 96
    scene = types.SimpleNamespace(frame=None)
    frames = [read_dump(d) for d in dirs[3:]]
    cam = types.SimpleNamespace(**vars(frames[0].camera))
    fx = effect.SSGIEffect(None, scene, cam, dict(width=W2, height=H2, steps=12, refineSteps=3), half_store_rtz=True)
    ctx = Context(W2, H2)
    state.load_state(ck, ctx, [fx])
    for f in frames:
        scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        fx.update(ctx, None)
    fx.mainImage(ctx)
    for name, tex in (("final", abi.TEX_FINAL), ("compose", abi.TEX_COMPOSE), ("denoise_b0", abi.TEX_DENOISE_B0), ("denoise_b1", abi.TEX_DENOISE_B1),
                      ("temporal0", abi.TEX_TEMPORAL0), ("ssgi", abi.TEX_SSGI)):
        assert ctx.download(tex).tobytes() == want[name + ".bin"], name
    ctx.close()


@pytest.mark.skipif(node is None, reason="node not installed")
@pytest.mark.skipif(os.environ.get("RFX_HOSTSIM") != "1", reason="one Node process per tile without RCCL / without N GPUs: pytest --hostsim")
def test_run_dump_resumes_across_rank_counts(tmp_path):
    """The same with --ranks 2 (the conditions of test_node_row_tiled_run_equals_single_process): every rank writes its rows of the
    whole-frame planes, and a checkpoint of either run resumes in the other."""
    dirs = _dumps(tmp_path, 6)
    env = dict(os.environ, RFX_ONE_GPU="1")
    whole, a1, a2, ck1, ck2 = (str(tmp_path / n) for n in ("whole", "a1", "a2", "ck1", "ck2"))
    _run_dump(dirs, whole, env=env)
    want = _bins(whole)
    _run_dump(dirs[:3], a1, "--saveState", ck1, env=env)
    _run_dump(dirs[:3], a2, "--saveState", ck2, "--ranks", "2", env=env)
    h1, h2 = (json.load(open(os.path.join(c, "state.json"))) for c in (ck1, ck2))
    assert h1 == h2
    for p in h1["planes"]:
        assert open(os.path.join(ck1, p["file"]), "rb").read() == open(os.path.join(ck2, p["file"]), "rb").read(), p["slot"]
    for i, (ck, ranks) in enumerate(((ck2, "2"), (ck1, "2"), (ck2, "1"), (ck1, "3"))):
        out = str(tmp_path / ("b%d" % i))
        info = _run_dump(dirs[3:], out, "--loadState", ck, *(("--ranks", ranks) if ranks != "1" else ()), env=env)
        assert info["haloViolations"] == 0
        got = _bins(out)
        assert sorted(got) == sorted(want)
        for name in want:
            assert want[name] == got[name], (ck, ranks, name)
