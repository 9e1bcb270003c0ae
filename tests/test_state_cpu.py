"""Checkpoint and resume of the temporal state (rfx_amd/state.py, js/state.js) without a GPU.

The in-memory renderer of tests/state_mem_renderer.py stands for the device on both hosts: a lost plane or a lost counter changes the
stream of draw digests.  Every comparison is byte for byte (digests of parameters and slot bytes; plane files; parsed headers)."""
import json
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from rfx_amd import abi, effect, state
from state_mem_renderer import MEM_RENDERER_JS, MemRenderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
needs_node = pytest.mark.skipif(node is None, reason="node not installed")

W, H, FRAMES, CUT = 12, 8, 12, 5


def camera_of(i):
    """A camera per frame, every number exactly a float32 (the two hosts then write the same header): it moves on some frames and rests
    on others, so didCameraMove / fullAccumulate and the previous-camera uniforms differ from frame to frame."""
    x = 0.25 * (i // 2)
    m = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, x, 1.5, 2, 1]
    mi = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -x, -1.5, -2, 1]
    p = [1.5, 0, 0, 0, 0, 2.5, 0, 0, 0, 0, -1.25, -1, 0, 0, -0.5, 0]
    pi = [0.75, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0, -2, 0, 0, -1, 2.5]
    return dict(projectionMatrix=p, projectionMatrixInverse=pi, matrixWorld=m, matrixWorldInverse=mi, position=[x, 1.5, 2],
                quaternion=[0, 0, 0, 1], near=0.25, far=64, isPerspectiveCamera=True)


def frame_of(i):
    f = types.SimpleNamespace(width=W, height=H)
    f.depth = np.full((H, W), 0.5, np.float32)
    f.gbuffer = np.full((H, W, 4), i + 1, np.uint32)
    f.velocity = np.full((H, W, 4), i + 2, np.uint32)
    f.direct = np.full((H, W, 4), 0.25 * (i + 1), np.float32)  # (exact in half precision: TRAA's HalfFloatType buffer)
    return f


# kind, effect options, TRAA buffer type, MotionBlurEffect chained after it
CASES = {
    "ssgi_full": ("ssgi", dict(denoiseIterations=2), None, False),
    "ssgi_full_temporal": ("ssgi", dict(denoiseMode="full_temporal"), None, False),
    "ssgi_denoised": ("ssgi", dict(denoiseMode="denoised"), None, False),
    "ssgi_temporal": ("ssgi", dict(denoiseMode="temporal"), None, False),
    "ssr": ("ssr", dict(), None, False),
    "ssgi_half_resolution": ("ssgi", dict(resolutionScale=0.5), None, False),
    "traa_half": ("traa", dict(fullAccumulate=True), "half", False),
    "traa_float": ("traa", dict(fullAccumulate=True), "float", False),
    "ssgi_full_motion_blur": ("ssgi", dict(), None, True),
    "ssr_motion_blur": ("ssr", dict(), None, True),
    "traa_half_motion_blur": ("traa", dict(fullAccumulate=True), "half", True),
    "traa_float_motion_blur": ("traa", dict(fullAccumulate=True), "float", True),
}


class PyRun:
    """One host-side set-up (fresh effects on a fresh renderer) of a case; `seeds` None = random blue-noise starts, as a user gets."""

    def __init__(self, case, seeds=None, renderer=None):
        kind, options, traa_type, with_mb = CASES[case] if isinstance(case, str) else case
        self.kind, self.traa_type = kind, traa_type
        self.r = renderer or MemRenderer(W, H)
        self.scene = types.SimpleNamespace(frame=None)
        self.cam = types.SimpleNamespace(**camera_of(0))
        self.per_frame = []
        if kind == "traa":
            self.vel = effect.VelocityDepthNormalPass(self.scene, self.cam)
            self.fx = effect.TRAAEffect(self.scene, self.cam, self.vel, dict(options))
        else:
            cls = effect.SSREffect if kind == "ssr" else effect.SSGIEffect
            self.fx = cls(None, self.scene, self.cam, dict(options, width=W, height=H), seeds=seeds)
            self.vel = self.fx.denoiser.velocityDepthNormalPass
        self.mb = effect.MotionBlurEffect(self.vel, dict(samples=8)) if with_mb else None
        if self.mb and kind == "traa":
            self.mb.shareEffectPass(self.fx)
        self.effects = [self.fx] + ([self.mb] if self.mb else [])

    def frames(self, a, b):
        for i in range(a, b):
            n0 = len(self.r.calls)
            self.scene.frame = frame_of(i)
            for k, v in camera_of(i).items():
                setattr(self.cam, k, v)
            if self.kind == "traa":
                ttype = effect.HalfFloatType if self.traa_type == "half" else effect.FloatType
                self.fx.update(self.r, dict(texture=dict(type=ttype), width=W, height=H, data=self.scene.frame.direct))
                if self.mb:
                    self.mb.update(self.r, None, 1 / 60)
                    self.mb.mainImage(self.r)
            else:
                self.fx.update(self.r, None)
                self.fx.mainImage(self.r)
                if self.mb:
                    self.mb.update(self.r, abi.TEX_FINAL, 1 / 60)
                    self.mb.mainImage(self.r)
            self.per_frame.append(self.r.calls[n0:])
        return self

    def save(self, d):
        return state.save_state(d, self.r, self.effects)

    def load(self, d):
        return state.load_state(d, self.r, self.effects)


@pytest.mark.parametrize("case", sorted(CASES))
def test_resumed_run_issues_the_same_calls(tmp_path, case):
    """12 frames straight == 5 frames, save, fresh objects with other random seeds, load, 7 more: the call streams of frames 6..12 and the
    final contents of every slot."""
    straight = PyRun(case, seeds=dict(ssgi=101, denoise=202)).frames(0, FRAMES)
    first = PyRun(case, seeds=dict(ssgi=101, denoise=202)).frames(0, CUT)
    header = first.save(str(tmp_path / "ck"))
    assert first.per_frame == straight.per_frame[:CUT]
    resumed = PyRun(case, seeds=None)  # random starts: the saved recurrences must replace them
    resumed.load(str(tmp_path / "ck"))
    resumed.frames(CUT, FRAMES)
    assert resumed.per_frame == straight.per_frame[CUT:]
    assert resumed.r.slot_digests() == straight.r.slot_digests()
    # the set of planes follows the effect objects (single-texture modes hold no *1 planes, "temporal" modes keep the framebuffer copy)
    slots = {p["slot"] for p in header["planes"]}
    kind, options, traa_type, _ = CASES[case]
    if kind == "traa":
        assert slots == {"temporal0", "fbcopy_f16" if traa_type == "half" else "fbcopy_f32"}
    elif kind == "ssr":
        assert slots == {"temporal0", "denoise_a0", "denoise_b0", "compose"}
    else:
        mode = options.get("denoiseMode", "full")
        want = {"temporal0", "temporal1"}
        want |= {"denoise_a0", "denoise_a1", "denoise_b0", "denoise_b1"} if mode in ("full", "denoised") else {"fbcopy_f32"}
        want |= {"compose"} if mode.startswith("full") else set()
        assert slots == want
    # a resume that forgets the planes, or the host state, is NOT the same run (the double shows what the test is able to see)
    blind = PyRun(case, seeds=dict(ssgi=101, denoise=202))
    for e, s in zip(blind.effects, header["effects"]):
        e.set_state(s)
    blind.frames(CUT, FRAMES)
    assert blind.per_frame != straight.per_frame[CUT:]


@pytest.mark.parametrize("case", ["ssgi_full", "traa_half_motion_blur", "ssgi_temporal"])
def test_save_before_the_first_frame_and_after_reset(tmp_path, case):
    straight = PyRun(case, seeds=dict(ssgi=7, denoise=8)).frames(0, 4)
    fresh = PyRun(case, seeds=dict(ssgi=7, denoise=8))
    fresh.save(str(tmp_path / "zero"))  # nothing drawn yet: TRAAEffect has no pass, MotionBlurEffect's frame is unset
    resumed = PyRun(case)
    resumed.load(str(tmp_path / "zero"))
    resumed.frames(0, 4)
    assert resumed.per_frame == straight.per_frame and resumed.r.slot_digests() == straight.r.slot_digests()
    # right after reset(): keepData 0 travels
    a = PyRun(case, seeds=dict(ssgi=7, denoise=8)).frames(0, 3)
    a.fx.reset()
    a.save(str(tmp_path / "reset"))
    a.frames(3, 6)
    b = PyRun(case)
    b.load(str(tmp_path / "reset"))
    assert b.fx.get_state() == json.loads(json.dumps(PyRun(case).load(str(tmp_path / "reset"))["effects"][0]))
    b.frames(3, 6)
    assert b.per_frame == a.per_frame[3:] and b.r.slot_digests() == a.r.slot_digests()
    never_reset = PyRun(case, seeds=dict(ssgi=7, denoise=8)).frames(0, 6)
    assert never_reset.per_frame[3:] != a.per_frame[3:]


def test_floats_survive_bit_for_bit(tmp_path):
    """The header keeps raw IEEE bytes: awkward values (denormals, -0.0, values no short decimal names) return unchanged."""
    run = PyRun("traa_float").frames(0, 2)
    tp = run.fx.temporalReprojectPass
    odd64 = np.array([np.nextafter(0.1, 1), -0.0, 5e-324], np.float64)
    tp.lastCameraTransform["position"] = odd64.copy()
    tp.lastCameraTransform["quaternion"] = np.array([1e-310, np.pi, -np.e, 1 / 3], np.float64)
    tp.uniforms.keepData = float(np.float32(1e-42))
    tp._prev.projectionMatrix[5] = float(np.nextafter(np.float32(2.5), np.float32(3)))
    run.fx.unjitteredProjectionMatrix = (np.arange(16, dtype=np.float32) / np.float32(3)).reshape(4, 4)
    want = run.fx.get_state()
    run.save(str(tmp_path / "ck"))
    other = PyRun("traa_float")
    other.load(str(tmp_path / "ck"))
    assert other.fx.get_state() == want
    t2 = other.fx.temporalReprojectPass
    assert t2.lastCameraTransform["position"].tobytes() == odd64.tobytes()
    assert np.float32(t2.uniforms.keepData).tobytes() == np.float32(1e-42).tobytes()
    assert bytes(t2._prev) == bytes(tp._prev)
    assert np.asarray(other.fx.unjitteredProjectionMatrix).tobytes() == np.asarray(run.fx.unjitteredProjectionMatrix).tobytes()


# ---- refusals
def _snapshot(run):
    return json.dumps([e.get_state() for e in run.effects], sort_keys=True), run.r.slot_digests()


def _edit_header(d, fn):
    p = os.path.join(d, "state.json")
    h = json.load(open(p))
    fn(h)
    json.dump(h, open(p, "w"))


def _plane_path(d, slot):
    h = json.load(open(os.path.join(d, "state.json")))
    return os.path.join(d, [p["file"] for p in h["planes"] if p["slot"] == slot][0])


def _flip_byte(d):
    p = _plane_path(d, "denoise_b0")
    raw = bytearray(open(p, "rb").read())
    raw[len(raw) // 2] ^= 0x10
    open(p, "wb").write(raw)


def _truncate(d):
    p = _plane_path(d, "temporal1")
    os.truncate(p, os.path.getsize(p) - 1)


REFUSALS = [
    ("format", lambda d: _edit_header(d, lambda h: h.update(format="something-else")), "ssgi_full", "format"),
    ("version", lambda d: _edit_header(d, lambda h: h.update(version=state.VERSION + 1)), "ssgi_full", "version"),
    ("width", lambda d: _edit_header(d, lambda h: h.update(width=W + 1)), "ssgi_full", "width"),
    ("height", lambda d: _edit_header(d, lambda h: h.update(height=H - 1)), "ssgi_full", "height"),
    ("flipped_byte", _flip_byte, "ssgi_full", "planes[denoise_b0].sha256"),
    ("truncated_plane", _truncate, "ssgi_full", "planes[temporal1].size"),
    ("missing_plane", lambda d: os.unlink(_plane_path(d, "compose")), "ssgi_full", "planes[compose].file"),
    ("effect_class", None, "ssr", "effects[0].class"),
    ("texture_count", lambda d: _edit_header(d, lambda h: h["effects"][0]["denoiser"]["temporalReprojectPass"].update(textureCount=1)), "ssgi_full",
     "effects[0].denoiser.temporalReprojectPass.textureCount"),
    ("denoise_mode", None, "ssgi_denoised", "effects[0].denoiser.denoiseMode"),
    ("resolution_scale", None, "ssgi_half_resolution", "effects[0].resolutionScale"),
    ("effect_count", None, "ssgi_full_motion_blur", "effects"),
    ("host_state_field", lambda d: _edit_header(d, lambda h: h["effects"][0]["ssgiPass"]["blueNoiseIndex"].pop("index")), "ssgi_full",
     "effects[0].ssgiPass.blueNoiseIndex.index"),
    ("not_hex", lambda d: _edit_header(d, lambda h: h["effects"][0]["denoiser"]["temporalReprojectPass"].update(keepData="1.0")), "ssgi_full",
     "effects[0].denoiser.temporalReprojectPass.keepData"),
]


@pytest.mark.parametrize("name,damage,loader,field", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_load_refuses_and_names_the_field(tmp_path, name, damage, loader, field):
    d = str(tmp_path / "ck")
    PyRun("ssgi_full", seeds=dict(ssgi=1, denoise=2)).frames(0, 3).save(d)
    if damage:
        damage(d)
    run = PyRun(loader, seeds=dict(ssgi=5, denoise=6)).frames(0, 2)  # running effects with state of their own, on a used device
    before = _snapshot(run)
    with pytest.raises(state.StateError) as e:
        run.load(d)
    assert e.value.field == field and field in str(e.value)
    assert _snapshot(run) == before  # validated first, then applied: nothing was touched


def test_load_refuses_a_target_type_that_differs(tmp_path):
    d = str(tmp_path / "ck")
    PyRun("traa_half").frames(0, 3).save(d)
    run = PyRun("traa_float").frames(0, 2)
    before = _snapshot(run)
    with pytest.raises(state.StateError) as e:
        run.load(d)
    assert e.value.field == "effects[0].temporalReprojectPass.targetType"
    assert _snapshot(run) == before
    assert PyRun("traa_float").load(d)["effects"][0]["temporalReprojectPass"]["targetType"] == effect.HalfFloatType  # no pass yet: built from the record


# ---- interrupted saves
class _Interrupted(Exception):
    pass


def test_an_interrupted_save_keeps_the_earlier_checkpoint(tmp_path, monkeypatch):
    """The writer fails (half-way through the file it is writing) after k files, for every k: what loads afterwards is the earlier
    checkpoint, bit for bit, never the partial one — and a save that fails before there is any checkpoint leaves none."""
    d = str(tmp_path / "ck")
    run = PyRun("ssgi_full", seeds=dict(ssgi=1, denoise=2)).frames(0, 3)
    n_files = len(state.state_slots(run.effects)) + 1  # the planes and the header
    real_write = state._io_write

    def failing(k):
        count = [0]

        def write(path, offset, data):
            if count[0] == k:
                real_write(path, offset, bytes(data)[:len(data) // 2])
                raise _Interrupted()
            count[0] += 1
            real_write(path, offset, data)
        return write

    for k in range(n_files):  # no earlier checkpoint: nothing loads
        monkeypatch.setattr(state, "_io_write", failing(k))
        with pytest.raises(_Interrupted):
            run.save(d)
        monkeypatch.setattr(state, "_io_write", real_write)
        with pytest.raises(state.StateError):
            PyRun("ssgi_full").load(d)
    run.save(d)
    want = _snapshot(run)
    run.frames(3, 5)
    for k in range(n_files):
        monkeypatch.setattr(state, "_io_write", failing(k))
        with pytest.raises(_Interrupted):
            run.save(d)
        monkeypatch.setattr(state, "_io_write", real_write)
        back = PyRun("ssgi_full")
        back.load(d)
        back_planes = {t: back.r.tex[t].tobytes() for t in state.state_slots(back.effects)}
        fresh = PyRun("ssgi_full")
        fresh.load(d)
        assert json.dumps([e.get_state() for e in back.effects], sort_keys=True) == want[0]
        assert all(want[1][abi.TEX_NAMES[t]] == __import__("hashlib").sha256(b).hexdigest() for t, b in back_planes.items())
    # the rename is the commit: a save that dies right after it has replaced the checkpoint
    monkeypatch.setattr(state, "_io_replace", lambda a, b: (os.replace(a, b), (_ for _ in ()).throw(_Interrupted())))
    with pytest.raises(_Interrupted):
        run.save(d)
    monkeypatch.undo()
    newer = PyRun("ssgi_full")
    newer.load(d)
    assert _snapshot(newer)[0] == _snapshot(run)[0]
    run.save(d)  # and the directory is not littered: one generation of planes, one header
    assert sorted(os.listdir(d)) == sorted(["state.json"] + [p["file"] for p in json.load(open(os.path.join(d, "state.json")))["planes"]])


# ---- the Node host
JS_DRIVER = r"""
const fx = require(process.argv[1] + "/effects")
const { TEX, FORMAT } = require(process.argv[1] + "/Renderer")
const st = require(process.argv[1] + "/state")
""" + MEM_RENDERER_JS + r"""
const job = JSON.parse(process.argv[2])
const { W, H } = job
function frameOf(i) {
  return { width: W, height: H, depth: new Float32Array(W * H).fill(0.5), gbuffer: new Uint32Array(W * H * 4).fill(i + 1),
    velocity: new Uint32Array(W * H * 4).fill(i + 2), direct: new Float32Array(W * H * 4).fill(0.25 * (i + 1)) }
}
const out = {}
for (const step of job.steps) {
  const [kind, options, traaType, withMb] = step.case
  const r = new MemRenderer(W, H)
  const scene = { frame: null }
  const cam = Object.assign({}, job.cameras[0])
  let e, vel
  if (kind === "traa") {
    vel = new fx.VelocityDepthNormalPass(scene, cam)
    e = new fx.TRAAEffect(scene, cam, vel, Object.assign({}, options))
  } else {
    e = new (kind === "ssr" ? fx.SSREffect : fx.SSGIEffect)(null, scene, cam, Object.assign({}, options, { width: W, height: H }), step.seeds)
    vel = e.denoiser.velocityDepthNormalPass
  }
  const mb = withMb ? new fx.MotionBlurEffect(vel, { samples: 8 }) : null
  if (mb && kind === "traa") mb.shareEffectPass(e)
  const effects = mb ? [e, mb] : [e]
  const res = { perFrame: [] }
  try {
    if (step.failAfter !== undefined) {
      const real = st.stateIO.write
      let count = 0
      st.stateIO.write = (file, offset, buf) => {
        if (count === step.failAfter) { real(file, offset, buf.slice(0, buf.length >> 1)); throw new Error("interrupted") }
        count++
        real(file, offset, buf)
      }
    }
    if (step.load) res.loaded = st.loadState(step.load, r, effects)
    for (let i = step.from; i < step.to; i++) {
      const n0 = r.calls.length
      scene.frame = frameOf(i)
      Object.assign(cam, job.cameras[i])
      if (kind === "traa") {
        e.update(r, { texture: { type: traaType === "half" ? fx.HalfFloatType : fx.FloatType }, width: W, height: H, data: scene.frame.direct })
        if (mb) { mb.update(r, null, 1 / 60); mb.mainImage(r) }
      } else {
        e.update(r, null)
        e.mainImage(r)
        if (mb) { mb.update(r, TEX.FINAL, 1 / 60); mb.mainImage(r) }
      }
      res.perFrame.push(r.calls.slice(n0))
    }
    if (step.save) res.saved = st.saveState(step.save, r, effects)
  } catch (err) {
    res.error = { name: err.name, field: err.field, message: err.message }
  }
  res.slots = r.slotDigests()
  res.state = effects.map(x => x.getState())
  out[step.name] = res
}
console.log(JSON.stringify(out))
"""


def run_node(steps):
    job = dict(W=W, H=H, cameras=[camera_of(i) for i in range(FRAMES)], steps=steps)
    return json.loads(subprocess.check_output([node, "-e", JS_DRIVER, JS, json.dumps(job)], cwd=JS))


@needs_node
@pytest.mark.parametrize("case", ["ssgi_full", "ssgi_temporal", "ssr_motion_blur", "traa_half_motion_blur", "ssgi_half_resolution"])
def test_node_and_python_resume_each_others_checkpoints(tmp_path, case):
    seeds = dict(ssgi=101, denoise=202)
    py_dir, js_dir = str(tmp_path / "py"), str(tmp_path / "js")
    straight = PyRun(case, seeds=seeds).frames(0, FRAMES)
    first = PyRun(case, seeds=seeds).frames(0, CUT)
    py_header = first.save(py_dir)
    js = run_node([
        dict(name="straight", case=CASES[case], seeds=seeds, **{"from": 0, "to": FRAMES}),
        dict(name="first", case=CASES[case], seeds=seeds, save=js_dir, **{"from": 0, "to": CUT}),
        dict(name="from_python", case=CASES[case], seeds=None, load=py_dir, **{"from": CUT, "to": FRAMES}),
        dict(name="from_node", case=CASES[case], seeds=None, load=js_dir, **{"from": CUT, "to": FRAMES}),
    ])
    assert not any("error" in v for v in js.values()), js
    # the two hosts drive the double identically to begin with ...
    assert js["straight"]["perFrame"] == straight.per_frame and js["straight"]["slots"] == straight.r.slot_digests()
    # ... write the same checkpoint: plane files byte-identical, headers equal after parsing ...
    js_header = json.load(open(os.path.join(js_dir, "state.json")))
    assert js_header == json.loads(json.dumps(py_header)) == js["first"]["saved"]
    for p in py_header["planes"]:
        assert open(os.path.join(py_dir, p["file"]), "rb").read() == open(os.path.join(js_dir, p["file"]), "rb").read(), p["slot"]
    # ... and continue from either one like the uninterrupted run
    for name in ("from_python", "from_node"):
        assert js[name]["perFrame"] == straight.per_frame[CUT:], name
        assert js[name]["slots"] == straight.r.slot_digests(), name
    resumed = PyRun(case)
    resumed.load(js_dir)
    resumed.frames(CUT, FRAMES)
    assert resumed.per_frame == straight.per_frame[CUT:] and resumed.r.slot_digests() == straight.r.slot_digests()


@needs_node
def test_node_refuses_and_survives_interrupted_saves(tmp_path):
    d = str(tmp_path / "ck")
    seeds = dict(ssgi=1, denoise=2)
    base = PyRun("ssgi_full", seeds=seeds).frames(0, 3)
    base.save(d)
    good = json.load(open(os.path.join(d, "state.json")))
    n_files = len(good["planes"]) + 1
    full = CASES["ssgi_full"]
    # every k: a Node save over the Python checkpoint dies half-way through file k; the Python checkpoint still loads (here, in Node)
    steps = []
    for k in range(n_files):
        steps.append(dict(name="fail%d" % k, case=full, seeds=seeds, save=d, failAfter=k, **{"from": 0, "to": 4}))
        steps.append(dict(name="load%d" % k, case=full, seeds=None, load=d, **{"from": 3, "to": 3}))
    js = run_node(steps)
    for k in range(n_files):
        assert js["fail%d" % k]["error"]["message"] == "interrupted"
        assert "error" not in js["load%d" % k] and js["load%d" % k]["loaded"] == good
        assert js["load%d" % k]["state"] == good["effects"]
        assert all(js["load%d" % k]["slots"][p["slot"]] == base.r.slot_digests()[p["slot"]] for p in good["planes"])
    # refusals, each with its field, the running effects and the double untouched
    damaged = {}
    for name, damage, loader, field in REFUSALS:
        dd = str(tmp_path / ("bad_" + name))
        shutil.copytree(d, dd)
        if damage:
            damage(dd)
        damaged[name] = (dd, loader, field)
    # (fixed seeds: a fresh set of effects of the same case is what "untouched" looks like)
    steps = [dict(name=name, case=CASES[loader], seeds=dict(ssgi=5, denoise=6), load=dd, **{"from": 0, "to": 0}) for name, (dd, loader, field) in damaged.items()]
    fresh = run_node([dict(name="fresh_" + key, case=CASES[key], seeds=dict(ssgi=5, denoise=6), **{"from": 0, "to": 0})
                      for key in sorted({v[1] for v in damaged.values()})])
    refused = run_node(steps)
    for name, (dd, loader, field) in damaged.items():
        err = refused[name].get("error")
        assert err and err["name"] == "StateError" and err["field"] == field and field in err["message"], (name, refused[name])
        assert refused[name]["state"] == fresh["fresh_" + loader]["state"] and refused[name]["slots"] == fresh["fresh_" + loader]["slots"], name
