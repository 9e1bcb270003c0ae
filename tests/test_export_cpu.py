"""CPU (-m "not gpu"): the streamed frame export without a device.  rfx_export_params and its constants in include/rfx.h against rfx_amd/abi.py
and the Node side (compile and print); K7's launch plan, as built, against a brute force over the output bytes; the order in which the two
hosts stage and wait (recording renderers: rfx_amd/frames.py, and run_dump.js itself under node with a recording addon); and the premise of
the U8 tolerance — the share of bytes the margin rule excuses — on the inputs the GPU tests use."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import export_cases as X
from rfx_amd import abi, frames

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")


# ---------------------------------------------------------------- ABI
def test_export_abi_matches_header(tmp_path):
    c = tmp_path / "abi_export.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rfx.h"\nint main(){printf("%d %d %d %d %d %d %d %d %d %d %d %d\\n",'
                 "(int)sizeof(rfx_export_params),(int)offsetof(rfx_export_params,source),(int)offsetof(rfx_export_params,format),"
                 "(int)offsetof(rfx_export_params,channels),(int)offsetof(rfx_export_params,tonemap),(int)offsetof(rfx_export_params,exposure),"
                 "(int)RFX_EXPORT_F32,(int)RFX_EXPORT_F16,(int)RFX_EXPORT_U8_SRGB,(int)RFX_PROF_K7,(int)RFX_PROF_COUNT,RFX_ABI_VERSION);return 0;}\n")
    exe = tmp_path / "abi_export"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    proto = tmp_path / "proto.c"  # the four prototypes, as the hosts call them (compiled, not linked)
    proto.write_text('#include "rfx.h"\n'
                     "size_t (*a)(const rfx_ctx *, const rfx_export_params *) = rfx_export_bytes;\n"
                     "int (*b)(rfx_ctx *, const rfx_export_params *, void *, size_t) = rfx_export;\n"
                     "int (*d)(rfx_ctx *, const rfx_export_params *, void *, size_t, int *) = rfx_stage_export;\n"
                     "int (*e)(rfx_ctx *, int) = rfx_export_wait;\n")
    subprocess.check_call(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o", str(tmp_path / "proto.o")])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = abi.ExportParams
    assert got == [C.sizeof(P), P.source.offset, P.format.offset, P.channels.offset, P.tonemap.offset, P.exposure.offset,
                   abi.EXPORT_F32, abi.EXPORT_F16, abi.EXPORT_U8_SRGB, abi.PROF_KINDS.index("k7_export"), len(abi.PROF_KINDS), abi.RFX_ABI_VERSION]
    assert got[9] == got[10] - 1  # appended: no earlier kind moved
    assert abi.EXPORT_FORMATS == {"f32": abi.EXPORT_F32, "f16": abi.EXPORT_F16, "u8_srgb": abi.EXPORT_U8_SRGB}
    assert {k: np.dtype(v).itemsize for k, v in abi.EXPORT_DTYPE.items()} == {abi.EXPORT_F32: 4, abi.EXPORT_F16: 2, abi.EXPORT_U8_SRGB: 1}
    lib = abi.load_library()
    for name in ("rfx_export_bytes", "rfx_export", "rfx_stage_export", "rfx_export_wait"):
        assert name in abi.EXPORTS and hasattr(lib, name)
    assert lib.rfx_abi_version() == abi.RFX_ABI_VERSION


@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_constants_agree():
    js = ("const r=require(%r);console.log(JSON.stringify({c:r.constants(),e:r.EXPORT,k:r.PROF_KINDS,v:r.abiVersion(),"
          "a:[0,1,2].map(f=>r.EXPORT_ARRAY[f].BYTES_PER_ELEMENT)}))" % os.path.join(JS, "Renderer"))
    got = json.loads(subprocess.check_output([node, "-e", js], text=True))
    assert got["c"] == {"EXPORT_F32": abi.EXPORT_F32, "EXPORT_F16": abi.EXPORT_F16, "EXPORT_U8_SRGB": abi.EXPORT_U8_SRGB, "PROF_K7": abi.PROF_KINDS.index("k7_export"),
                        "PROF_COUNT": len(abi.PROF_KINDS), "TEX_COUNT": abi.TEX_COUNT, "ABI_VERSION": abi.RFX_ABI_VERSION}
    assert got["e"] == {"F32": abi.EXPORT_F32, "F16": abi.EXPORT_F16, "U8_SRGB": abi.EXPORT_U8_SRGB}
    assert got["k"] == list(abi.PROF_KINDS) and got["v"] == abi.RFX_ABI_VERSION and got["a"] == [4, 2, 1]


# ---------------------------------------------------------------- the launch plan, as built
class Plan(C.Structure):  # rfx_launch.h rfx_export_plan
    _fields_ = [("pixels", C.c_int), ("groups", C.c_int), ("blocks", C.c_int), ("tail_start", C.c_int), ("tail_pixels", C.c_int),
                ("elem_bytes", C.c_int), ("pixel_bytes", C.c_int), ("group_bytes", C.c_int), ("bytes", C.c_ulonglong)]


BLOCK = 256  # rfx_launch.h RFX_K7_BLOCK
ELEM = {abi.EXPORT_F32: 4, abi.EXPORT_F16: 2, abi.EXPORT_U8_SRGB: 1}


def _plan(pixels, fmt, ch):
    lib = abi.load_library()
    lib.rfx_internal_export_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(Plan)]
    p = Plan()
    assert lib.rfx_internal_export_plan(pixels, fmt, ch, C.byref(p)) == abi.RFX_OK
    return p


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("fmt", [abi.EXPORT_F32, abi.EXPORT_F16, abi.EXPORT_U8_SRGB])
def test_export_plan_against_brute_force(fmt, ch):
    for pixels in list(range(1, 131)) + [97 * 55, 3840 * 2160]:
        p = _plan(pixels, fmt, ch)
        px_bytes = ELEM[fmt] * ch
        assert (p.pixels, p.elem_bytes, p.pixel_bytes, p.group_bytes) == (pixels, ELEM[fmt], px_bytes, 4 * px_bytes)
        assert p.group_bytes in (12, 16, 24, 32, 48, 64)
        assert p.tail_start == pixels - pixels % 4 and p.tail_pixels == pixels % 4 and p.groups == pixels // 4
        assert p.bytes == pixels * px_bytes
        # the lanes the grid launches: t < groups stores [t * group_bytes, (t + 1) * group_bytes) as whole dwords, t == groups the tail's elements
        need = p.groups + (1 if p.tail_pixels else 0)
        assert p.blocks == (need + BLOCK - 1) // BLOCK
        lanes = p.blocks * BLOCK
        assert p.group_bytes % 4 == 0  # every body store starts on a dword: t * group_bytes
        if pixels <= 97 * 55:  # brute force: every output byte exactly once
            written = np.zeros(p.bytes, np.int32)
            for t in range(lanes):
                if t < p.groups:
                    assert (t * p.group_bytes) % 4 == 0
                    written[t * p.group_bytes:(t + 1) * p.group_bytes] += 1
                elif t == p.groups:
                    for k in range(p.tail_pixels):
                        for c in range(ch):
                            o = ((p.tail_start + k) * ch + c) * p.elem_bytes
                            written[o:o + p.elem_bytes] += 1
            assert (written == 1).all()
        else:  # 4K: the same by arithmetic (a multiple of four pixels: no tail)
            assert p.groups * p.group_bytes + p.tail_pixels * px_bytes == p.bytes and p.tail_pixels == 0
            assert (p.groups - 1) * p.group_bytes + p.group_bytes <= p.bytes
    lib = abi.load_library()
    bad = Plan()
    for args in ((0, fmt, ch), (-4, fmt, ch), (16, fmt, 2), (16, fmt, 5), (16, 3, ch), (16, -1, ch)):
        assert lib.rfx_internal_export_plan(*args, C.byref(bad)) == abi.RFX_EINVAL


# ---------------------------------------------------------------- orchestration: the Python host
class _RecCtx:
    """a recording stand-in for Context (the pattern of tests/state_mem_renderer.py): draws and export calls in order"""
    W, H, tile_rows = 8, 4, 4

    def __init__(self):
        self.calls, self.ticket, self.in_flight, self.max_in_flight, self._bufs = [], 0, set(), 0, {}

    def host_alloc(self, shape, dtype):
        return np.zeros(shape, dtype)

    def draw(self, frame):
        self.calls.append(("draw", frame))

    def stage_export(self, source, format, channels=3, tonemap="linear", exposure=1.0, *, out):
        self.ticket += 1
        assert not any(out is self._bufs[t] for t in self.in_flight), "a buffer was staged again before its export was waited for"
        self.in_flight.add(self.ticket)
        self._bufs[self.ticket] = out
        self.max_in_flight = max(self.max_in_flight, len(self.in_flight))
        self.calls.append(("stage", self.ticket, source, format, channels, tonemap, exposure))
        return self.ticket

    def export_wait(self, ticket):
        self.in_flight.discard(ticket)
        self.calls.append(("wait", ticket))


def _check_order(calls, n):
    """calls: ("draw", i) / ("stage", ticket) / ("wait", ticket), tickets 1..n in frame order"""
    pos = {(c[0], c[1]): k for k, c in enumerate(calls)}
    in_flight = most = 0
    for c in calls:
        in_flight += (c[0] == "stage") - (c[0] == "wait")
        most = max(most, in_flight)
    assert most <= 2 and in_flight == 0
    for i in range(n):
        assert pos[("draw", i)] < pos[("stage", i + 1)] < pos[("wait", i + 1)]
        if i + 1 < n:  # the wait for frame i comes after frame i + 1's draws (and its staging)
            assert pos[("wait", i + 1)] > pos[("draw", i + 1)] and pos[("wait", i + 1)] > pos[("stage", i + 2)]
    assert [c for c in calls if c[0] != "draw"][-1] == ("wait", n)  # the last ticket is waited for


@pytest.mark.parametrize("fmt,want", [("png", ("u8_srgb", 3, "aces", 0.5)), ("exr", ("f16", 4, "linear", 1.0)), ("pfm", ("f32", 3, "linear", 1.0))])
def test_python_frame_exporter_call_order(fmt, want):
    ctx = _RecCtx()
    written = []
    ex = frames.FrameExporter(ctx, "unused", fmt, tonemap="aces", exposure=0.5, write=lambda i, a: written.append((i, a.dtype, a.shape)))
    for i in range(5):
        ctx.draw(i)
        ex.submit(abi.TEX_FINAL)
    ex.finish()
    _check_order([c[:2] for c in ctx.calls], 5)
    assert ctx.max_in_flight == 2
    assert all(c[2:] == (abi.TEX_FINAL,) + want for c in ctx.calls if c[0] == "stage")
    dtype = abi.EXPORT_DTYPE[abi.EXPORT_FORMATS[want[0]]]
    assert written == [(i, np.dtype(dtype), (4, 8, want[1])) for i in range(5)]
    with pytest.raises(ValueError):
        frames.FrameExporter(ctx, "unused", "jpg")


# ---------------------------------------------------------------- orchestration: run_dump.js itself, on a recording addon
RECORDING_ADDON = r"""
// preloaded with `node -r`: every require of the N-API addon gets this recording stand-in
const Module = require("module"), fs = require("fs")
const calls = []
let ticket = 0, W = 0, H = 0
const DRAWS = new Set(["ssgiMarch", "ssgiTrace", "ssgiShade", "temporalReproject", "poissonDenoise", "compose", "finalCompose", "motionBlur", "copyFramebuffer"])
const base = {
  abiVersion: () => 21, constants: () => ({}),
  create(dev, w, h) { W = w; H = h; return {} },
  heldRows: (h, tex) => [0, tex === 4 ? 128 : H],
  ssgiTargetRows: () => [0, H],
  hostAlloc: bytes => new ArrayBuffer(bytes),
  haloViolations: () => 0,
  exportBytes: () => 0,
  stageExport(h, p, out) { calls.push(["stage", ++ticket, p.source, p.format, p.channels, p.tonemap, p.exposure, out.constructor.name, out.length]); return ticket },
  exportWait(h, t) { calls.push(["wait", t]) }
}
const addon = new Proxy(base, { get(t, name) {
  if (name in t) return t[name]
  return (...a) => { if (DRAWS.has(name)) calls.push(["draw", name]); else if (name === "stageFlip" || name === "sync") calls.push([name]) }
} })
const load = Module._load
Module._load = function (request) { return /rfx_napi\.node$/.test(request) ? addon : load.apply(this, arguments) }
process.on("exit", () => fs.writeFileSync(process.env.RFX_RECORD, JSON.stringify(calls)))
"""


def _record_run_dump(tmp_path, extra, frames_n=3):
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    dirs = []
    for i in range(frames_n):
        d = str(tmp_path / ("dump%d" % i))
        if not os.path.isdir(d):
            write_dump(d, synthetic_frame(32, 16, i))
        dirs.append(d)
    pre = tmp_path / "recording_addon.js"
    pre.write_text(RECORDING_ADDON)
    rec = str(tmp_path / "calls.json")
    env = dict(os.environ, RFX_RECORD=rec)
    p = subprocess.run([node, "-r", str(pre), os.path.join(JS, "run_dump.js")] + dirs + ["--out", str(tmp_path / "out")] + extra, env=env, capture_output=True, text=True)
    return p, (json.load(open(rec)) if os.path.exists(rec) else None)


@pytest.mark.skipif(node is None, reason="node not installed")
@pytest.mark.parametrize("variant", ["plain", "stream", "motion_blur"])
def test_run_dump_stages_and_waits_one_frame_late(tmp_path, variant):
    extra = {"plain": [], "stream": ["--stream", "true"], "motion_blur": ["--motionBlur", '{"samples":4}']}[variant]
    written = str(tmp_path / "frames")
    p, calls = _record_run_dump(tmp_path, extra + ["--framesOut", written, "--framesFormat", '"exr"'])
    assert p.returncode == 0, p.stderr
    # frames in draw order: a frame's draws end with its last draw before the stage
    seq, frame = [], 0
    for c in calls:
        if c[0] == "draw":
            if not seq or seq[-1] != ("draw", frame):
                seq.append(("draw", frame))
        elif c[0] == "stage":
            seq.append(("stage", c[1]))
            frame += 1
        elif c[0] == "wait":
            seq.append(("wait", c[1]))
    seq = [s for s in seq if not (s[0] == "draw" and s[1] >= 3)]  # (the closing mainImage for final.bin)
    _check_order(seq, 3)
    stages = [c for c in calls if c[0] == "stage"]
    src = abi.TEX_MOTION_BLUR if variant == "motion_blur" else abi.TEX_FINAL
    assert [c[2:] for c in stages] == [[src, abi.EXPORT_F16, 4, 0, 1, "Uint16Array", 32 * 16 * 4]] * 3
    # what the frame shows is drawn before it is staged: the effect's own fragment (and the blur)
    for k, c in enumerate(calls):
        if c[0] == "stage":
            before = [d[1] for d in calls[:k] if d[0] == "draw"]
            assert before[-1] == ("motionBlur" if variant == "motion_blur" else "finalCompose")
    if variant == "stream":  # the effect's fragment reads this frame's planes: staged before the flip
        kinds = [c[0] for c in calls if c[0] in ("stage", "stageFlip")]
        assert kinds == ["stageFlip"] + ["stage", "stageFlip"] * 3
    assert sorted(os.listdir(written)) == ["frame_%05d.exr" % i for i in range(3)]
    # without --framesOut: the same draws, no export call
    p2, calls2 = _record_run_dump(tmp_path, extra)
    assert p2.returncode == 0, p2.stderr
    assert not [c for c in calls2 if c[0] in ("stage", "wait")]
    draws = lambda cs: [c[1] for c in cs if c[0] == "draw"]
    if variant == "motion_blur":
        assert draws(calls) == draws(calls2)
    else:  # one more finalCompose per frame (it writes TEX.FINAL only), nothing else
        assert [d for d in draws(calls) if d != "finalCompose"] == [d for d in draws(calls2) if d != "finalCompose"]
        assert draws(calls).count("finalCompose") == draws(calls2).count("finalCompose") + 3


@pytest.mark.skipif(node is None, reason="node not installed")
def test_run_dump_png_params_and_ranks_refused(tmp_path):
    p, calls = _record_run_dump(tmp_path, ["--framesOut", str(tmp_path / "f"), "--tonemap", '"linear"', "--exposure", "0.37"], frames_n=2)
    assert p.returncode == 0, p.stderr
    got = [c[2:] for c in calls if c[0] == "stage"]
    assert len(got) == 2 and got[0][:4] == [abi.TEX_FINAL, abi.EXPORT_U8_SRGB, 3, 0] and abs(got[0][4] - 0.37) < 1e-12 and got[0][5:] == ["Uint8Array", 32 * 16 * 3]
    assert sorted(os.listdir(tmp_path / "f")) == ["frame_00000.png", "frame_00001.png"]
    p, calls = _record_run_dump(tmp_path, ["--framesOut", str(tmp_path / "g"), "--ranks", "2"], frames_n=2)
    assert p.returncode != 0 and "--framesOut" in p.stderr and "--ranks" in p.stderr
    assert not calls and not os.path.exists(tmp_path / "g")


@pytest.mark.skipif(node is None, reason="node not installed")
def test_run_dump_frames_out_with_traa_and_checkpoints(tmp_path):
    staged = lambda calls: [c[2] for c in calls if c[0] == "stage"]
    fr = str(tmp_path / "fr")
    p, calls = _record_run_dump(tmp_path, ["--traa", '"half"', "--framesOut", fr, "--framesFormat", '"pfm"'])
    assert p.returncode == 0 and staged(calls) == [abi.TEX_TEMPORAL0] * 3, p.stderr  # TRAA's accumulated colour
    p, calls = _record_run_dump(tmp_path, ["--traa", '"float"', "--motionBlur", '{"samples":4}', "--framesOut", fr, "--framesFormat", '"exr"'])
    assert p.returncode == 0 and staged(calls) == [abi.TEX_MOTION_BLUR] * 3, p.stderr
    p, calls = _record_run_dump(tmp_path, ["--traa", '"half"', "--framesOut", fr, "--framesFormat", '"exr"'])  # alpha 1 is the host's
    assert p.returncode != 0 and "--framesOut" in p.stderr and not staged(calls)
    p, calls = _record_run_dump(tmp_path, ["--saveState", str(tmp_path / "ck"), "--saveEvery", "1", "--framesOut", fr])
    assert p.returncode == 0 and staged(calls) == [abi.TEX_FINAL] * 3, p.stderr
    assert [c[1] for c in calls if c[0] == "wait"] == [1, 2, 3]


# ---------------------------------------------------------------- the premise of the U8 tolerance
@pytest.mark.parametrize("case", X.u8_cases(), ids=X.case_id)
def test_share_excused_by_the_margin_rule(case):
    """the GPU tests' own inputs: at most 1 % of a case's bytes lie within DELTA of a rounding boundary (a uniform v: 0.2 %)"""
    W, H, channels, family, exposure, operator = case
    v, ref = X.reference_v(X.linear_input(W, H, family), channels, operator, exposure)
    share = float(X.excluded(v).mean())
    print("%s: excused share %.5f of %d bytes" % (X.case_id(case), share, v.size))
    assert share <= X.SHARE_CAP
    # ... and the rule is met by an fp32 evaluation on the host: numpy float32 arithmetic in the kernel's order
    X.check_margin(_fp32_chain(X.linear_input(W, H, family), channels, operator, exposure), v, ref)


def _fp32_chain(linear, channels, operator, exposure):
    f = np.float32
    a = np.asarray(linear, f)
    c = a[..., :3]
    c = np.where(np.isnan(c), f(0), c)
    c = np.minimum(np.maximum(c, f(0)), f(65504)) * f(exposure)
    if operator == "aces":
        c = c / f(0.6)
        r, g, b = c[..., 0], c[..., 1], c[..., 2]
        fit = lambda x: (x * (x + f(0.0245786)) - f(0.000090537)) / (x * (f(0.983729) * x + f(0.4329510)) + f(0.238081))
        x, y, z = (fit(f(0.59719) * r + f(0.35458) * g + f(0.04823) * b), fit(f(0.07600) * r + f(0.90834) * g + f(0.01566) * b),
                   fit(f(0.02840) * r + f(0.13383) * g + f(0.83777) * b))
        c = np.stack([f(1.60475) * x + f(-0.53108) * y + f(-0.07367) * z, f(-0.10208) * x + f(1.10813) * y + f(-0.00605) * z,
                      f(-0.00327) * x + f(-0.07276) * y + f(1.07602) * z], -1)
    c = np.where(np.isnan(c), f(0), c)
    c = np.minimum(np.maximum(c, f(0)), f(1))
    with np.errstate(divide="ignore"):
        s = np.where(c <= f(0.0031308), c * f(12.92), f(1.055) * np.exp2(f(1.0 / 2.4) * np.log2(c)).astype(f) - f(0.055))
    out = (s * f(255) + f(0.5)).astype(np.uint8)
    if channels == 4:
        al = a[..., 3:4]
        al = np.minimum(np.maximum(np.where(np.isnan(al), f(0), al), f(0)), f(1))
        out = np.concatenate([out, (al * f(255) + f(0.5)).astype(np.uint8)], -1)
    return out
