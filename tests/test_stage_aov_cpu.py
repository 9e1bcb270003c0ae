"""CPU (-m "not gpu") side of the streamed AOV frames (include/rfx.h rfx_stage_aov): the header against the ctypes mirror, the launch plan as
the library computes it (rfx_launch.h rfx_aov_plan_for, through the host simulator's build) against a restatement of the row rule, the typed
importer (imageio.narrow_exact / exr_to_typed_planes), the typed dump files on both hosts, and a run of tests/test_gpu_stage_aov.py on the host
simulator, so that the entry point's logic is exercised where there is no device."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from launch_plans import needs_hostsim
from rfx_amd import abi, dump, imageio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
NAMES = abi.AOV_PLANES
FULL = dict(diffuse=4, normal=3, roughness=1, metalness=1, emissive=3, velocity=2, depth=1, direct=4)
TYPED = {k: (0 if k in ("velocity", "depth") else 1) for k in NAMES}  # RFX_PLANE_F16 for every plane but velocity and depth


def test_header_and_ctypes_mirror_agree(tmp_path):
    fields = ", ".join("offsetof(rfx_aov_frame, %s)" % n for n in NAMES)
    c = tmp_path / "aov.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rfx.h"\nint main(){size_t v[] = {(size_t)RFX_PLANE_F32, (size_t)RFX_PLANE_F16, sizeof(rfx_plane), '
                 "offsetof(rfx_plane, data), offsetof(rfx_plane, type), offsetof(rfx_plane, channels), sizeof(rfx_aov_frame), %s, (size_t)RFX_ABI_VERSION};\n"
                 'for (unsigned i = 0; i < sizeof v / sizeof v[0]; i++) printf("%%zu ", v[i]);\nreturn 0;}\n' % fields)
    exe = tmp_path / "aov"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [abi.PLANE_F32, abi.PLANE_F16, C.sizeof(abi.Plane), abi.Plane.data.offset, abi.Plane.type.offset, abi.Plane.channels.offset, C.sizeof(abi.AovFrame)] + [
        getattr(abi.AovFrame, n).offset for n in NAMES] + [abi.RFX_ABI_VERSION]
    assert got == want
    assert C.sizeof(abi.AovFrame) == 8 * C.sizeof(abi.Plane) and abi.RFX_ABI_VERSION == 21  # additive: no version bump
    lib = abi.load_library()
    for name in ("rfx_aov_stage_bytes", "rfx_stage_aov"):
        assert name in abi.EXPORTS and hasattr(lib, name)
    assert abi.PLANE_TYPES == {np.dtype(np.float32): 0, np.dtype(np.float16): 1}


_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
I, U = ctypes.c_int, ctypes.c_ulonglong
class Seg(ctypes.Structure):
    _fields_ = [(n, I) for n in ("row0", "rows", "full", "pixels", "groups", "blocks", "tail_start", "tail_pixels")] + [("offset", U * 8)]
class Plan(ctypes.Structure):
    _fields_ = [("nseg", I), ("seg", Seg * 3), ("plane_row0", I * 8), ("plane_rows", I * 8), ("elem_bytes", I * 8), ("write_gbuffer", I), ("write_velocity", I),
                ("write_direct", I), ("copy_bytes", U), ("stage_bytes", U)]
lib.rfx_internal_aov_plan.argtypes = [I, I, I, I, ctypes.POINTER(I), ctypes.POINTER(I), I, I, ctypes.POINTER(Plan)]
out = []
for W, H, h0, hn, types, chans, r0, n in json.load(sys.stdin):
    t = Plan()
    rc = lib.rfx_internal_aov_plan(W, H, h0, hn, (I * 8)(*types), (I * 8)(*chans), r0, n, ctypes.byref(t))
    d = dict(rc=rc)
    if rc == 0:
        d.update({k: getattr(t, k) for k in ("nseg", "write_gbuffer", "write_velocity", "write_direct", "copy_bytes", "stage_bytes")})
        d.update(plane_row0=list(t.plane_row0), plane_rows=list(t.plane_rows), elem_bytes=list(t.elem_bytes))
        d["seg"] = [dict({k: getattr(s, k) for k, _ in Seg._fields_[:8]}, offset=[None if o == 2 ** 64 - 1 else o for o in s.offset]) for s in t.seg[:t.nseg]]
    out.append(d)
json.dump(out, sys.stdout)
"""


def aov_plans(cases):
    """[(W, H, held_row0, held_rows, {name: type}, {name: channels, 0 = not given}, row0, rows)] -> one dict per case"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    from conftest import hostsim_child_env
    env = dict(os.environ, **hostsim_child_env(sim))
    rows = [[W, H, h0, hn, [ty.get(k, 0) for k in NAMES], [ch.get(k, 0) for k in NAMES], r0, n] for W, H, h0, hn, ty, ch, r0, n in cases]
    p = subprocess.run([sys.executable, "-c", _CHILD, env["RFX_TEST_LIB"]], input=json.dumps(rows), capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout)


def row_rule(W, H, h0, hn, ty, ch, r0, n):
    """The contract restated: DEPTH holds every row, the other slots [h0, h0 + hn); a written slot receives band ∩ its rows; a plane is copied
    for the rows some slot that reads it receives.  -> ({plane: (first row, rows)}, bytes)"""
    given = {k for k in NAMES if ch.get(k, 0)}
    gbuffer = {"diffuse", "normal", "roughness", "metalness", "emissive"} <= given
    inner = (max(r0, h0), max(0, min(r0 + n, h0 + hn) - max(r0, h0)))
    readers = dict(diffuse=gbuffer, roughness=gbuffer, metalness=gbuffer, emissive=gbuffer, normal=gbuffer or "velocity" in given, velocity="velocity" in given,
                   direct="direct" in given)
    rows, total = {}, 0
    for k in given:
        first, cnt = (r0, n) if k == "depth" else (inner if readers[k] else (0, 0))
        rows[k] = (first, cnt)
        total += cnt * W * ch[k] * (2 if ty.get(k, 0) else 4)
    return rows, total


@needs_hostsim
def test_aov_plan_rows_offsets_groups_and_tail():
    f32 = {}
    no_direct = {k: v for k, v in FULL.items() if k != "direct"}
    depth_direct3 = dict(depth=1, direct=3)
    vel = dict(depth=1, velocity=2, normal=3)
    tile = (96, 54, 16, 26)  # tile_y0 20, 18 rows, halo 4: the slots but DEPTH hold rows [16, 42)
    cases = [(97, 55, 0, 55, TYPED, FULL, 0, 55), (5, 3, 0, 3, f32, FULL, 0, 3), tile + (TYPED, FULL, 0, 54), tile + (f32, FULL, 0, 54),
             tile + (TYPED, FULL, 0, 16), tile + (TYPED, FULL, 10, 10), tile + (TYPED, FULL, 30, 24), tile + (TYPED, FULL, 42, 12), tile + (TYPED, FULL, 20, 5),
             tile + (TYPED, no_direct, 0, 54), tile + (dict(TYPED, depth=1), depth_direct3, 0, 54), tile + (f32, dict(depth=1), 3, 40), tile + (TYPED, vel, 0, 54),
             (97, 55, 17, 25, dict(TYPED, normal=0), dict(FULL, direct=3, diffuse=3), 0, 55)]
    plans = aov_plans(cases)
    for case, t in zip(cases, plans):
        W, H, h0, hn, ty, ch, r0, n = case
        assert t["rc"] == 0, case
        rows, total = row_rule(*case)
        assert t["copy_bytes"] == total, case
        for i, k in enumerate(NAMES):
            first, cnt = rows.get(k, (0, 0))
            assert t["plane_rows"][i] == cnt and (cnt == 0 or t["plane_row0"][i] == first), (case, k)
            assert t["elem_bytes"][i] == (0 if not ch.get(k, 0) else 2 if ty.get(k, 0) else 4)
        # the segments tile the band, in order, and only the one inside the held rows is full
        assert 1 <= t["nseg"] <= 3 and t["seg"][0]["row0"] == r0 and sum(s["rows"] for s in t["seg"]) == n
        pieces = []
        for j, s in enumerate(t["seg"]):
            assert s["rows"] > 0 and (j == 0 or s["row0"] == t["seg"][j - 1]["row0"] + t["seg"][j - 1]["rows"])
            assert s["pixels"] == s["rows"] * W and s["groups"] == s["pixels"] // 4 and s["tail_start"] == 4 * s["groups"] and s["tail_pixels"] == s["pixels"] % 4
            assert s["blocks"] == -(-(s["groups"] + (1 if s["tail_pixels"] else 0)) // 256) and s["blocks"] >= 1
            if s["full"]:
                assert h0 <= s["row0"] and s["row0"] + s["rows"] <= h0 + hn and (t["write_gbuffer"] or t["write_velocity"] or t["write_direct"])
            for i, k in enumerate(NAMES):
                o = s["offset"][i]
                reads = bool(ch.get(k, 0)) and (k == "depth" or (s["full"] and rows[k][1] > 0))
                assert (o is not None) == reads, (case, j, k)
                if reads:
                    assert o % 256 == 0
                    pieces.append((o, s["pixels"] * ch[k] * t["elem_bytes"][i]))
        assert sum(s["full"] for s in t["seg"]) == (1 if any(cnt for k, (_, cnt) in rows.items() if k != "depth") else 0)
        pieces.sort()
        for (o, b), (o2, _) in zip(pieces, pieces[1:]):
            assert o + b <= o2, case
        assert pieces[-1][0] + pieces[-1][1] <= t["stage_bytes"] and sum(b for _, b in pieces) == t["copy_bytes"]
        assert t["stage_bytes"] <= 76 * n * W + 256 * len(pieces)  # the staging memory: at most 76 B per band pixel, and the alignment
    whole, small, tiled = plans[0], plans[1], plans[2]
    assert (whole["nseg"], whole["seg"][0]["groups"], whole["seg"][0]["tail_start"], whole["seg"][0]["tail_pixels"], whole["seg"][0]["blocks"]) == (1, 1333, 5332, 3, 6)
    assert whole["copy_bytes"] == 44 * 97 * 55
    assert (small["nseg"], small["seg"][0]["groups"], small["seg"][0]["tail_pixels"], small["seg"][0]["blocks"], small["copy_bytes"]) == (1, 3, 3, 1, 76 * 15)
    assert [(s["row0"], s["rows"], s["full"]) for s in tiled["seg"]] == [(0, 16, 0), (16, 26, 1), (42, 12, 0)]
    assert tiled["copy_bytes"] == 96 * (54 * 4 + 26 * 40)
    assert [(s["row0"], s["rows"], s["full"]) for s in plans[4]["seg"]] == [(0, 16, 0)]  # a band that misses the held rows: depth alone
    assert (plans[10]["write_gbuffer"], plans[10]["write_velocity"], plans[10]["write_direct"]) == (0, 0, 1)
    assert (plans[12]["write_gbuffer"], plans[12]["write_velocity"], plans[12]["write_direct"]) == (0, 1, 0)
    # what rfx_stage_aov answers RFX_EINVAL to
    bad = [tile + (dict(TYPED, depth=2), FULL, 0, 54), tile + (dict(TYPED, emissive=-1), FULL, 0, 54), tile + (TYPED, dict(FULL, normal=4), 0, 54),
           tile + (TYPED, dict(FULL, velocity=3), 0, 54), tile + (TYPED, dict(FULL, diffuse=2), 0, 54), tile + (TYPED, dict(FULL, direct=5), 0, 54),
           tile + (TYPED, dict(FULL, depth=0), 0, 54), tile + (TYPED, dict(FULL, roughness=0), 0, 54), tile + (TYPED, dict(FULL, normal=0, velocity=0), 0, 54),
           tile + (TYPED, dict(depth=1, normal=3), 0, 54), tile + (TYPED, dict(depth=1, velocity=2), 0, 54), tile + (TYPED, FULL, 0, 0), tile + (TYPED, FULL, -1, 4),
           tile + (TYPED, FULL, 50, 5)]
    assert [t["rc"] for t in aov_plans(bad)] == [abi.RFX_EINVAL] * len(bad)


def test_narrow_exact():
    rng = np.random.RandomState(3)
    halves = rng.randn(64, 5).astype(np.float16)
    for a in (halves.astype(np.float32), np.array([1, 0x3ff, 0x400, 0x8001, 0x83ff], np.uint16).view(np.float16).astype(np.float32),  # denormals, the first normal
              np.array([0.0, -0.0, np.inf, -np.inf, 65504.0, -65504.0], np.float32)):
        h = imageio.narrow_exact(a)
        assert h.dtype == np.float16 and h.shape == a.shape and h.astype(np.float32).tobytes() == a.tobytes()
    assert imageio.narrow_exact(np.array([-0.0], np.float32)).view(np.uint16)[0] == 0x8000
    for a in (rng.randn(64).astype(np.float32), np.array([1.0, 65520.0], np.float32), np.array([1.0, 2.0 ** -25], np.float32), np.array([0.1], np.float32),
              np.array([1.0, np.float32(1) + np.float32(2.0 ** -11)], np.float32)):
        assert imageio.narrow_exact(a) is a  # (65520 is the first float that rounds to the half infinity)
    assert imageio.narrow_exact(halves) is halves


def _exr_channels(planes):
    ch = {}
    for key, names in imageio.AOV_LAYOUT.items():
        a = planes[key][..., None] if planes[key].ndim == 2 else planes[key]
        for i, n in enumerate(names):
            ch[n] = a[..., i]
    return ch


def _frame_planes(W=23, H=9, seed=7):
    rng = np.random.RandomState(seed)
    return {k: rng.rand(*((H, W, ch) if ch > 1 else (H, W))).astype(np.float32) for k, ch in FULL.items()}


@pytest.mark.parametrize("compression", ["zip", "piz"])
def test_exr_to_typed_planes(tmp_path, compression):
    p = _frame_planes()
    ch = _exr_channels(p)
    # every channel HALF
    path = str(tmp_path / "half.exr")
    imageio.write_exr(path, ch, compression, half=True)
    assert set(imageio.exr_channel_types(path).values()) == {"half"}
    t, d = imageio.exr_to_typed_planes(path), imageio.exr_to_dump_planes(path)
    flat_t, flat_d = dict(t["aov"], depth=t["depth"], direct=t["direct"]), dict(d["aov"], depth=d["depth"], direct=d["direct"])
    for k in NAMES:
        assert flat_t[k].dtype == np.float16 and flat_d[k].dtype == np.float32 and flat_t[k].shape == p[k].shape
        assert flat_t[k].astype(np.float32).tobytes() == flat_d[k].tobytes() and flat_t[k].tobytes() == p[k].astype(np.float16).tobytes()
    # mixed: velocity and depth FLOAT (the 44 B/px frame); one layer with a single FLOAT channel among HALF ones stays float32; no alpha layers
    path = str(tmp_path / "mixed.exr")
    half = {n for k, names in imageio.AOV_LAYOUT.items() if k not in ("velocity", "depth") for n in names} - {"emissive.G"}
    ch3 = {n: v for n, v in ch.items() if n not in ("diffuse.A", "direct.A")}
    imageio.write_exr(path, ch3, compression, half=half)
    types_ = imageio.exr_channel_types(path)
    assert types_["velocity.X"] == "float" and types_["emissive.G"] == "float" and types_["emissive.R"] == "half" and "diffuse.A" not in types_
    t, d = imageio.exr_to_typed_planes(path), imageio.exr_to_dump_planes(path)
    flat_t, flat_d = dict(t["aov"], depth=t["depth"], direct=t["direct"]), dict(d["aov"], depth=d["depth"], direct=d["direct"])
    assert {k for k in NAMES if flat_t[k].dtype == np.float16} == {"diffuse", "normal", "roughness", "metalness", "direct"}
    for k in NAMES:
        assert flat_t[k].shape == p[k].shape and flat_t[k].astype(np.float32).tobytes() == flat_d[k].tobytes()
    assert (flat_t["diffuse"][..., 3] == 1).all() and (flat_t["direct"][..., 3] == 1).all()
    assert flat_t["velocity"].tobytes() == p["velocity"].tobytes() and flat_t["depth"].tobytes() == p["depth"].tobytes()


_NODE_DUMP = r"""
const { readDump } = require(process.argv[1] + "/dump.js")
const f = readDump(process.argv[2])
const crypto = require("crypto")
const out = {}
const all = Object.assign({ depth: f.depth, direct: f.direct }, f.aov)
for (const k of Object.keys(all)) out[k] = [all[k].constructor.name, all[k].length, crypto.createHash("sha1").update(Buffer.from(all[k].buffer, all[k].byteOffset, all[k].byteLength)).digest("hex")]
console.log(JSON.stringify(out))
"""


def test_typed_dump_round_trip(tmp_path):
    import hashlib
    import types
    from rfx_amd.scene import synthetic_frame
    W, H = 23, 9
    p = _frame_planes(W, H)
    cam = synthetic_frame(8, 8, 0).camera
    aov = {k: p[k] for k in NAMES if k not in ("depth", "direct")}
    frame = types.SimpleNamespace(width=W, height=H, camera=cam, depth=p["depth"], direct=p["direct"][..., :3], aov=aov)
    half = ("diffuse", "normal", "roughness", "metalness", "emissive", "direct")
    d = str(tmp_path / "typed")
    dump.write_dump(d, frame, packed=False, half=half)
    files = sorted(f for f in os.listdir(d) if f.endswith(".bin"))
    assert files == sorted(["depth.bin", "direct.f16.bin", "aov_velocity.bin"] + ["aov_%s.f16.bin" % k for k in half if k != "direct"])
    assert os.path.getsize(os.path.join(d, "direct.f16.bin")) == W * H * 3 * 2 and os.path.getsize(os.path.join(d, "aov_diffuse.f16.bin")) == W * H * 4 * 2
    r = dump.read_dump(d)
    got = dict(r.aov, depth=r.depth, direct=r.direct)
    assert r.gbuffer is None and r.velocity is None and r.direct.shape == (H, W, 3)
    for k in NAMES:
        want = (p[k][..., :3] if k == "direct" else p[k])
        want = want.astype(np.float16) if k in half else want
        assert got[k].dtype == want.dtype and got[k].shape == want.shape and got[k].tobytes() == want.tobytes(), k
    # an all-float dump reads as before
    d2 = str(tmp_path / "plain")
    frame.direct = p["direct"]
    dump.write_dump(d2, frame, packed=False)
    r2 = dump.read_dump(d2)
    assert not [f for f in os.listdir(d2) if ".f16." in f] and all(v.dtype == np.float32 for v in r2.aov.values()) and r2.direct.shape == (H, W, 4)
    with pytest.raises(ValueError):
        dump.write_dump(str(tmp_path / "bad"), frame, packed=False, half=("depth",))
    if node is None:
        return
    res = json.loads(subprocess.check_output([node, "-e", _NODE_DUMP, JS, d], text=True).strip().splitlines()[-1])
    for k in NAMES:
        assert res[k][0] == ("Uint16Array" if k in half else "Float32Array") and res[k][1] == got[k].size, k
        assert res[k][2] == hashlib.sha1(got[k].tobytes()).hexdigest(), k


@needs_hostsim
def test_gpu_file_on_the_host_simulator():
    """tests/test_gpu_stage_aov.py with the host simulator's library in place of the device's: the entry point's state handling, the plan, the
    kernel's indexing (groups, tails, segments of a row tile) and the Python host, executed here"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    env = {k: v for k, v in os.environ.items() if k not in ("RFX_HOSTSIM", "RFX_TEST_LIB")}
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--hostsim", "-p", "no:cacheprovider", os.path.join(HERE, "test_gpu_stage_aov.py")],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert " passed" in p.stdout and "skipped" not in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]
