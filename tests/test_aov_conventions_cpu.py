"""CPU (-m "not gpu") side of rfx.h "AOV conventions": the header against the ctypes mirror, the host conversion against the restatement, the
restatement against the float64 scene it was rounded from, the plan under every kind, and a run of tests/test_gpu_aov_conventions.py on the
host simulator."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_convention_cases as CC
import aov_convention_ref as R
from launch_plans import needs_hostsim
from rfx_amd import abi, conventions, imageio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = abi.AOV_PLANES


def test_header_and_ctypes_mirror_agree(tmp_path):
    fields = [n for n, _ in abi.AovConventions._fields_]
    c = tmp_path / "conv.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rfx.h"\nint main(){size_t v[] = {sizeof(rfx_aov_conventions), %s, '
                 "RFX_AOV_DEPTH_FRAGCOORD, RFX_AOV_DEPTH_VIEW_Z, RFX_AOV_DEPTH_POSITION, RFX_AOV_VELOCITY_UV, RFX_AOV_VELOCITY_SCALED, RFX_AOV_VELOCITY_CAMERAS, "
                 "RFX_AOV_NORMAL_WORLD, RFX_AOV_NORMAL_VIEW, (size_t)RFX_ABI_VERSION};\n"
                 'for (unsigned i = 0; i < sizeof v / sizeof v[0]; i++) printf("%%zu ", v[i]);\nreturn 0;}\n' % ", ".join("offsetof(rfx_aov_conventions, %s)" % n for n in fields))
    exe = tmp_path / "conv"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.AovConventions)] + [getattr(abi.AovConventions, n).offset for n in fields] + [0, 1, 2, 0, 1, 2, 0, 1, 21]
    assert "rfx_set_aov_conventions" in abi.EXPORTS and hasattr(abi.load_library(), "rfx_set_aov_conventions")  # no skip on a missing symbol


def test_both_products_of_the_velocity_matrix_agree():
    """conventions.multiply_matrices (what the hosts hand the library) == the cases' restatement of three's multiplyMatrices in float64"""
    for frame in range(5):
        for perspective in (True, False):
            cam = CC.camera(frame, perspective)
            got, want = conventions.multiply_matrices(cam["P"], cam["V"]), CC.three_product(cam["P"], cam["V"])
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    conv = CC.setting(2, 2, 1)
    back = conventions.AovConventions.from_json(CC.host(conv).to_json())
    assert bytes(back.to_abi()) == bytes(CC.host(conv).to_abi())  # the record a dump directory carries loses nothing


@pytest.mark.parametrize("dk,vk,ns", CC.COMBINATIONS)
def test_host_conversion_equals_the_restatement(dk, vk, ns):
    """1. imageio.aov_to_reference_conventions == tests/aov_convention_ref.py bit for bit (NaN payloads aside: numpy's own on both sides), on
    whole frames and on a band of one, both cameras, the coverage edges included"""
    for perspective in (True, False):
        conv = CC.setting(dk, vk, ns, perspective)
        for W, H, r0, n in ((37, 5, 0, 5), (16, 9, 3, 4)):
            frame = CC.stage(CC.engine_frame(W, H, conv, 0x600 + W), "typed")
            band = {k: v[r0:r0 + n] for k, v in frame.items()}
            want = R.convert(band, conv, W, H, r0)
            key = CC.DEPTH_KINDS[dk] if dk else "depth"
            got = imageio.aov_to_reference_conventions(dict({k: v for k, v in band.items() if k != "depth"}, **{key: band["depth"]}), CC.host(conv), r0, H)
            for k in ("depth", "velocity", "normal"):
                a, b = np.ascontiguousarray(got[k], np.float32), np.ascontiguousarray(want[k], np.float32)
                assert a.shape == b.shape, k
                same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
                assert same.all(), (k, perspective, W, int((~same).sum()))


# 2. Measured here, on the CPU, from the restatement (the reference) on this test's frames, times 2.  The position's own float32 rounding
# dominates both figures — half an ulp of a coordinate of magnitude ~8 is 4.8e-7 world units; the view Z the depth is made of inherits it — and
# scales with the scene's extent, hence the margin.  Measured max |delta|: perspective, depth 1.70e-7 (POSITION) / 9.12e-8 (VIEW_Z), velocity
# 1.70e-7 (CAMERAS) / 1.22e-9 (SCALED); orthographic, depth 7.70e-8 / 5.82e-8, velocity 9.99e-8 / 6.11e-10.  profiles/import/README.md
# carries the same numbers.
DEPTH_BOUND = {"perspective": 2 * 1.70e-7, "orthographic": 2 * 7.70e-8}
VELOCITY_BOUND = {"perspective": 2 * 1.70e-7, "orthographic": 2 * 9.99e-8}


@pytest.mark.parametrize("camera", ["perspective", "orthographic"])
def test_restatement_on_engine_planes_against_the_float64_scene(camera):
    """2. scene.py's engine planes (96 x 54, frame 3: the camera moved) through the restatement, against the float64 depth / velocity the same
    render call rounded them from.  POSITION and VIEW_Z depth, CAMERAS velocity from either, SCALED velocity from the pixel motion.
    Coverage differs only where the float64 z lies within 2^-22 of 1.0.
    Measured max |delta| (restatement, float32, against float64), this scene: depth 1.70e-7 (perspective) / 7.70e-8 (orthographic), velocity
    1.70e-7 / 9.99e-8; no texel's coverage differs.  The bounds asserted are twice that (DEPTH_BOUND, VELOCITY_BOUND above)."""
    from rfx_amd.scene import AnalyticScene
    W, H = 96, 54
    f = AnalyticScene(1234).render(W, H, 3, aov=True, engine=True, ortho_half_height=None if camera == "perspective" else 4.0)
    e = f.engine
    assert e["hit"].any() and not e["hit"].all()
    base = dict(background_position=(0.0, 0.0, 0.0), velocity_scale=(1.0 / W, -1.0 / H))
    worst_d, worst_v = 0.0, 0.0
    for dk, plane in (("position", e["position"]), ("view_z", e["view_z"])):
        for vk in ("cameras", "scaled"):
            conv = conventions.AovConventions.from_cameras(f.camera, f.prev_camera, depth_kind=dk, velocity_kind=vk, normal_space="view", **base)
            ref = dict(depth_kind=conventions.DEPTH_KINDS[dk], velocity_kind=conventions.VELOCITY_KINDS[vk], normal_space=1, perspective=conv.perspective,
                       scale=conv.velocity_scale, near=conv.near, far=conv.far, background=conv.background_position, VM=conv.velocityMatrix,
                       PVM=conv.prevVelocityMatrix, P=conv.projectionMatrix, Pi=conv.projectionMatrixInverse, C=conv.cameraMatrixWorld)
            planes = dict(depth=plane, normal=e["view_normal"])
            if vk == "scaled":
                planes["velocity"] = e["motion"]
            out = R.convert(planes, ref, W, H)
            covered = out["depth"] < 1.0
            differs = covered != e["hit"]
            assert (np.abs(e["depth64"][differs] - 1.0) <= 2.0 ** -22).all(), (dk, int(differs.sum()))
            both = covered & e["hit"]
            dd = float(np.abs(out["depth"][both].astype(np.float64) - e["depth64"][both]).max())
            dv = float(np.abs(out["velocity"][both].astype(np.float64) - e["velocity64"][both]).max())
            print("%s %s %s: max |ddepth| %.3g  max |dvel| %.3g  coverage differs at %d texels" % (camera, dk, vk, dd, dv, int(differs.sum())))
            worst_d, worst_v = max(worst_d, dd), max(worst_v, dv)
            # the world normals the scene drew, from the camera-space ones: rounding of a rotation
            assert np.abs(out["normal"][both] - f.aov["normal"][both]).max() < 1e-6
    assert worst_d <= DEPTH_BOUND[camera] and worst_v <= VELOCITY_BOUND[camera], (worst_d, worst_v)
    assert f.engine is not None and AnalyticScene(1234).render(W, H, 3, aov=True).engine is None  # every existing output: as before


_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
I, U = ctypes.c_int, ctypes.c_ulonglong
class Seg(ctypes.Structure):
    _fields_ = [(n, I) for n in ("row0", "rows", "full", "pixels", "groups", "blocks", "tail_start", "tail_pixels")] + [("offset", U * 8)]
class Plan(ctypes.Structure):
    _fields_ = [("nseg", I), ("seg", Seg * 3), ("plane_row0", I * 8), ("plane_rows", I * 8), ("elem_bytes", I * 8), ("write_gbuffer", I), ("write_velocity", I),
                ("write_direct", I), ("copy_bytes", U), ("stage_bytes", U)]
P = ctypes.POINTER
lib.rfx_internal_aov_plan_conv.argtypes = [I, I, I, I, P(I), P(I), I, I, I, I, P(Plan)]
lib.rfx_internal_aov_plan.argtypes = [I, I, I, I, P(I), P(I), I, I, P(Plan)]
out = []
for W, H, h0, hn, types, chans, r0, n, dk, vk in json.load(sys.stdin):
    t = Plan()
    rc = lib.rfx_internal_aov_plan_conv(W, H, h0, hn, (I * 8)(*types), (I * 8)(*chans), r0, n, dk, vk, ctypes.byref(t))
    d = dict(rc=rc)
    if rc == 0:
        d.update({k: getattr(t, k) for k in ("nseg", "write_gbuffer", "write_velocity", "write_direct", "copy_bytes", "stage_bytes")})
        d["seg_pixels"] = [(s.full, s.pixels) for s in t.seg[:t.nseg]]
    if dk == 0 and vk == 0:
        u = Plan()
        d["same_as_default"] = lib.rfx_internal_aov_plan(W, H, h0, hn, (I * 8)(*types), (I * 8)(*chans), r0, n, ctypes.byref(u)) == rc and (rc != 0 or bytes(u) == bytes(t))
    out.append(d)
json.dump(out, sys.stdout)
"""


@needs_hostsim
def test_plan_under_every_kind():
    """3. rfx_launch.h rfx_aov_plan_conv_for as the library computes it: the copy and staging bytes for every kind combination — the position
    plane counts three channels, CAMERAS writes VELOCITY without a velocity plane — and the refusals; kinds (0, 0) give rfx_aov_plan_for's plan."""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    from conftest import hostsim_child_env
    env = dict(os.environ, **hostsim_child_env(sim))
    W, H, h0, hn = 37, 12, 3, 6   # the slots but DEPTH hold rows [3, 9)
    full = dict(diffuse=4, normal=3, roughness=1, metalness=1, emissive=3, velocity=2, depth=1, direct=3)
    typed = {k: (0 if k in ("velocity", "depth") else 1) for k in NAMES}
    cases, expect = [], []
    for dk in range(3):
        for vk in range(3):
            for ty in ({}, typed, {k: 1 for k in NAMES}):
                ch = dict(full, depth=3 if dk == 2 else 1)
                if vk == 2:
                    del ch["velocity"]
                cases.append((ch, ty, dk, vk))
                elem = lambda k: 2 if ty.get(k, 0) else 4  # noqa: E731
                inner = sum(ch[k] * elem(k) for k in ch if k != "depth") * W * hn
                expect.append(dict(rc=0, copy_bytes=inner + ch["depth"] * elem("depth") * W * H, write_velocity=1, write_gbuffer=1, write_direct=1, nseg=3))
    refusals = [(dict(full, depth=3), {}, 0, 0), (dict(full, depth=3), {}, 1, 0), (full, {}, 2, 0), (full, {}, 0, 2), (dict(full, depth=2), {}, 2, 2),
                (full, {}, 3, 0), (full, {}, 0, 3), (full, {}, -1, 0), (dict(depth=1, velocity=2), {}, 0, 1)]
    # CAMERAS: VELOCITY is written iff normal is given
    extra = [(dict(depth=3, normal=3), {}, 2, 2), (dict(depth=1), {}, 1, 2), (dict(depth=3, direct=4), {}, 2, 2)]
    rows = [[W, H, h0, hn, [ty.get(k, 0) for k in NAMES], [ch.get(k, 0) for k in NAMES], 0, H, dk, vk] for ch, ty, dk, vk in cases + refusals + extra]
    p = subprocess.run([sys.executable, "-c", _CHILD, env["RFX_TEST_LIB"]], input=json.dumps(rows), capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    plans = json.loads(p.stdout)
    for (ch, ty, dk, vk), want, got in zip(cases, expect, plans):
        assert {k: got.get(k) for k in want} == want, (dk, vk, ty, got)
        assert got["stage_bytes"] >= got["copy_bytes"] and got["stage_bytes"] <= 84 * W * H + 256 * 3 * 8  # at most 84 bytes per band pixel
        assert got["seg_pixels"] == [[0, 3 * W], [1, 6 * W], [0, 3 * W]]
        if dk == 0 and vk == 0:
            assert got["same_as_default"]
    for got in plans[len(cases):len(cases) + len(refusals)]:
        assert got["rc"] == abi.RFX_EINVAL, got
    a, b, c = plans[len(cases) + len(refusals):]
    assert (a["rc"], a["write_velocity"], a["write_gbuffer"]) == (0, 1, 0) and a["copy_bytes"] == 12 * W * H + 12 * W * hn
    assert (b["rc"], b["write_velocity"], b["nseg"]) == (0, 0, 1) and b["copy_bytes"] == 4 * W * H
    assert (c["rc"], c["write_velocity"], c["write_direct"]) == (0, 0, 1)
    # the largest frame: a float position and every other plane float
    assert max(g["copy_bytes"] for g in plans[:len(cases)]) <= 84 * W * H


def test_layout_names_for_engine_planes(tmp_path):
    """names= maps `position` (default channels position.X/.Y/.Z) and `view_z`; AOV_LAYOUT is unchanged"""
    assert list(imageio.AOV_LAYOUT) == list(NAMES) and imageio.AOV_LAYOUT["depth"] == ("depth.Z",)
    W, H = 9, 5
    conv = CC.setting(2, 2, 0)
    frame = CC.stage(CC.engine_frame(W, H, conv, 9), "f32")
    ch = {}
    for k, v in frame.items():
        names = ("P.X", "P.Y", "P.Z") if k == "depth" else imageio.AOV_LAYOUT[k]
        v3 = v.reshape(H, W, -1)
        for j in range(v3.shape[2]):
            ch[names[j]] = v3[..., j]
    path = str(tmp_path / "p.exr")
    imageio.write_exr(path, ch, "zip")
    names = {"position": ("P.X", "P.Y", "P.Z")}
    lay = imageio.exr_aov_layout(path, names)
    assert lay.planes["depth"] == (3, "float") and "velocity" not in lay.planes
    t = imageio.exr_to_typed_planes(path, dict(names, velocity=()))
    assert t["depth"].shape == (H, W, 3) and np.array_equal(t["depth"], frame["depth"], equal_nan=True)
    with pytest.raises(ValueError):
        imageio.exr_aov_layout(path, {"position": None, "view_z": None})
    assert "depth" not in imageio.exr_aov_layout(path, {"position": None}).planes  # position.X is not in this file: no depth plane, the library refuses


@needs_hostsim
def test_gpu_file_on_the_host_simulator():
    """4. tests/test_gpu_aov_conventions.py with the host simulator's library in place of the device's"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    env = {k: v for k, v in os.environ.items() if k not in ("RFX_HOSTSIM", "RFX_TEST_LIB")}
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--hostsim", "-p", "no:cacheprovider", os.path.join(HERE, "test_gpu_aov_conventions.py")],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert " passed" in p.stdout and "skipped" not in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]


def test_exr_to_dump_with_conventions(tmp_path):
    """tools/exr_to_dump.py --conventions: an engine-form EXR (P.X/P.Y/P.Z, camera-space normals, no velocity layer) + side-car cameras -> a
    reference-form dump directory whose planes are the host conversion's"""
    import types

    from rfx_amd import dump
    from rfx_amd.scene import AnalyticScene
    W, H = 48, 27
    f = AnalyticScene(1234).render(W, H, 2, aov=True, engine=True)
    ch = {}
    for key, names in imageio.AOV_LAYOUT.items():
        if key in ("velocity", "depth"):
            continue
        a = f.direct if key == "direct" else (f.engine["view_normal"] if key == "normal" else f.aov[key])
        a = a[..., None] if a.ndim == 2 else a
        for i, n in enumerate(names):
            ch[n] = a[..., i]
    for i, n in enumerate(("P.X", "P.Y", "P.Z")):
        ch[n] = f.engine["position"][..., i]
    path = str(tmp_path / "engine.exr")
    imageio.write_exr(path, ch, "zip")
    dump.write_exr_dump(str(tmp_path / "side.exr"), types.SimpleNamespace(width=W, height=H, camera=f.camera, prev_camera=f.prev_camera, depth=f.depth, direct=f.direct, aov=f.aov))
    os.replace(str(tmp_path / "side.exr.json"), path + ".json")
    kinds = dict(depth_kind="position", velocity_kind="cameras", normal_space="view", background_position=[0, 0, 0])
    out = str(tmp_path / "dump")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "exr_to_dump.py"), path, out, "--map", "position=P.X,P.Y,P.Z", "--map", "velocity=",
                           "--conventions", json.dumps(kinds)], stdout=subprocess.DEVNULL)
    got = dump.read_dump(out)
    conv = conventions.AovConventions.from_cameras(f.camera, f.prev_camera, **dict(kinds, background_position=(0.0, 0.0, 0.0)))
    want = imageio.aov_to_reference_conventions(dict(position=f.engine["position"], normal=f.engine["view_normal"]), conv)
    assert got.conventions is None and got.depth.tobytes() == want["depth"].tobytes()
    assert got.aov["velocity"].tobytes() == want["velocity"].tobytes() and got.aov["normal"].tobytes() == want["normal"].tobytes()
    # ... which are the scene's own reference-form planes up to the float32 position's rounding (bounds: the test above)
    hit = f.engine["hit"] & (got.depth < 1.0)
    assert np.abs(got.depth[hit] - f.depth[hit]).max() <= DEPTH_BOUND["perspective"] + 2.0 ** -24
    assert np.abs(got.aov["velocity"][hit] - f.aov["velocity"][hit]).max() <= VELOCITY_BOUND["perspective"] + 2.0 ** -24
