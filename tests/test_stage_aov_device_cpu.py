"""CPU (-m "not gpu") side of the device planes (include/rfx.h rfx_stage_aov_device): the header against the ctypes mirror, the launch plan as
the library computes it (rfx_launch.h rfx_aov_device_plan_for, through the host simulator's build) against a restatement over seeded random
strides, alignments, bands and held rows, the plan's refusals, the test layouts themselves, the tensor-to-plane function on CPU tensors, and a
run of tests/test_gpu_stage_aov_device.py on the host simulator, so that the entry point and the strided kernel's indexing are exercised where
there is no device."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_device_cases as D
from launch_plans import needs_hostsim
from rfx_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = abi.AOV_PLANES
FULL = dict(diffuse=4, normal=3, roughness=1, metalness=1, emissive=3, velocity=2, depth=1, direct=4)
NONE, INTERLEAVED, PLANAR, ELEMENT = 0, 1, 2, 3


def test_header_and_ctypes_mirror_agree(tmp_path):
    plane_fields = ("data", "type", "channels", "stride_x", "stride_y", "stride_c")
    exprs = ["sizeof(rfx_device_plane)"] + ["offsetof(rfx_device_plane, %s)" % n for n in plane_fields] + ["sizeof(rfx_aov_device_frame)"] + [
        "offsetof(rfx_aov_device_frame, %s)" % n for n in NAMES] + ["(size_t)RFX_ABI_VERSION"]
    c = tmp_path / "dev.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rfx.h"\nint (*entry)(rfx_ctx *, const rfx_aov_device_frame *, int, int, void *) = rfx_stage_aov_device;\n'
                 'int main(){size_t v[] = {%s};\nfor (unsigned i = 0; i < sizeof v / sizeof v[0]; i++) printf("%%zu ", v[i]);\nreturn 0;}\n' % ", ".join(exprs))
    obj = tmp_path / "dev.o"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(obj)])  # (the prototype, type-checked)
    c.write_text(c.read_text().replace("int (*entry)(rfx_ctx *, const rfx_aov_device_frame *, int, int, void *) = rfx_stage_aov_device;\n", ""))
    exe = tmp_path / "dev"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(abi.DevicePlane)] + [getattr(abi.DevicePlane, n).offset for n in plane_fields] + [C.sizeof(abi.AovDeviceFrame)] + [
        getattr(abi.AovDeviceFrame, n).offset for n in NAMES] + [abi.RFX_ABI_VERSION]
    assert got == want
    assert C.sizeof(abi.DevicePlane) == 40 and C.sizeof(abi.AovDeviceFrame) == 8 * 40 and abi.RFX_ABI_VERSION == 21  # additive: no version bump
    lib = abi.load_library()
    assert "rfx_stage_aov_device" in abi.EXPORTS and hasattr(lib, "rfx_stage_aov_device")
    from rfx_amd.context import Context
    assert isinstance(Context.has_stage_aov_device, property)


_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
I, U, L = ctypes.c_int, ctypes.c_ulonglong, ctypes.c_longlong
class Seg(ctypes.Structure):
    _fields_ = [(n, I) for n in ("row0", "rows", "full", "pixels", "groups", "blocks", "tail_start", "tail_pixels")] + [("offset", U * 8)]
class Rows(ctypes.Structure):
    _fields_ = [("nseg", I), ("seg", Seg * 3), ("plane_row0", I * 8), ("plane_rows", I * 8), ("elem_bytes", I * 8), ("write_gbuffer", I), ("write_velocity", I),
                ("write_direct", I), ("copy_bytes", U), ("stage_bytes", U)]
class Plan(ctypes.Structure):
    _fields_ = [("rows", Rows), ("layout", I * 8), ("flat", I * 3), ("groups_x", I), ("tail_x", I), ("tail_pixels", I), ("lanes_x", I), ("grid_x", I), ("grid_y", I * 3),
                ("seg_offset", (L * 8) * 3)]
lib.rfx_internal_aov_device_plan.argtypes = [I, I, I, I, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(U), ctypes.POINTER(L), ctypes.POINTER(L), ctypes.POINTER(L), I, I, I, I,
                                             ctypes.POINTER(Plan)]
out = []
for W, H, h0, hn, types, chans, addr, sx, sy, sc, r0, n, dk, vk in json.load(sys.stdin):
    t = Plan()
    rc = lib.rfx_internal_aov_device_plan(W, H, h0, hn, (I * 8)(*types), (I * 8)(*chans), (U * 8)(*addr), (L * 8)(*sx), (L * 8)(*sy), (L * 8)(*sc), r0, n, dk, vk, ctypes.byref(t))
    d = dict(rc=rc)
    if rc == 0:
        d.update(layout=list(t.layout), flat=list(t.flat)[:t.rows.nseg], groups_x=t.groups_x, tail_x=t.tail_x, tail_pixels=t.tail_pixels, lanes_x=t.lanes_x, grid_x=t.grid_x,
                 grid_y=list(t.grid_y)[:t.rows.nseg], write=[t.rows.write_gbuffer, t.rows.write_velocity, t.rows.write_direct],
                 seg=[dict(row0=s.row0, rows=s.rows, full=s.full, reads=[o != 2 ** 64 - 1 for o in s.offset], offset=list(t.seg_offset[k])) for k, s in enumerate(t.rows.seg[:t.rows.nseg])])
    out.append(d)
json.dump(out, sys.stdout)
"""


def device_plans(cases):
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    from conftest import hostsim_child_env
    env = dict(os.environ, **hostsim_child_env(sim))
    p = subprocess.run([sys.executable, "-c", _CHILD, env["RFX_TEST_LIB"]], input=json.dumps(cases), capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout)


def restated(W, H, h0, hn, types, chans, addr, sx, sy, sc, r0, n, dk, vk):
    """The contract of include/rfx.h "device planes" and rfx_launch.h restated in Python integers (no overflow to mind).  None: refused."""
    want = [4, 3, 1, 1, 3, 2, 3 if dk == 2 else 1, 4]
    given = [c != 0 for c in chans]
    for i in range(8):
        if not given[i]:
            continue
        if types[i] not in (0, 1) or (chans[i] != want[i] and not (i in (0, 7) and chans[i] == 3)):
            return None
    if not given[6] or (vk == 2 and given[5]):
        return None
    g = sum(given[i] for i in (0, 2, 3, 4))
    gbuffer = g == 4 and given[1]
    velocity = given[1] if vk == 2 else given[5]
    if (velocity and not given[1]) or (not gbuffer and (g or (given[1] and not velocity))):
        return None
    if n <= 0 or r0 < 0 or r0 + n > H:
        return None
    elem = [0 if not given[i] else 2 if types[i] else 4 for i in range(8)]
    layout = [NONE] * 8
    for i in range(8):
        if not given[i]:
            continue
        ch = chans[i]
        if addr[i] % elem[i]:
            return None
        span = 1 + abs(sx[i]) * (W - 1) + abs(sy[i]) * (n - 1) + (abs(sc[i]) * (ch - 1) if ch > 1 else 0)
        if span * elem[i] > 2 ** 62 - 1:
            return None
        c1 = ch == 1 or sc[i] == 1
        aligned = addr[i] % (4 * elem[i]) == 0 and sy[i] % 4 == 0
        if c1 and sx[i] == ch:
            layout[i] = INTERLEAVED if aligned else ELEMENT
        elif sx[i] == 1:
            layout[i] = PLANAR if aligned and (ch == 1 or sc[i] % 4 == 0) else ELEMENT
        else:
            layout[i] = ELEMENT
    direct = given[7]
    a, b = max(r0, h0), min(r0 + n, h0 + hn)
    if not (gbuffer or velocity or direct) or b <= a:
        a = b = r0 + n
    segs = []
    for k, (lo, hi) in enumerate(((r0, a), (a, b), (b, r0 + n))):
        if hi <= lo:
            continue
        full = k == 1
        reads = [given[i] and (i == 6 or full) for i in range(8)]
        off = [(lo - r0) * sy[i] if reads[i] else 0 for i in range(8)]
        flat = all((chans[i] == 1 or sc[i] == 1) and sx[i] == chans[i] and sy[i] == W * chans[i] and (addr[i] + off[i] * elem[i]) % 16 == 0 for i in range(8) if reads[i])
        segs.append(dict(row0=lo, rows=hi - lo, full=int(full), reads=reads, offset=off, flat=int(flat), grid_y=-(-(hi - lo) // 4)))
    lanes = W // 4 + (1 if W % 4 else 0)
    return dict(layout=layout, segs=segs, groups_x=W // 4, tail_x=W // 4 * 4, tail_pixels=W % 4, lanes_x=lanes, grid_x=-(-lanes // 64), write=[int(gbuffer), int(velocity), int(direct)])


def random_cases(n=400, seed=0xdeb1ce):
    rng = np.random.RandomState(seed)
    out = []
    subsets = [NAMES, ("depth",), ("depth", "direct"), ("depth", "velocity", "normal"), tuple(k for k in NAMES if k != "direct"), tuple(k for k in NAMES if k != "velocity"),
               ("depth", "normal"), ("depth", "diffuse", "normal"), ("normal", "velocity")]  # (refused, but for depth + normal under CAMERAS)
    for _ in range(n):
        W, H = int(rng.randint(1, 140)), int(rng.randint(1, 60))
        y0 = int(rng.randint(0, H))
        hn = int(rng.randint(1, H - y0 + 1))
        r0 = int(rng.randint(0, H))
        rows = int(rng.randint(1, H - r0 + 1))
        dk, vk = int(rng.randint(3)), int(rng.randint(3))
        subset = subsets[int(rng.randint(len(subsets)))]
        if vk == 2:
            subset = tuple(k for k in subset if k != "velocity")
        types, chans, addr, sx, sy, sc = [], [], [], [], [], []
        for k in NAMES:
            ch = FULL[k] if k in subset else 0
            if k in ("diffuse", "direct") and ch and rng.randint(2):
                ch = 3
            if k == "depth" and dk == 2:
                ch = 3
            ty = int(rng.randint(2))
            e = 2 if ty else 4
            form = int(rng.randint(6))
            pitch = int(rng.choice([0, 1, 4, 5, 8]))
            if form == 0:    # tight
                s = (ch, W * ch, 1)
            elif form == 1:  # interleaved, pitched
                s = (ch, W * ch + pitch, 1)
            elif form == 2:  # planar, pitched rows and planes
                s = (1, W + pitch, (W + pitch) * rows + int(rng.choice([0, 2, 4])))
            elif form == 3:  # top-down
                s = (ch, -(W * ch + pitch), 1)
            elif form == 4:  # mirrored, broadcast
                s = [(-ch, W * ch, 1), (0, 0, 0), (1, 0, W)][int(rng.randint(3))]
            else:            # anything
                s = tuple(int(v) for v in rng.randint(-9, 10, 3))
            types.append(ty)
            chans.append(ch)
            addr.append(0x7f0000000000 + 256 * int(rng.randint(1 << 20)) + e * int(rng.choice([0, 0, 1, 2, 4, 8])))
            sx.append(s[0]); sy.append(s[1]); sc.append(s[2])
        out.append([W, H, y0, hn, types, chans, addr, sx, sy, sc, r0, rows, dk, vk])
    return out


@needs_hostsim
def test_device_plan_against_the_restatement():
    cases = random_cases()
    # a tight, aligned frame on a row tile: every segment flat; the same with a depth plane two rows of odd width in: misaligned segments
    tight = lambda W, ch: (ch, W * ch, 1)  # noqa: E731
    for W, base in ((96, 0), (97, 0), (97, 4)):
        s = [tight(W, FULL[k]) for k in NAMES]
        cases.append([W, 54, 16, 26, [0] * 8, [FULL[k] for k in NAMES], [0x7f0000001000 + base] * 8, [v[0] for v in s], [v[1] for v in s], [v[2] for v in s], 0, 54, 0, 0])
    plans = device_plans(cases)
    seen_layouts, seen_flat, refused = set(), set(), 0
    for case, t in zip(cases, plans):
        want = restated(*case)
        if want is None:
            assert t["rc"] == abi.RFX_EINVAL, case
            refused += 1
            continue
        assert t["rc"] == 0, case
        assert t["layout"] == want["layout"], (case, t["layout"], want["layout"])
        for k in ("groups_x", "tail_x", "tail_pixels", "lanes_x", "grid_x", "write"):
            assert t[k] == want[k], (case, k)
        assert len(t["seg"]) == len(want["segs"])
        for j, (s, w) in enumerate(zip(t["seg"], want["segs"])):
            assert (s["row0"], s["rows"], s["full"], s["reads"]) == (w["row0"], w["rows"], w["full"], w["reads"]), (case, j)
            assert [o for o, r in zip(s["offset"], s["reads"]) if r] == [o for o, r in zip(w["offset"], w["reads"]) if r], (case, j)
            assert t["flat"][j] == w["flat"] and t["grid_y"][j] == w["grid_y"], (case, j)
            seen_flat.add(w["flat"])
        seen_layouts |= set(want["layout"])
    assert seen_layouts == {NONE, INTERLEAVED, PLANAR, ELEMENT} and seen_flat == {0, 1} and 10 < refused < len(cases) - 100
    assert plans[-3]["flat"] == [1, 1, 1] and plans[-3]["layout"] == [INTERLEAVED] * 8
    assert plans[-2]["flat"] == [1, 1, 0]  # 97 wide: row 16 starts a multiple of 16 bytes in, row 42 of the depth plane (42 x 97 x 4 bytes) does not
    assert plans[-1]["layout"] == [ELEMENT] * 8 and plans[-1]["flat"] == [0, 0, 0]


@needs_hostsim
def test_device_plan_refusals():
    """what rfx_stage_aov_device answers RFX_EINVAL to on top of rfx_stage_aov's cases: alignment to the element size, extents beyond 62 bits"""
    W, H = 5, 4
    ch = [FULL[k] for k in NAMES]
    tight = [(c, W * c, 1) for c in ch]
    ok = [W, H, 0, H, [0, 1, 0, 1, 0, 0, 0, 1], ch, [0x7f0000001000] * 8, [s[0] for s in tight], [s[1] for s in tight], [s[2] for s in tight], 0, H, 0, 0]

    def change(**kw):
        case = json.loads(json.dumps(ok))
        for k, (i, v) in kw.items():
            case[dict(types=4, chans=5, addr=6, sx=7, sy=8, sc=9)[k]][i] = v
        return case
    lim = 2 ** 62 - 1
    accepted = [ok, change(addr=(1, 0x7f0000001002)), change(addr=(0, 0x7f0000001004)),  # halves at 2 bytes, floats at 4
                change(sy=(6, (lim // 4 - 1 - 4 * 1) // 3)),      # depth (float, C 1): 1 + 4 sx + 3 sy elements of 4 bytes, just inside
                change(sx=(6, 0), sy=(6, -((lim // 4 - 1) // 3))),
                change(sc=(1, -((lim // 2 - 1 - 4 * 3 - 3 * 15) // 2)))]  # normal (half, C 3)
    refused = [change(addr=(0, 0x7f0000001002)), change(addr=(1, 0x7f0000001001)), change(addr=(6, 0x7f0000001003)),
               change(sy=(6, (lim // 4 - 1 - 4 * 1) // 3 + 1)), change(sx=(6, 0), sy=(6, -((lim // 4 - 1) // 3) - 1)),
               change(sc=(1, -((lim // 2 - 1 - 4 * 3 - 3 * 15) // 2) - 1)),
               change(sy=(6, 2 ** 62)), change(sx=(6, -2 ** 63)), change(sy=(6, 2 ** 63 - 1)), change(sc=(0, 2 ** 61)), change(sx=(7, 2 ** 58), sy=(7, -2 ** 59)),
               change(types=(6, 2)), change(chans=(6, 0)), change(chans=(1, 4)), change(chans=(2, 0))]
    for case in accepted:
        assert restated(*case) is not None, case
    for case in refused:
        assert restated(*case) is None, case
    assert [t["rc"] for t in device_plans(accepted)] == [0] * len(accepted)
    assert [t["rc"] for t in device_plans(refused)] == [abi.RFX_EINVAL] * len(refused)


def test_layouts_address_their_values():
    """the helper's own premise: every layout of aov_device_cases addresses exactly the values it was given"""
    rng = np.random.RandomState(4)
    for W, H in D.SIZES:
        for C_ in (1, 2, 3, 4):
            for dt in (np.float32, np.float16):
                v = rng.rand(H, W, C_).astype(dt) if C_ > 1 else rng.rand(H, W).astype(dt)
                for layout in [la for la in D.LAYOUTS if la != "broadcast"] + ["planar_top", "planar_pitch_top", "pitch4_top"]:
                    flat, off, sx, sy, sc = D.lay(v, layout)
                    p = abi.DevicePlane(0, abi.PLANE_TYPES[v.dtype], C_, sx, sy, sc)  # (the record keeps signed 64-bit strides)
                    assert np.array_equal(D.gather(flat, off, p.stride_x, p.stride_y, p.stride_c, H, W, p.channels), v.reshape(H, W, C_)), (layout, W, H, C_)
    one = np.full((3, 5), 0.375, np.float16)
    assert np.array_equal(D.gather(*D.lay(one, "one"), 3, 5, 1)[..., 0], one)


def test_tensor_to_plane_on_cpu_tensors():
    """context.device_plane: permuted, expanded, sliced with pitch, origin="top" — every plane addresses the tensor's own values"""
    import torch
    from rfx_amd.context import device_plane

    def read(p, rows, W):
        """the (rows, W, C) values the plane addresses, through its own pointer arithmetic"""
        dt, e = (np.float16, 2) if p.type == abi.PLANE_F16 else (np.float32, 4)
        out = np.empty((rows, W, p.channels), dt)
        for y in range(rows):
            for x in range(W):
                for c in range(p.channels):
                    out[y, x, c] = np.frombuffer((C.c_char * e).from_address(p.data + e * (x * p.stride_x + y * p.stride_y + c * p.stride_c)), dt)[0]
        return out

    H, W = 5, 7
    rng = np.random.RandomState(8)
    chw = torch.from_numpy(rng.rand(3, H, W).astype(np.float32))
    p = device_plane(chw.permute(1, 2, 0), H, W)
    assert (p.type, p.channels, p.stride_x, p.stride_y, p.stride_c, p.data) == (abi.PLANE_F32, 3, 1, W, H * W, chw.data_ptr())
    assert np.array_equal(read(p, H, W), chw.permute(1, 2, 0).numpy())
    top = device_plane(chw.permute(1, 2, 0), H, W, origin="top")
    assert (top.stride_x, top.stride_y, top.stride_c, top.data) == (1, -W, H * W, chw.data_ptr() + 4 * (H - 1) * W)
    assert np.array_equal(read(top, H, W), chw.permute(1, 2, 0).numpy()[::-1])
    const = torch.tensor([[0.375]], dtype=torch.float16).expand(H, W)
    q = device_plane(const, H, W)
    assert (q.type, q.channels, q.stride_x, q.stride_y, q.data) == (abi.PLANE_F16, 1, 0, 0, const.data_ptr()) and (read(q, H, W) == np.float16(0.375)).all()
    assert device_plane(const, H, W, origin="top").data == const.data_ptr()
    wide = torch.from_numpy(rng.rand(H + 2, W + 3, 4).astype(np.float16))
    cut = wide[1:H + 1, 2:W + 2]
    r = device_plane(cut, H, W)
    assert (r.channels, r.stride_x, r.stride_y, r.stride_c, r.data) == (4, 4, 4 * (W + 3), 1, wide.data_ptr() + 2 * (4 * (W + 3) + 8))
    assert np.array_equal(read(r, H, W), cut.numpy())
    assert np.array_equal(read(device_plane(cut, H, W, origin="top"), H, W), cut.numpy()[::-1])
    rows2 = device_plane(cut[1:3], 2, W, origin="top")  # a band of two rows
    assert np.array_equal(read(rows2, 2, W), cut.numpy()[1:3][::-1])
    flat = torch.from_numpy(rng.rand(H, W).astype(np.float32))
    d = device_plane(flat, H, W)
    assert (d.channels, d.stride_x, d.stride_y) == (1, 1, W) and np.array_equal(read(d, H, W)[..., 0], flat.numpy())
    with pytest.raises(ValueError):
        device_plane(flat, H + 1, W)
    with pytest.raises(ValueError):
        device_plane(flat, H, W, origin="left")
    with pytest.raises(TypeError):
        device_plane(flat.double(), H, W)


def test_context_call_takes_plane_records():
    """anything but an abi.DevicePlane never reaches the library; `view_z` names the depth plane"""
    import torch
    from rfx_amd.context import Context
    ctx = Context.__new__(Context)  # (no library call is made: the check comes first)
    ctx.W, ctx.H = 7, 5
    for bad in (torch.zeros(5, 7), np.zeros((5, 7), np.float32)):
        with pytest.raises(TypeError, match="abi.DevicePlane"):
            ctx._aov_device_frame(dict(depth=bad), None, None)
    f, r0, n = ctx._aov_device_frame(dict(view_z=abi.DevicePlane(4096, abi.PLANE_F32, 1, 1, 7, 0)), None, None)
    assert (f.depth.data, r0, n) == (4096, 0, 5) and not f.normal.data


@needs_hostsim
def test_gpu_file_on_the_host_simulator():
    """tests/test_gpu_stage_aov_device.py with the host simulator's library in place of the device's: explicit DevicePlane records over numpy
    arrays (simulator "device" memory is host memory)"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    env = {k: v for k, v in os.environ.items() if k not in ("RFX_HOSTSIM", "RFX_TEST_LIB")}
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--hostsim", "-p", "no:cacheprovider", os.path.join(HERE, "test_gpu_stage_aov_device.py")],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert " passed" in p.stdout and "skipped" not in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]
