"""CPU (-m "not gpu") side of the device images (include/rfx.h rfx_export_device, rfx_queue_wait_stream, rfx_stream_wait_queue): the header
against the ctypes mirror, the store plan as the library computes it (rfx_launch.h rfx_export_device_plan_for, through the host simulator's
build) against export_device_cases.restated_form over seeded random strides, alignments, formats and tiles and over hand-made cases at the
edges of the nesting and extent rules, the test layouts and the case list themselves, the tensor-to-image function on CPU tensors, the Python
checks that come before the library, and a run of tests/test_gpu_export_device.py on the host simulator, so that the entry points and the
strided kernel's indexing are exercised where there is no device."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import export_device_cases as X
from launch_plans import needs_hostsim
from rfx_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE = 0x7f0000001000


def test_header_and_ctypes_mirror_agree(tmp_path):
    fields = ("data", "stride_x", "stride_y", "stride_c")
    exprs = ["sizeof(rfx_device_image)"] + ["offsetof(rfx_device_image, %s)" % n for n in fields] + ["(size_t)RFX_QUEUE_DRAW", "(size_t)RFX_QUEUE_UPLOAD", "(size_t)RFX_ABI_VERSION"]
    protos = ("int (*e0)(rfx_ctx *, const rfx_export_params *, const rfx_device_image *) = rfx_export_device;\n"
              "int (*e1)(rfx_ctx *, int, void *) = rfx_queue_wait_stream;\nint (*e2)(rfx_ctx *, int, void *) = rfx_stream_wait_queue;\n")
    body = '#include <stdio.h>\n#include <stddef.h>\n#include "rfx.h"\n%sint main(){size_t v[] = {%s};\nfor (unsigned i = 0; i < sizeof v / sizeof v[0]; i++) printf("%%zu ", v[i]);\nreturn 0;}\n'
    c = tmp_path / "img.c"
    c.write_text(body % (protos, ", ".join(exprs)))
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "img.o")])  # (the prototypes, type-checked)
    c.write_text(body % ("", ", ".join(exprs)))
    exe = tmp_path / "img"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.DeviceImage)] + [getattr(abi.DeviceImage, n).offset for n in fields] + [abi.QUEUE_DRAW, abi.QUEUE_UPLOAD, abi.RFX_ABI_VERSION]
    assert C.sizeof(abi.DeviceImage) == 32 and got[1:5] == [0, 8, 16, 24] and abi.RFX_ABI_VERSION == 21  # additive: no version bump
    lib = abi.load_library()
    for name in ("rfx_export_device", "rfx_queue_wait_stream", "rfx_stream_wait_queue"):
        assert name in abi.EXPORTS and hasattr(lib, name)
    from rfx_amd.context import Context
    assert isinstance(Context.has_export_device, property)


_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
I, U, L = ctypes.c_int, ctypes.c_ulonglong, ctypes.c_longlong
class Flat(ctypes.Structure):
    _fields_ = [(n, I) for n in ("pixels", "groups", "blocks", "tail_start", "tail_pixels", "elem_bytes", "pixel_bytes", "group_bytes")] + [("bytes", U)]
class Plan(ctypes.Structure):
    _fields_ = [(n, I) for n in ("form", "elem_bytes", "groups_x", "tail_x", "tail_pixels", "lanes_x", "grid_x", "grid_y")] + [("flat", Flat)]
lib.rfx_internal_export_device_plan.argtypes = [I, I, I, I, U, L, L, L, ctypes.POINTER(Plan)]
out = []
for W, rows, fmt, ch, addr, sx, sy, sc in json.load(sys.stdin):
    t = Plan()
    t.form = -7
    rc = lib.rfx_internal_export_device_plan(W, rows, fmt, ch, addr, sx, sy, sc, ctypes.byref(t))
    out.append(dict(rc=rc, form=t.form, elem=t.elem_bytes, groups_x=t.groups_x, tail_x=t.tail_x, tail_pixels=t.tail_pixels, lanes_x=t.lanes_x, grid_x=t.grid_x,
                    grid_y=t.grid_y, flat=[t.flat.pixels, t.flat.groups, t.flat.blocks, t.flat.tail_start, t.flat.tail_pixels, t.flat.bytes]))
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


def random_cases(n=480, seed=0xe1b0a7):
    """[W, rows, format, channels, addr, stride_x, stride_y, stride_c]: the layouts callers keep, with the pitches and base offsets that move
    them between the forms, and the ways they go wrong — rows or planes that overlap, a 0 stride, an address off its element size, anything"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        W, rows = int(rng.randint(1, 140)), int(rng.randint(1, 60))
        fmt, ch = int(rng.randint(3)), int(rng.choice([3, 4]))
        e = (4, 2, 1)[fmt]
        pitch = int(rng.choice([0, 0, 1, 2, 4, 5, 8]))
        kind = int(rng.randint(10))
        if kind == 0:    # tight
            s = (ch, W * ch, 1)
        elif kind == 1:  # interleaved, pitched
            s = (ch, W * ch + pitch, 1)
        elif kind == 2:  # planar, pitched rows and planes
            s = (1, W + pitch, (W + pitch) * rows + int(rng.choice([0, 2, 4, 8])))
        elif kind == 3:  # top-down
            s = (ch, -(W * ch + pitch), 1)
        elif kind == 4:  # scanline-planar
            s = (1, ch * (W + pitch), W + pitch)
        elif kind == 5:  # mirrored x, mirrored channels
            s = [(-ch, W * ch + pitch, 1), (ch, W * ch, -1), (-1, W, -W * rows)][int(rng.randint(3))]
        elif kind == 6:  # rows or planes that overlap by a few elements
            s = [(ch, W * ch - 1 - int(rng.randint(3)), 1), (1, W, W * rows - 1 - int(rng.randint(W))), (1, W - 1, W * rows)][int(rng.randint(3))]
        elif kind == 7:  # a 0 stride
            s = [(0, W * ch, 1), (ch, 0, 1), (ch, W * ch, 0)][int(rng.randint(3))]
        else:            # anything
            s = tuple(int(v) for v in rng.randint(-9, 10, 3))
        addr = BASE + 256 * int(rng.randint(1 << 20)) + e * int(rng.choice([0, 0, 0, 1, 2, 4, 8])) + int(rng.choice([0, 0, 0, 0, 0, 0, 1, 2]))
        out.append([W, rows, fmt, ch, addr, s[0], s[1], s[2]])
    return out


def expected(case):
    W, rows, fmt, ch = case[:4]
    form = X.restated_form(*case)
    if form is None:
        return None
    lanes = W // 4 + (1 if W % 4 else 0)
    px = W * rows
    flat = [px, px // 4, -(-(px // 4 + (1 if px % 4 else 0)) // 256), px // 4 * 4, px % 4, px * ch * (4, 2, 1)[fmt]] if form == X.TIGHT else [0] * 6
    return dict(rc=0, form=form, elem=(4, 2, 1)[fmt], groups_x=W // 4, tail_x=W // 4 * 4, tail_pixels=W % 4, lanes_x=lanes, grid_x=-(-lanes // 64), grid_y=-(-rows // 4), flat=flat)


@needs_hostsim
def test_plan_against_the_restatement():
    cases = random_cases()
    assert len(cases) >= 400
    plans = device_plans(cases)
    seen, refused = set(), 0
    for case, t in zip(cases, plans):
        want = expected(case)
        if want is None:
            assert t["rc"] == abi.RFX_EINVAL and t["form"] == -7, (case, t)  # (*out untouched)
            refused += 1
            continue
        assert t == want, (case, t, want)
        seen.add(want["form"])
    print("export device plan: %d of %d random cases refused, forms seen %s" % (refused, len(cases), sorted(seen)))
    assert seen == {X.TIGHT, X.INTERLEAVED, X.PLANAR, X.ELEMENT}
    assert 0.10 * len(cases) < refused < 0.75 * len(cases), refused  # neither side is starved


@needs_hostsim
def test_plan_at_the_edges_of_its_rules():
    """just inside and just outside: the nesting rule on every pair of axes, the extent rule with products that overflow 64 bits, the
    alignments that separate the forms"""
    W, H = 5, 4
    lim = 2 ** 62 - 1
    inside = [
        [W, H, 0, 3, BASE, 3, 15, 1],            # tight
        [W, H, 0, 3, BASE, 3, 16, 1],            # one element of row padding
        [W, H, 1, 4, BASE, 4, -20, 1],           # top-down, rows touching
        [W, H, 2, 3, BASE, 1, 5, 20],            # planar, planes touching
        [W, H, 2, 3, BASE, 1, 15, 5],            # scanline-planar, planes touching inside the row
        [W, H, 2, 4, BASE, -4, 20, -1],          # both mirrored
        [W, H, 0, 3, BASE, 12, 3, 1],            # column-major: x steps over whole columns of rows
        [1, H, 0, 3, BASE, 0, 3, 1],             # one column: stride_x is not read
        [W, 1, 0, 3, BASE, 3, 0, 1],             # one row: stride_y is not read
        [1, 1, 1, 4, BASE + 2, 0, 0, 1],
        [W, H, 0, 3, BASE, 3, (lim // 4 - 1 - 2 - 12) // 3, 1],            # the extent, just inside: 1 + 2 sc + 4 sx + 3 sy elements of 4 bytes
        [W, H, 2, 3, BASE, 3, -((lim - 1 - 2 - 12) // 3), 1],
        [W, H, 1, 4, BASE, 1, 5, -((lim // 2 - 1 - 4 - 15) // 3)],
    ]
    outside = [
        [W, H, 0, 3, BASE, 3, 14, 1],            # rows overlap by one element
        [W, H, 1, 4, BASE, 4, -19, 1],
        [W, H, 2, 3, BASE, 1, 5, 19],            # planes overlap by one element
        [W, H, 2, 3, BASE, 1, 14, 5],            # scanline-planar, the last plane runs into the next row
        [W, H, 2, 3, BASE, 1, 15, 4],            # ... a plane pitch inside the row
        [W, H, 0, 3, BASE, 2, 15, 1],            # 3 channels in a pixel step of 2
        [W, H, 0, 3, BASE, 11, 3, 1],            # column-major, columns overlap
        [W, H, 0, 3, BASE, 0, 15, 1], [W, H, 0, 3, BASE, 3, 0, 1], [W, H, 0, 3, BASE, 3, 15, 0],   # a 0 stride
        [W, H, 0, 3, BASE, 3, 3, 1],             # two axes with one stride
        [1, 1, 0, 3, BASE, 3, 15, 0],            # the channel axis always steps
        [W, H, 0, 3, BASE, 3, (lim // 4 - 1 - 2 - 12) // 3 + 1, 1],        # the extent, just outside
        [W, H, 2, 3, BASE, 3, -((lim - 1 - 2 - 12) // 3) - 1, 1],
        [W, H, 1, 4, BASE, 1, 5, -((lim // 2 - 1 - 4 - 15) // 3) - 1],
        [W, H, 0, 3, BASE, 3, 2 ** 62, 1], [W, H, 0, 3, BASE, -2 ** 63, 15, 1], [W, H, 2, 4, BASE, 4, 2 ** 63 - 1, 1], [W, H, 2, 3, BASE, 2 ** 60, -2 ** 62, 2 ** 57],
        [W, H, 1, 3, BASE, 2 ** 58, -2 ** 61, 1],
        [W, H, 0, 3, BASE + 2, 3, 15, 1], [W, H, 0, 3, BASE + 1, 3, 15, 1], [W, H, 1, 3, BASE + 1, 3, 15, 1],  # the address against the element size
        [W, H, 0, 3, 0, 3, 15, 1],               # data NULL
        [W, H, 3, 3, BASE, 3, 15, 1], [W, H, 0, 2, BASE, 2, 10, 1], [W, H, 0, 5, BASE, 5, 25, 1], [0, H, 0, 3, BASE, 3, 15, 1], [W, 0, 0, 3, BASE, 3, 15, 1],
    ]
    for case in inside:
        assert X.restated_form(*case) is not None, case
    for case in outside:
        assert X.restated_form(*case) is None, case
    got = device_plans(inside)
    assert [t["rc"] for t in got] == [0] * len(inside)
    assert [t["form"] for t in got] == [X.restated_form(*c) for c in inside]
    assert [t["rc"] for t in device_plans(outside)] == [abi.RFX_EINVAL] * len(outside)
    # the alignments between the forms: (format, channels, base offset in bytes, strides) -> form
    T, I, P, E = X.TIGHT, X.INTERLEAVED, X.PLANAR, X.ELEMENT
    forms = [
        ([8, H, 0, 3, BASE + 4, 3, 24, 1], T), ([8, H, 1, 3, BASE + 2, 3, 24, 1], E), ([8, H, 1, 3, BASE + 4, 3, 24, 1], T), ([8, H, 2, 3, BASE + 3, 3, 24, 1], E),
        ([8, H, 1, 3, BASE, 3, 25, 1], E), ([8, H, 1, 3, BASE, 3, 26, 1], I), ([8, H, 2, 3, BASE, 3, 26, 1], E), ([8, H, 2, 3, BASE, 3, 28, 1], I),
        ([8, H, 0, 3, BASE, 3, 25, 1], I), ([8, H, 2, 4, BASE, 4, -36, 1], I), ([8, 1, 2, 4, BASE, 4, 33, 1], E),
        ([8, H, 0, 4, BASE, 1, 8, 32], P), ([8, H, 0, 4, BASE + 8, 1, 8, 32], E), ([8, H, 0, 4, BASE + 16, 1, 8, 32], P), ([8, H, 1, 4, BASE + 4, 1, 8, 32], E),
        ([8, H, 1, 4, BASE + 8, 1, 8, 32], P), ([8, H, 2, 4, BASE + 4, 1, 8, 32], P), ([8, H, 2, 4, BASE + 2, 1, 8, 32], E), ([8, H, 0, 4, BASE, 1, 10, 40], E),
        ([8, H, 0, 4, BASE, 1, 12, 50], E), ([8, H, 0, 4, BASE, 1, -8, -32], P), ([8, H, 0, 4, BASE, 1, 32, 8], P), ([7, H, 0, 4, BASE, 1, 28, 7], E),
        ([8, H, 0, 4, BASE, -4, 32, 1], E), ([8, H, 0, 4, BASE, 4, 32, -1], E),
    ]
    for case, form in forms:
        assert X.restated_form(*case) == form, (case, X.restated_form(*case))
    assert [t["form"] for t in device_plans([c for c, _ in forms])] == [f for _, f in forms]


def test_layouts_address_their_values():
    """the helper's own premise: every layout addresses exactly the values it was given, every other element of the backing array holds PAD,
    and the strides satisfy the nesting rule"""
    rng = np.random.RandomState(5)
    for W, H in X.SIZES:
        for C_ in (3, 4):
            for fmt, dt in enumerate((np.float32, np.float16, np.uint8)):
                v = (rng.rand(H, W, C_) * 200 + 8).astype(dt)  # (no value equals PAD)
                for layout in X.LAYOUTS:
                    flat, off, sx, sy, sc = X.lay(v, layout)
                    img = abi.DeviceImage(0, sx, sy, sc)  # (the record keeps signed 64-bit strides)
                    assert np.array_equal(X.gather(flat, off, img.stride_x, img.stride_y, img.stride_c, H, W, C_), v), (layout, W, H, C_)
                    assert int((flat != dt(X.PAD)).sum()) == v.size, (layout, W, H, C_)  # ... and addresses nothing twice, nothing else
                    assert X.restated_form(W, H, fmt, C_, BASE + off * v.dtype.itemsize, sx, sy, sc) is not None, (layout, W, H, C_)


def test_case_list_covers_every_specialisation_in_every_form():
    cases = X.cases()
    assert {c[0] for c in cases} == set(X.LAYOUTS) and {c[1:3] for c in cases} == set(X.SIZES)
    assert all(len({c[3] for c in cases if c[0] == layout}) == 8 for layout in X.LAYOUTS)  # dealt out in turn: every layout sees all eight
    pairs = {(c[3], X.layout_form(c[0], c[1], c[2], X.SPECS[c[3]])) for c in cases}
    assert pairs == {(k, f) for k in range(8) for f in (X.TIGHT, X.INTERLEAVED, X.PLANAR, X.ELEMENT)}, sorted(pairs)
    assert len({X.case_id(c) for c in cases}) == len(cases)
    assert {s[:3] for s in X.SPECS} == {(f, c, "linear") for f in ("f32", "f16", "u8_srgb") for c in (3, 4)} | {("u8_srgb", c, "aces") for c in (3, 4)}


def _read(img, dtype, rows, W, ch):
    """the (rows, W, ch) values the image addresses, through its own pointer arithmetic"""
    e = np.dtype(dtype).itemsize
    out = np.empty((rows, W, ch), dtype)
    for y in range(rows):
        for x in range(W):
            for c in range(ch):
                out[y, x, c] = np.frombuffer((C.c_char * e).from_address(img.data + e * (x * img.stride_x + y * img.stride_y + c * img.stride_c)), dtype)[0]
    return out


def test_tensor_to_image_on_cpu_tensors():
    """context.device_image: permuted, sliced with pitch, origin="top", uint8 — every image addresses the tensor's own values; an `expand`ed
    tensor is made into a record and refused by the library's rule"""
    import torch
    from rfx_amd.context import device_image
    H, W = 5, 7
    rng = np.random.RandomState(9)
    chw = torch.from_numpy(rng.rand(3, H, W).astype(np.float32))
    p = device_image(chw.permute(1, 2, 0), H, W)
    assert (p.stride_x, p.stride_y, p.stride_c, p.data, p.format, p.channels) == (1, W, H * W, chw.data_ptr(), abi.EXPORT_F32, 3)
    assert np.array_equal(_read(p, np.float32, H, W, 3), chw.permute(1, 2, 0).numpy())
    top = device_image(chw.permute(1, 2, 0), H, W, origin="top")
    assert (top.stride_x, top.stride_y, top.stride_c, top.data) == (1, -W, H * W, chw.data_ptr() + 4 * (H - 1) * W)
    assert np.array_equal(_read(top, np.float32, H, W, 3), chw.permute(1, 2, 0).numpy()[::-1])
    wide = torch.from_numpy(rng.rand(H + 2, W + 3, 4).astype(np.float16))
    cut = wide[1:H + 1, 2:W + 2]
    r = device_image(cut, H, W)
    assert (r.stride_x, r.stride_y, r.stride_c, r.data, r.format, r.channels) == (4, 4 * (W + 3), 1, wide.data_ptr() + 2 * (4 * (W + 3) + 8), abi.EXPORT_F16, 4)
    assert np.array_equal(_read(r, np.float16, H, W, 4), cut.numpy())
    assert np.array_equal(_read(device_image(cut, H, W, origin="top"), np.float16, H, W, 4), cut.numpy()[::-1])
    assert np.array_equal(_read(device_image(cut[1:3], 2, W, origin="top"), np.float16, 2, W, 4), cut.numpy()[1:3][::-1])  # a band of two rows
    u8 = torch.from_numpy(rng.randint(0, 256, (H, W, 3)).astype(np.uint8))
    b = device_image(u8, H, W)
    assert (b.stride_x, b.stride_y, b.stride_c, b.format) == (3, 3 * W, 1, abi.EXPORT_U8_SRGB) and np.array_equal(_read(b, np.uint8, H, W, 3), u8.numpy())
    assert X.restated_form(W, H, 2, 3, b.data, b.stride_x, b.stride_y, b.stride_c) in (X.TIGHT, X.ELEMENT)
    for img, fmt in ((p, 0), (top, 0), (r, 1)):
        assert X.restated_form(W, H, fmt, img.channels, img.data, img.stride_x, img.stride_y, img.stride_c) is not None
    # an expanded tensor (one row, or one pixel, shown H x W times): a record like any other, refused by the nesting rule
    for t in (torch.zeros(1, W, 3).expand(H, W, 3), torch.zeros(1, 1, 4, dtype=torch.float16).expand(H, W, 4), torch.zeros(H, W, 1, dtype=torch.uint8).expand(H, W, 3)):
        q = device_image(t, H, W)
        assert 0 in (q.stride_x, q.stride_y, q.stride_c)
        assert X.restated_form(W, H, q.format, q.channels, q.data, q.stride_x, q.stride_y, q.stride_c) is None
    with pytest.raises(ValueError):
        device_image(u8, H + 1, W)
    with pytest.raises(ValueError):
        device_image(u8[..., 0], H, W)                 # (rows, W): an image has its channels
    with pytest.raises(ValueError):
        device_image(torch.zeros(H, W, 2), H, W)
    with pytest.raises(ValueError):
        device_image(u8, H, W, origin="left")
    with pytest.raises(TypeError):
        device_image(torch.zeros(H, W, 3, dtype=torch.float64), H, W)
    with pytest.raises(TypeError):
        device_image(torch.zeros(H, W, 3, dtype=torch.int32), H, W)


@needs_hostsim
def test_expanded_tensor_is_refused_by_the_plan():
    import torch
    from rfx_amd.context import device_image
    H, W = 5, 7
    keep = [torch.zeros(1, W, 3).expand(H, W, 3), torch.zeros(H, 1, 4, dtype=torch.float16).expand(H, W, 4), torch.zeros(H, W, 3, dtype=torch.uint8)]
    imgs = [device_image(t, H, W) for t in keep]
    got = device_plans([[W, H, q.format, q.channels, q.data, q.stride_x, q.stride_y, q.stride_c] for q in imgs])
    assert [t["rc"] for t in got] == [abi.RFX_EINVAL, abi.RFX_EINVAL, 0]


def test_python_checks_come_before_the_library():
    """anything but an abi.DeviceImage, a tensor of another dtype than the format, a stream that is no non-zero integer: refused in Python"""
    import torch
    from rfx_amd.context import Context, device_image

    class NoCalls:
        """stands in for the library: has the symbols, fails the test when one is called"""
        def __getattr__(self, name):
            if name in ("rfx_export_device", "rfx_stage_aov_device", "rfx_queue_wait_stream", "rfx_stream_wait_queue"):
                def called(*a):
                    raise AssertionError("%s was called" % name)
                return called
            raise AttributeError(name)

    ctx = Context.__new__(Context)  # (no context is made: every check below comes before the library)
    ctx.lib, ctx._h, ctx.W, ctx.H, ctx.tile_rows = NoCalls(), None, 7, 5, 5
    assert ctx.has_export_device and ctx.has_stage_aov_device
    for bad in (torch.zeros(5, 7, 3), np.zeros((5, 7, 3), np.float32), None, abi.DevicePlane()):
        with pytest.raises(TypeError, match="abi.DeviceImage"):
            ctx.export_device(abi.TEX_FINAL, "f32", 3, image=bad)
    img = device_image(torch.zeros(5, 7, 3, dtype=torch.float16), 5, 7)
    for fmt, ch in (("f32", 3), ("u8_srgb", 3), ("f16", 4)):
        with pytest.raises(ValueError, match="another dtype or channel count"):
            ctx.export_device(abi.TEX_FINAL, fmt, ch, image=img)
    for stream, err in ((0, ValueError), (1.5, TypeError), ("7", TypeError), (True, TypeError)):
        with pytest.raises(err):
            ctx.export_device(abi.TEX_FINAL, "f16", 3, image=img, stream=stream)
        with pytest.raises(err):
            ctx.stage_aov_device(dict(depth=abi.DevicePlane(4096, abi.PLANE_F32, 1, 1, 7, 0)), producer=stream)
        with pytest.raises(err):
            ctx.queue_wait_stream(abi.QUEUE_UPLOAD, stream)
        with pytest.raises(err):
            ctx.stream_wait_queue(abi.QUEUE_DRAW, stream)
    with pytest.raises(ValueError):
        ctx.stage_aov_device(dict(depth=abi.DevicePlane(4096, abi.PLANE_F32, 1, 1, 7, 0)), producer=0)


@needs_hostsim
def test_gpu_file_on_the_host_simulator():
    """tests/test_gpu_export_device.py with the host simulator's library in place of the device's: nothing skipped but the one case that
    needs streams that run side by side"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    env = {k: v for k, v in os.environ.items() if k not in ("RFX_HOSTSIM", "RFX_TEST_LIB")}
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--hostsim", "-p", "no:cacheprovider", "-rs", os.path.join(HERE, "test_gpu_export_device.py")],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert " passed" in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]
    assert re.search(r"\b1 skipped\b", p.stdout) and p.stdout.count("SKIPPED") == 1 and "no order to observe" in p.stdout, p.stdout[-2000:]
