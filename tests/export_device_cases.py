"""Test helper: the layouts, the readable "device" memory, the restated plan and the case list of the device-image tests
(tests/test_gpu_export_device.py on the device and under --hostsim, tests/test_export_device_cpu.py for the plan and the helper's own premises).

A LAYOUT (aov_device_cases.lay, plus the scanline-planar (H, C, W) one here) turns the contiguous (rows, W, C) array rfx_export returns into
the flat backing array a caller keeps and the offset and element strides that address the same values in it.  The tests pre-fill a backing
array with PAD, let rfx_export_device write the image into it and compare the WHOLE array with `lay(reference)`: the values and every padding
byte at once.  The reference everywhere is Context.export — the merged host path — on the same context."""
import ctypes as C

import numpy as np

import aov_device_cases as D
import export_cases as E
from aov_device_cases import HOSTSIM, PAD, SIZES, gather  # noqa: F401  (re-exported)

TIGHT, INTERLEAVED, PLANAR, ELEMENT = 0, 1, 2, 3
FORM_NAMES = ("tight", "interleaved", "planar", "element")
# the layouts of aov_device_cases that a store image can have (no broadcast: a 0 stride aliases), and "scanline": scanline-planar (H, C, W), the
# planar vector form where W is a multiple of four, the element form at every other width
LAYOUTS = ("tight", "offset1", "pitch1", "pitch5", "pitch4", "planar", "planar_pitch", "top", "planar_top", "planar_pitch_top", "pitch4_top", "mirror_x",
           "scanline")
# the eight K7 specialisations: (format, channels, tonemap, exposure)
SPECS = (("f32", 3, "linear", 1.0), ("f32", 4, "linear", 1.0), ("f16", 3, "linear", 1.0), ("f16", 4, "linear", 1.0),
         ("u8_srgb", 3, "linear", 1.0), ("u8_srgb", 4, "linear", 2.5), ("u8_srgb", 3, "aces", 0.37), ("u8_srgb", 4, "aces", 1.0))
ELEM = {"f32": 4, "f16": 2, "u8_srgb": 1}
FORMAT_ID = {"f32": 0, "f16": 1, "u8_srgb": 2}


def lay(v, layout):
    """aov_device_cases.lay, and the scanline-planar layout"""
    if layout == "scanline":
        H, W, Cn = v.shape
        return np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(-1), 0, 1, Cn * W, W
    return D.lay(v, layout)


def restated_form(W, rows, fmt, ch, addr, sx, sy, sc):
    """include/rfx.h "device images" and rfx_launch.h rfx_export_device_plan_for restated in Python integers (no overflow to mind): the store
    form, or None where the call is RFX_EINVAL.  fmt: 0 / 1 / 2 (F32 / F16 / U8_SRGB)"""
    if W <= 0 or rows <= 0 or fmt not in (0, 1, 2) or ch not in (3, 4):
        return None
    e = (4, 2, 1)[fmt]
    if addr == 0 or addr % e:
        return None
    axes = [(abs(s), n) for s, n in ((sx, W), (sy, rows), (sc, ch))]
    if (1 + sum(s * (n - 1) for s, n in axes)) * e > 2 ** 62 - 1:
        return None
    live = sorted(a for a in axes if a[1] > 1)
    if live and live[0][0] < 1:
        return None
    for (s0, n0), (s1, _) in zip(live, live[1:]):
        if s1 < s0 * n0:
            return None
    interleaved = sc == 1 and sx == ch
    if interleaved and addr % 4 == 0 and sy == W * ch:
        return TIGHT
    if interleaved and addr % 4 == 0 and (sy * e) % 4 == 0:
        return INTERLEAVED
    if sx == 1 and addr % (4 * e) == 0 and sy % 4 == 0 and sc % 4 == 0:
        return PLANAR
    return ELEMENT


def layout_form(layout, W, H, spec, base=0x7f0000001000):
    """the form of a whole-frame image in `layout` whose backing array starts at a 256-byte-aligned address"""
    fmt, ch = spec[0], spec[1]
    dtype = {"f32": np.float32, "f16": np.float16, "u8_srgb": np.uint8}[fmt]
    _, off, sx, sy, sc = lay(np.zeros((H, W, ch), dtype), layout)
    return restated_form(W, H, FORMAT_ID[fmt], ch, base + off * ELEM[fmt], sx, sy, sc)


def cases():
    """Case 1's list: every layout at every size (78), each with two specialisations dealt out in turn, four apart — so the six sizes of one
    layout see all eight — -> [(layout, W, H, spec index)].  tests/test_export_device_cpu.py checks that every (specialisation, form) pair occurs."""
    out = []
    for i, layout in enumerate(LAYOUTS):
        for j, (W, H) in enumerate(SIZES):
            for k in (0, 4):
                out.append((layout, W, H, (i + j + k) % 8))
    return out


def case_id(c):
    return "%s-%dx%d-%s%d%s" % (c[0], c[1], c[2], SPECS[c[3]][0], SPECS[c[3]][1], SPECS[c[3]][2][0])


def input_frame(W, H, seed=0):
    """(H, W, 4) float32 for RFX_TEX_EFFECT_INPUT: export_cases' planted frames — NaN, +-inf, negatives, values above 65504 (linear_input), the
    half roundings: subnormals, ties, overflow to inf (f16_input) — and the sRGB transfer function's branch point with both neighbours.  A frame
    too small for linear_input's plants is f16_edge_input's values alone."""
    if W * H < 64:
        a = E.f16_edge_input(W, H).copy()
    else:
        a = E.linear_input(W, H, "lognormal").copy()
        flat = a.reshape(-1)
        special = E.f16_input(W, H).reshape(-1)[:16]
        b = np.float32(0.0031308)
        branch = np.array([b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1)), 0.0031, 0.0032, 1.0, np.nextafter(np.float32(1), np.float32(0))], np.float32)
        flat[8:8 + special.size] = special
        flat[32:32 + branch.size] = branch
        flat[-special.size - 4:-4] = special[::-1]  # ... and in the last row's tail pixels
    if seed:
        a = np.roll(a, 4 * seed + 1, axis=1) if W > 1 else a
        a = (a * np.float32(1.0 + 0.25 * seed)).astype(np.float32)
    return np.ascontiguousarray(a)


class ReadArena(D.Arena):
    """aov_device_cases.Arena whose backing arrays can be read back: hipMemcpy device -> host on the device (the caller has made the writes
    complete: Context.sync or a synchronised stream), the memory itself under the simulator"""

    def put(self, flat):
        addr = super().put(flat)
        self.__dict__.setdefault("sizes", {})[addr] = np.ascontiguousarray(flat).nbytes
        return addr

    def blank(self, like):
        """a backing array of `like`'s size and dtype holding PAD everywhere -> its address"""
        return self.put(np.full(like.shape, PAD, like.dtype))

    def read(self, addr):
        """the bytes of the backing array at `addr`"""
        n = self.sizes[addr]
        if HOSTSIM:
            return C.string_at(addr, n)
        out = np.empty(n, np.uint8)
        assert D.hip().hipMemcpy(out.ctypes.data, addr, n, 2) == 0  # (device to host, complete on return)
        return out.tobytes()


def image(addr, off, sx, sy, sc, itemsize):
    from rfx_amd import abi
    return abi.DeviceImage(addr + off * itemsize, sx, sy, sc)


class Streams:
    """the tests' own streams and copies, on the HIP runtime the library runs on; under the simulator, whose streams are immediate, a stream is
    a made-up non-zero handle and a copy a memmove"""

    def __init__(self):
        self.made = []
        if not HOSTSIM:
            h = D.hip()
            h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
            h.hipStreamDestroy.argtypes = [C.c_void_p]
            h.hipStreamSynchronize.argtypes = [C.c_void_p]
            h.hipStreamQuery.argtypes = [C.c_void_p]
            h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            h.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]

    def stream(self):
        if HOSTSIM:
            self.made.append(0x1000 + 16 * len(self.made))
            return self.made[-1]
        s = C.c_void_p()
        assert D.hip().hipStreamCreateWithFlags(C.byref(s), 1) == 0 and s.value  # (hipStreamNonBlocking)
        self.made.append(s.value)
        return s.value

    def copy_async(self, dst, src, n, kind, stream):
        """kind: 1 host -> device, 3 device -> device"""
        if HOSTSIM:
            C.memmove(dst, src, n)
        else:
            assert D.hip().hipMemcpyAsync(dst, src, n, kind, stream) == 0

    def sync(self, stream):
        if not HOSTSIM:
            assert D.hip().hipStreamSynchronize(stream) == 0

    def close(self):
        if not HOSTSIM:
            for s in self.made:
                D.hip().hipStreamSynchronize(s)
                D.hip().hipStreamDestroy(s)
        self.made = []
