"""Test helper: the layouts, the "device" memory and the reference of the device-plane tests (tests/test_gpu_stage_aov_device.py on the device
and under --hostsim, tests/test_stage_aov_device_cpu.py for the plan's restatement and the refusals).

A LAYOUT turns the contiguous (rows, W, C) array of a plane's element values (row 0 = the band's first frame row) into a flat backing array and
the offset and element strides that address the same values in it: `lay` is pure numpy and `gather` reads a layout back, so the layouts are
checked here before any kernel sees them.  `Arena` puts backing arrays where the library can read them — hipMalloc'ed memory on the
device, 256-byte-aligned host memory under the host simulator, whose "device" memory is host memory — and `plane` gives the abi.DevicePlane.

The reference everywhere is the merged host path: the same element values as contiguous host arrays through Context.stage_aov on a second
context, both contexts flipped, the held rows of DEPTH, GBUFFER, VELOCITY and DIRECT_LIGHT compared as bytes."""
import os

import numpy as np

import aov_cases as AC

HOSTSIM = bool(os.environ.get("RFX_HOSTSIM"))
SIZES = [(1, 1), (3, 2), (4, 3), (5, 4), (66, 5), (97, 55)]
# tight: the staging area's own layout (the flat kernel); pitch1 / pitch5: interleaved rows padded by 1 and 5 elements (misaligned row starts:
# the element form); pitch4: interleaved rows padded to the next multiple of four, and four more (the interleaved vector form); planar:
# (C, H, W) (the planar vector form where W is a multiple of four, else the element form); planar_pitch: planar with rows padded to a multiple
# of four and a plane pitch of eight more elements (the planar vector form at every width); top: image row 0 at the top (negative stride_y);
# mirror_x: negative stride_x; offset1: tight, base one element in; broadcast: roughness and metalness one element each, all strides 0
LAYOUTS = ("tight", "pitch1", "pitch5", "pitch4", "planar", "planar_pitch", "top", "mirror_x", "offset1", "broadcast")
TYPES = {"f32": 0, "typed": AC.TYPED, "mix": AC.BIT["diffuse"] | AC.BIT["roughness"] | AC.BIT["velocity"] | AC.BIT["direct"] | AC.BIT["depth"]}
PAD = 7.0  # what the elements no plane addresses hold


def lay(v, layout):
    """(rows, W, C) or (rows, W) values -> (flat backing array, offset of element (x 0, row 0, channel 0), stride_x, stride_y, stride_c)"""
    H, W = v.shape[:2]
    C = 1 if v.ndim == 2 else v.shape[2]
    v = np.ascontiguousarray(v).reshape(H, W, C)
    if layout in ("tight", "offset1", "broadcast"):
        off = 1 if layout == "offset1" else 0
        flat = np.full(off + v.size, PAD, v.dtype)
        flat[off:] = v.reshape(-1)
        return flat, off, C, W * C, 1
    if layout in ("pitch1", "pitch5", "pitch4"):
        pitch = W * C + {"pitch1": 1, "pitch5": 5, "pitch4": (-W * C) % 4 + 4}[layout]
        buf = np.full((H, pitch), PAD, v.dtype)
        buf[:, :W * C] = v.reshape(H, W * C)
        return buf.reshape(-1), 0, C, pitch, 1
    if layout == "planar":
        return np.ascontiguousarray(v.transpose(2, 0, 1)).reshape(-1), 0, 1, W, H * W
    if layout == "planar_pitch":
        wp = W + (-W) % 4 + 4
        plane = H * wp + 8
        buf = np.full((C, plane), PAD, v.dtype)
        for c in range(C):
            rows = buf[c, :H * wp].reshape(H, wp)
            rows[:, :W] = v[:, :, c]
        return buf.reshape(-1), 0, 1, wp, plane
    if layout == "top":
        return np.ascontiguousarray(v[::-1]).reshape(-1), (H - 1) * W * C, C, -W * C, 1
    if layout == "planar_top":
        return np.ascontiguousarray(v[::-1].transpose(2, 0, 1)).reshape(-1), (H - 1) * W, 1, -W, H * W
    if layout == "planar_pitch_top":  # planar_pitch with the image's row 0 at the top: a negative stride_y in the planar vector form
        flat, _, sx, sy, sc = lay(v[::-1], "planar_pitch")
        return flat, (H - 1) * sy, sx, -sy, sc
    if layout == "pitch4_top":        # ... in the interleaved vector form
        flat, _, sx, sy, sc = lay(v[::-1], "pitch4")
        return flat, (H - 1) * sy, sx, -sy, sc
    if layout == "mirror_x":
        return np.ascontiguousarray(v[:, ::-1]).reshape(-1), (W - 1) * C, -C, W * C, 1
    if layout == "one":
        assert (v == v.reshape(-1)[0]).all()
        return v.reshape(-1)[:1].copy(), 0, 0, 0, 0
    raise ValueError(layout)


def gather(flat, off, sx, sy, sc, H, W, C):
    """the (H, W, C) values a layout addresses"""
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    return flat[off + x * sx + y * sy + c * sc]


_HIP = None


def hip():
    """the HIP runtime the library itself runs on (already in the process once the library is loaded), for the tests' own device buffers:
    a second runtime in the process — torch's, initialised after the library's — finds no device"""
    global _HIP
    if _HIP is None:
        import ctypes as C
        from rfx_amd import abi
        abi.load_library()
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
        assert len(paths) == 1, paths
        _HIP = C.CDLL(paths[0])
        _HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.hipFree.argtypes = [C.c_void_p]
    return _HIP


class Arena:
    """backing arrays in memory the library reads as device memory: hipMalloc'ed on the device, 256-byte-aligned host memory under the host
    simulator; keeps them alive until it goes"""

    def __init__(self):
        self.keep = []

    def put(self, flat):
        """-> the address of flat[0], 256-byte aligned"""
        raw = np.ascontiguousarray(flat).view(np.uint8).reshape(-1)
        if HOSTSIM:
            buf = np.empty(raw.size + 256, np.uint8)
            at = (-buf.ctypes.data) % 256
            buf[at:at + raw.size] = raw
            self.keep.append(buf)
            return buf.ctypes.data + at
        import ctypes as C
        p = C.c_void_p()
        assert hip().hipMalloc(C.byref(p), raw.size) == 0 and p.value and p.value % 256 == 0
        self.keep.append(p.value)
        assert hip().hipMemcpy(p, raw.ctypes.data, raw.size, 1) == 0  # (host to device, complete on return)
        return p.value

    def ready(self):
        """the copies into device memory have executed: the planes are complete (what a call without a producer stream requires)"""
        if not HOSTSIM:
            assert hip().hipDeviceSynchronize() == 0

    def __del__(self):
        if not HOSTSIM and _HIP is not None:
            for p in self.keep:
                _HIP.hipFree(p)  # (waits for the device: no kernel is still reading it)


def plane(arena, v, layout):
    from rfx_amd import abi
    flat, off, sx, sy, sc = lay(v, layout)
    C = 1 if v.ndim == 2 else v.shape[2]
    return abi.DevicePlane(arena.put(flat) + off * v.dtype.itemsize, abi.PLANE_TYPES[v.dtype], C, sx, sy, sc)


def device_planes(arena, staged, layout, row0=0, rows=None):
    """the band [row0, row0 + rows) of whole-frame staged planes as abi.DevicePlane records in one layout ("broadcast": roughness and metalness
    from one element — `constant` made them so —, the rest tight)"""
    out = {}
    for k, v in staged.items():
        band = v[row0:None if rows is None else row0 + rows]
        out[k] = plane(arena, band, "one" if layout == "broadcast" and k in ("roughness", "metalness") else layout)
    arena.ready()
    return out


def constant(staged):
    """the staged planes with a constant roughness and metalness (what a broadcast plane can hold)"""
    out = dict(staged)
    for k, c in (("roughness", 0.375), ("metalness", 0.75)):
        if k in out:
            out[k] = np.full_like(out[k], c)
    return out


def frame(W, H, seed, non_finite=True):
    """aov_cases.random_planes (depth == 1 texels included) with non-finite velocities on a few covered texels"""
    p = {k: np.array(v) for k, v in AC.random_planes(W, H, seed).items()}
    if non_finite and W * H >= 6:
        v = p["velocity"].reshape(-1, 2)
        v[1, 0], v[2, 1], v[W * H - 2] = np.inf, -np.inf, (np.inf, np.inf)
    return p


def tex():
    from rfx_amd import abi
    return (abi.TEX_DEPTH, abi.TEX_GBUFFER, abi.TEX_VELOCITY, abi.TEX_DIRECT_LIGHT)


def context(W, H, tile=None, conv=None):
    from rfx_amd.context import Context
    ctx = Context(W, H) if tile is None else Context(W, H, tile_y0=tile[0], tile_rows=tile[1], halo_rows=tile[2])
    if conv is not None:
        ctx.set_aov_conventions(conv)
    return ctx


def slots_of(ctx):
    return [ctx.download(t) for t in tex()]


def host_reference(W, H, staged, tile=None, conv=None):
    """the merged host path: contiguous host arrays through stage_aov on a context of its own"""
    ctx = context(W, H, tile, conv)
    ctx.stage_aov({k: np.ascontiguousarray(v) for k, v in staged.items()})
    ctx.stage_flip()
    out = slots_of(ctx)
    ctx.close()
    return out


def same_bytes(got, want, written=(True, True, True, True)):
    """[messages] for the written slots whose bytes differ"""
    return AC.differing(got, [w if on else None for w, on in zip(want, written)])
