#!/usr/bin/env python3
"""What the input side of a run over a dumped sequence costs at 4K (GPU box; fails without a device): wall time per frame of the SSGI chain
(steps 20 / refineSteps 5) when every frame's planes cross PCIe as

    P0  a packed dump, stage_upload from two pinned sets (52 B/px)
    A0  an AOV frame through the synchronous importer: pack_gbuffer + pack_velocity + upload of depth and direct, float32, pageable (96 B/px)
    A1  an AOV frame through stage_aov, every plane float32, two pinned sets (76 B/px)
    A2  the typed AOV frame through stage_aov: diffuse, normal, roughness, metalness, emissive, direct as halves, velocity and depth float32 (44 B/px)

on the seeded dump whose AOV planes are rounded to half wherever A2 sends halves (all four modes see the same values), in ONE process: every
mode is warmed first, then three alternating rounds, each mode a steady state of at least --seconds with a device synchronise inside the clock.

--modes E0,E1: the same typed frame as an OpenEXR file — multi-part, one part per plane, half / float as A2 types them, written once per
compression (ZIPS, ZIP) —

    E0  file -> imageio.exr_to_typed_planes (the host inflates, unpredicts, de-interleaves) -> stage_aov
    E1  file -> readinto a pinned buffer -> imageio.exr_aov_layout (header and offset table) -> stage_exr_aov (the device decodes: K9)

measured the same way, per compression, with A2 in the same rounds; the result is merged into --out under "exr".

--forms tiled_zip,pxr24,rle (with --modes E0,E1): the file forms of rfx.h "EXR blocks" — the same typed frame as ZIP tiles of 64 x 64, as PXR24
scanline chunks (depth and velocity, the FLOAT planes, keep 24 bits in that file; E0 and E1 read the same file) and as RLE scanline chunks — where
E1 is readinto + imageio.exr_aov_layout(forms="blocks") + stage_exr_blocks; "zip" is measured in the same run through the same call, so that every
new figure has E1's ZIP figure beside it.  The result is merged into --out under "exr_blocks".  The RLE file is written by a vectorised coder
of this tool (imageio's is a byte loop), and its E0 — imageio's byte loop again — is timed over --e0-frames frames only.

--forms piz,tiled_piz (with --modes E0,E1): the typed frame as PIZ scanline blocks of 32 rows and as PIZ tiles of 64 x 64, decoded on the device on
request (rfx.h "EXR blocks with PIZ"): E1 is readinto + imageio.exr_aov_layout(forms="blocks", piz=True) + stage_exr_blocks.  imageio's PIZ
writer and reader are Python loops of a few microseconds per 16-bit word, so frame 0's file is written once (and kept: with --exr-dir a later run
reuses it) and serves both staging slots, and E0 — the host decode, where such a file goes by default — is not looped: the host's
imageio._exr_unpack_block is timed over the blocks of the file's first block row (32 scanlines, or one row of tiles) and scaled by height / those
rows ("E0_band_scaled"; the de-interleave and stage_aov behind it, milliseconds, are not in it).  Merged into --out under "exr_piz".  With them: K9_PIZ_FAST_BITS, the waves per CU
the decode's LDS leaves, and the table scratch bytes of the frame.

--modes C2: the typed frame as an engine writes it (rfx.h "AOV conventions"): a float32 world position in place of depth and velocity, camera-space
normals, no velocity plane — POSITION + CAMERAS + VIEW, set per frame — the same 44 B/px, through stage_aov, beside A2 in three alternating
rounds; with --parent-lib PATH (a librfx_hip.so built from the parent commit, loaded into the same process on a context of its own) A2 on that
library too, so that each round is an A/B/C triple.  Beside each: "stage_only", the wall time of stage + flip + sync without draws — the copies
with the pack kernel behind them, where a kernel that leaves the copy's shadow shows.  Merged into --out under "conventions".

--modes A2,D2,D2p: the typed frame RESIDENT in device memory (rfx.h "device planes"; hipMalloc'ed on the library's own runtime, handed over as
abi.DevicePlane records, no torch in the process), through stage_aov_device:

    D2   tight and interleaved, row 0 at the bottom: the staging area's own layout — k0_aov_pack on the caller's pointers
    D2p  the same values as planar (C, H, W) planes, image row 0 at the top: the strided kernel's planar form
    D2i  (--kernel-only) interleaved rows padded by four elements: the strided kernel's interleaved form

each stage + flip + the chain's draws beside A2 in three alternating rounds; D2 < A2 and D2p < A2 is required in every round (A2 is the PCIe copy
the D modes do not make).  Merged into --out under "device_planes".  With --kernel-only: A2, D2, D2p, D2i, stage + flip alone, for one kernel trace.

    python tools/import_rate.py [--modes P0,A0,A1,A2 | E0,E1 | C2 | A2,D2,D2p] [--out profiles/import/rates.json] [--seconds 1.0]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/import_rate.py --kernel-only --modes A2,D2,D2p   (... flat beside strided, device planes)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/import_rate.py --kernel-only      (the pack kernel's own time: a run of its own)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/import_rate.py --kernel-only --modes E1      (... and the K9 kernels')
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/import_rate.py --kernel-only --modes C2      (... default beside converting)
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))

from rfx_amd import abi, effect, imageio  # noqa: E402
from rfx_amd.context import Context  # noqa: E402
from rfx_amd.scene import AnalyticScene, _pool_worker_init  # noqa: E402

W, H = 3840, 2160
MODES = ("P0", "A0", "A1", "A2")
EXR_MODES = ("E0", "E1")
EXR_COMPRESSIONS = ("zips", "zip")
# --forms: name -> (compression, tiles); the two above are the forms rfx_stage_exr_aov takes, the others go through rfx_stage_exr_blocks
EXR_FORMS = {"zips": ("zips", None), "zip": ("zip", None), "tiled_zip": ("zip", (64, 64)), "pxr24": ("pxr24", None), "rle": ("rle", None),
             "piz": ("piz", None), "tiled_piz": ("piz", (64, 64))}
BLOCK_FORMS = ("tiled_zip", "pxr24", "rle", "piz", "tiled_piz")
PIZ_FORMS = ("piz", "tiled_piz")
# csrc/k9_piz.h: the primary table's bits, the LDS of one decoding wave (K9PizHuf + the 64 counts of the bitmap scan), a block's table scratch
PIZ_FAST_BITS, PIZ_WAVE_LDS, PIZ_TABLE_BYTES, CU_LDS = 12, 17824, 131072 + 131328 + 256, 160 * 1024


def rle_compress_fast(buf: bytes) -> bytes:
    """imageio._rle_compress's code (runs of 3 .. 128, literals up to 127) with the run search in numpy: a valid stream of the same format, not
    necessarily the same bytes"""
    a = np.frombuffer(buf, np.uint8)
    n = a.size
    if n == 0:
        return b""
    starts = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
    lens = np.diff(np.concatenate((starts, [n])))
    out, lit0 = bytearray(), 0  # lit0: where the pending literal stretch starts

    def flush(end):
        nonlocal lit0
        while lit0 < end:
            m = min(127, end - lit0)
            out.append(256 - m)
            out.extend(buf[lit0:lit0 + m])
            lit0 += m
    for s0, ln in zip(starts[lens >= 3].tolist(), lens[lens >= 3].tolist()):
        flush(s0)
        v = buf[s0]
        while ln >= 3:
            m = min(128, ln)
            out.append(m - 1)
            out.append(v)
            ln -= m
            s0 += m
        lit0 = s0  # (a rest of one or two bytes joins the next literal)
    flush(n)
    return bytes(out)
BYTES_PER_PIXEL = dict(P0=52, A0=96, A1=76, A2=44)
HALF = ("diffuse", "normal", "roughness", "metalness", "emissive", "direct")
AOV = ("diffuse", "normal", "roughness", "metalness", "emissive", "velocity")


def _band(args):
    seed, index, row0, rows = args
    f = AnalyticScene(seed).render(W, rows, index, row0=row0, rows=rows, frame_height=H, aov=True)
    return f.depth, f.gbuffer, f.velocity, f.direct, f.aov, f.camera


def render(seed, index, workers=16):
    """frame `index` of the seeded scene with its unpacked planes, ray-cast by a pool of processes"""
    import multiprocessing as mp
    edges = [H * i // workers for i in range(workers + 1)]
    jobs = [(seed, index, edges[i], edges[i + 1] - edges[i]) for i in range(workers) if edges[i + 1] > edges[i]]
    pool = mp.get_context("fork").Pool(len(jobs), initializer=_pool_worker_init)
    try:
        parts = pool.map(_band, jobs)
        pool.close()
        pool.join()
    except BaseException:
        pool.terminate()
        raise
    cat = lambda get: np.ascontiguousarray(np.concatenate([get(p) for p in parts], axis=0))  # noqa: E731
    planes = {k: cat(lambda p, k=k: p[4][k]) for k in AOV}
    planes["depth"], planes["direct"] = cat(lambda p: p[0]), cat(lambda p: p[3])
    return planes, parts[0][5]


class Run:
    def __init__(self, seed, modes=MODES, exr_dir=None, files_only=False, forms=EXR_COMPRESSIONS):
        self.ctx = ctx = Context(W, H)  # raises without a device
        self.scene = types.SimpleNamespace(frame=None)
        self.frames = {m: [] for m in MODES}
        exr = [m for m in modes if m in EXR_MODES]
        self.exr_bytes = {}
        self.forms = forms
        files = {(i, comp): os.path.join(exr_dir, "frame%d_%s.exr" % (0 if comp in PIZ_FORMS else i, comp)) for i in range(2) for comp in forms} if exr else {}
        if files_only:  # a kernel trace of E1 over files an earlier run left in --exr-dir: nothing is rendered, nothing is drawn
            for (i, comp), path in sorted(files.items()):
                self.exr_bytes.setdefault(comp, []).append(os.path.getsize(path))
                self.frames.setdefault("E1:" + comp, []).append(types.SimpleNamespace(path=path, exr="E1"))
            self.file_buffers = [ctx.host_alloc((max(max(v) for v in self.exr_bytes.values()),), np.uint8) for _ in range(2)]
            return

        def pin(a):  # a pinned copy: what makes the staged copies asynchronous
            p = ctx.host_alloc(a.shape, a.dtype)
            p[...] = a
            return p
        for i in range(2):
            planes, camera = render(seed, i)
            wide = {k: (v.astype(np.float16).astype(np.float32) if k in HALF else v) for k, v in planes.items()}
            typed = {k: (v.astype(np.float16) if k in HALF else v) for k, v in planes.items()}
            # the packed planes of the same values: the device's own importer
            ctx.pack_gbuffer(wide, wide["depth"])
            ctx.pack_velocity(wide, wide["depth"])
            gbuffer, velocity = ctx.download(abi.TEX_GBUFFER), ctx.download(abi.TEX_VELOCITY)
            ns = lambda static, depth, direct, **kw: types.SimpleNamespace(camera=camera, static=static, depth=depth, direct=direct, **kw)  # noqa: E731
            self.frames["P0"].append(ns("resident", pin(wide["depth"]), pin(wide["direct"]), gbuffer=pin(gbuffer), velocity=pin(velocity), aov=None))
            self.frames["A0"].append(ns(False, wide["depth"], wide["direct"], gbuffer=None, velocity=None, aov={k: wide[k] for k in AOV}))
            self.frames["A1"].append(ns("resident", pin(wide["depth"]), pin(wide["direct"]), gbuffer=None, velocity=None, aov={k: pin(wide[k]) for k in AOV}))
            self.frames["A2"].append(ns("resident", pin(typed["depth"]), pin(typed["direct"]), gbuffer=None, velocity=None, aov={k: pin(typed[k]) for k in AOV}))
            for comp in forms if exr else ():  # the typed frame as a file: one part per plane, halves where A2 sends halves
                path = files[(i, comp)]
                parts = {k: {cn.split(".")[1]: (typed[k][..., j] if typed[k].ndim == 3 else typed[k]) for j, cn in enumerate(imageio.AOV_LAYOUT[k])} for k in imageio.AOV_LAYOUT}
                slow = imageio._rle_compress
                if comp == "rle":
                    imageio._rle_compress = rle_compress_fast
                try:
                    if not (comp in PIZ_FORMS and os.path.exists(path)):  # (a PIZ file: minutes to write; frame 0's, once)
                        imageio.write_exr_multipart(path, parts, EXR_FORMS[comp][0], half=set(HALF), tiles=EXR_FORMS[comp][1])
                        print("wrote %s" % os.path.basename(path), file=sys.stderr, flush=True)
                finally:
                    imageio._rle_compress = slow
                self.exr_bytes.setdefault(comp, []).append(os.path.getsize(path))
                for m in EXR_MODES:
                    self.frames.setdefault(m + ":" + comp, []).append(ns("resident", None, None, gbuffer=None, velocity=None, aov=None, path=path, exr=m))
            print("frame %d ready" % i, file=sys.stderr, flush=True)
        if exr:  # E1's two pinned file buffers
            self.file_buffers = [ctx.host_alloc((max(max(v) for v in self.exr_bytes.values()),), np.uint8) for _ in range(2)]
        self.cam = types.SimpleNamespace(**vars(self.frames["P0"][0].camera))
        self.fx = effect.SSGIEffect(None, self.scene, self.cam, dict(width=W, height=H, steps=20, refineSteps=5), seeds=dict(ssgi=11, denoise=22), half_store_rtz=True)
        for m in ("A1", "A2"):
            f = self.frames[m][0]
            assert ctx.aov_stage_bytes(dict(f.aov, depth=f.depth, direct=f.direct)) == BYTES_PER_PIXEL[m] * W * H

    def draw(self, f):
        self.scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(self.cam, k, v)
        self.fx.update(self.ctx, None)

    def stage(self, f, k):
        """stage frame f, the k-th staged of its loop"""
        ctx = self.ctx
        if getattr(f, "exr", None) == "E0":
            t = imageio.exr_to_typed_planes(f.path)
            ctx.stage_aov(dict(t["aov"], depth=t["depth"], direct=t["direct"]))
        elif getattr(f, "exr", None) == "E1":
            buf, size = self.file_buffers[k & 1], os.path.getsize(f.path)
            with open(f.path, "rb", buffering=0) as fh:
                assert fh.readinto(memoryview(buf)[:size]) == size
            if self.forms == EXR_COMPRESSIONS:
                ctx.stage_exr_aov(buf, imageio.exr_aov_layout(buf[:size]))
            else:
                ctx.stage_exr_blocks(buf, imageio.exr_aov_layout(buf[:size], forms="blocks", piz=ctx.has_exr_piz))
        else:
            ctx.stage_frame(f)

    def loop(self, mode, n):
        """n frames; wall seconds, the device synchronised inside the clock"""
        ctx, fr = self.ctx, self.frames[mode]
        staged = mode != "A0"
        if staged:
            self.stage(fr[0], 0)
            ctx.stage_flip()
        ctx.sync()
        t0 = time.perf_counter()
        for i in range(n):
            if staged:
                self.stage(fr[(i + 1) & 1], i + 1)  # frame i + 1 crosses while frame i draws
            self.draw(fr[i & 1])
            if staged:
                ctx.stage_flip()
        ctx.sync()
        return time.perf_counter() - t0

    def kernel_only(self, n=20, modes=("A1", "A2")):
        """stage + flip alone, for a kernel trace: A1's frame, then A2's (or, --modes E1: the ZIPS file, then the ZIP file)"""
        ctx = self.ctx
        for mode in modes:
            for i in range(n):
                self.stage(self.frames[mode][i & 1], i)
                ctx.stage_flip()
            ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "import", "rates.json"))
    ap.add_argument("--seconds", type=float, default=1.0, help="steady state per measurement, at least")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--size", default="3840x2160", help="frame size (the committed numbers are 4K; a small size checks the script itself)")
    ap.add_argument("--kernel-only", action="store_true", help="only stage and flip AOV frames (under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--modes", default=",".join(MODES), help="P0,A0,A1,A2 (the default) or E0,E1 (the EXR file modes, measured beside A2)")
    ap.add_argument("--exr-dir", default=None, help="where the E modes write their files (default: a temporary directory)")
    ap.add_argument("--forms", default=None, help="with --modes E0,E1: tiled_zip,pxr24,rle,piz,tiled_piz (any of them) — the EXR blocks forms, measured beside E1's zip")
    ap.add_argument("--parent-lib", default=None, help="with --modes C2: a librfx_hip.so of the parent commit, measured beside this one in the same rounds")
    ap.add_argument("--e0-frames", type=int, default=2, help="--forms rle: the frames of one E0 loop (the host's RLE decode is a byte loop)")
    a = ap.parse_args()
    global W, H
    W, H = (int(v) for v in a.size.split("x"))
    modes = tuple(a.modes.split(","))
    if "C2" in modes:
        return main_conventions(a)
    if "D2" in modes or "D2p" in modes:
        return main_device(a)
    if any(m in EXR_MODES for m in modes):
        return main_exr_blocks(a, modes) if a.forms else main_exr(a, modes)
    run = Run(a.seed)
    if a.kernel_only:
        run.kernel_only()
        run.ctx.close()
        return
    result = dict(width=W, height=H, seed=a.seed, seconds=a.seconds, steps=20, refineSteps=5,
                  bytes_per_frame={m: BYTES_PER_PIXEL[m] * W * H for m in MODES}, rounds=[], frames={})
    n = {}
    for mode in MODES:  # warm every mode, and size its loop from the warm rate
        run.loop(mode, 5)
        per = run.loop(mode, 20) / 20
        n[mode] = max(20, int(math.ceil(a.seconds / per)))
    result["frames"] = n
    for r in range(3):
        row = {mode: round(run.loop(mode, n[mode]) / n[mode] * 1e3, 4) for mode in MODES}
        row["A1_below_A0"] = row["A1"] < row["A0"]
        row["A2_below_A0"] = row["A2"] < row["A0"]
        row["A2_over_P0"] = round(row["A2"] / row["P0"], 4)
        row["A1_over_P0"] = round(row["A1"] / row["P0"], 4)
        result["rounds"].append(row)
        print(json.dumps(row), flush=True)
    result["required_A1_and_A2_below_A0_every_round"] = all(r["A1_below_A0"] and r["A2_below_A0"] for r in result["rounds"])
    assert run.ctx.halo_violations() == 0
    run.ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not result["required_A1_and_A2_below_A0_every_round"]:
        sys.exit("import_rate: stage_aov is not faster than the synchronous importer in every round: the staging does not overlap")


def resident(v, layout, held):
    """a plane's (H, W[, C]) values in hipMalloc'ed memory (on the runtime the library itself uses) -> the abi.DevicePlane that addresses them;
    the layouts ("tight", "planar_top", "pitch4") and the runtime handle are the device-plane tests' own (tests/aov_device_cases.py)"""
    import ctypes as C
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import aov_device_cases as D
    flat, off, sx, sy, sc = D.lay(v, layout)
    p = C.c_void_p()
    assert D.hip().hipMalloc(C.byref(p), flat.nbytes) == 0 and p.value and p.value % 256 == 0
    held.append(p.value)
    assert D.hip().hipMemcpy(p, flat.ctypes.data, flat.nbytes, 1) == 0  # (host to device, complete on return)
    return abi.DevicePlane(p.value + off * v.dtype.itemsize, abi.PLANE_TYPES[v.dtype], 1 if v.ndim == 2 else v.shape[2], sx, sy, sc)


def device_plan_flat(f):
    """rfx_internal_aov_device_plan's `flat` for the whole frame of DevicePlane records f: 1 = k0_aov_pack serves it, 0 = the strided kernel"""
    import ctypes as C
    I, U, L = C.c_int, C.c_ulonglong, C.c_longlong

    class Seg(C.Structure):
        _fields_ = [(n, I) for n in ("row0", "rows", "full", "pixels", "groups", "blocks", "tail_start", "tail_pixels")] + [("offset", U * 8)]

    class Rows(C.Structure):
        _fields_ = [("nseg", I), ("seg", Seg * 3), ("plane_row0", I * 8), ("plane_rows", I * 8), ("elem_bytes", I * 8), ("write_gbuffer", I), ("write_velocity", I),
                    ("write_direct", I), ("copy_bytes", U), ("stage_bytes", U)]

    class Plan(C.Structure):
        _fields_ = [("rows", Rows), ("layout", I * 8), ("flat", I * 3), ("groups_x", I), ("tail_x", I), ("tail_pixels", I), ("lanes_x", I), ("grid_x", I), ("grid_y", I * 3),
                    ("seg_offset", (L * 8) * 3)]
    planes = [dict(f.aov, depth=f.depth, direct=f.direct)[k] for k in abi.AOV_PLANES]
    t = Plan()
    rc = abi.load_library().rfx_internal_aov_device_plan(
        C.c_int(W), C.c_int(H), C.c_int(0), C.c_int(H), (I * 8)(*[p.type for p in planes]), (I * 8)(*[p.channels for p in planes]), (U * 8)(*[p.data for p in planes]),
        (L * 8)(*[p.stride_x for p in planes]), (L * 8)(*[p.stride_y for p in planes]), (L * 8)(*[p.stride_c for p in planes]), C.c_int(0), C.c_int(H), C.c_int(0), C.c_int(0),
        C.byref(t))
    assert rc == 0 and t.rows.nseg == 1
    return t.flat[0], list(t.layout)


def main_device(a):
    """A2 beside D2 and D2p; merged into --out under "device_planes" """
    run = Run(a.seed)
    ctx = run.ctx
    assert ctx.has_stage_aov_device
    held = []
    layouts = dict(D2="tight", D2p="planar_top", D2i="pitch4")
    for mode, layout in layouts.items():
        run.frames[mode] = []
        for f in run.frames["A2"]:
            run.frames[mode].append(types.SimpleNamespace(camera=f.camera, static="resident", depth=resident(f.depth, layout, held), direct=resident(f.direct, layout, held),
                                                          gbuffer=None, velocity=None, aov={k: resident(v, layout, held) for k, v in f.aov.items()}))
    import aov_device_cases as D  # (on sys.path since resident())
    assert D.hip().hipDeviceSynchronize() == 0
    # D2 is the flat kernel on the caller's pointers; D2p is the strided kernel's PLANAR form, D2i its INTERLEAVED form, on every plane
    plans = {m: device_plan_flat(run.frames[m][0]) for m in layouts}
    multi = [i for i, k in enumerate(abi.AOV_PLANES) if k not in ("roughness", "metalness", "depth")]  # (a 1-channel plane with stride_x 1 is INTERLEAVED)
    assert plans["D2"][0] == 1 and plans["D2p"][0] == 0 and plans["D2i"] == (0, [1] * 8), plans
    assert all(plans["D2p"][1][i] == 2 for i in multi) and all(v in (1, 2) for v in plans["D2p"][1]), plans

    def release():
        ctx.close()
        for p in held:
            D.hip().hipFree(p)
    if a.kernel_only:  # under rocprofv3 --kernel-trace --stats: 20 x k0_aov_pack<1, false> on staged copies, 20 x the same on device planes, 20 + 20 x strided
        run.kernel_only(modes=("A2", "D2", "D2p", "D2i"))
        release()
        return
    order = ["A2", "D2", "D2p"]
    n = {}
    for m in order:
        run.loop(m, 5)
        n[m] = max(20, int(math.ceil(a.seconds / (run.loop(m, 20) / 20))))
    out = dict(width=W, height=H, seed=a.seed, seconds=a.seconds, steps=20, refineSteps=5, bytes_per_frame=BYTES_PER_PIXEL["A2"] * W * H, frames=n, rounds=[], stage_only=[])
    for r in range(3):  # (the order rotates: no mode is always the first or the last of its round)
        row = {m: round(run.loop(m, n[m]) / n[m] * 1e3, 4) for m in order[r:] + order[:r]}
        row = {m: row[m] for m in order}
        row["D2_below_A2"], row["D2p_below_A2"] = row["D2"] < row["A2"], row["D2p"] < row["A2"]
        out["rounds"].append(row)
        print(json.dumps(row), flush=True)

    def stage_only(m, k=40):
        ctx.sync()
        t0 = time.perf_counter()
        for i in range(k):
            run.stage(run.frames[m][i & 1], i)
            ctx.stage_flip()
        ctx.sync()
        return (time.perf_counter() - t0) / k
    for r in range(3):
        row = {m: round(stage_only(m) * 1e3, 4) for m in order + ["D2i"]}
        out["stage_only"].append(row)
        print("stage_only", json.dumps(row), flush=True)
    out["required_D2_and_D2p_below_A2_every_round"] = ok = all(r["D2_below_A2"] and r["D2p_below_A2"] for r in out["rounds"])
    assert ctx.halo_violations() == 0
    release()
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result["device_planes"] = out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not ok:
        sys.exit("import_rate: staging from device planes is not faster than the PCIe copy in every round")


def _engine_band(args):
    seed, index, row0, rows = args
    f = AnalyticScene(seed).render(W, rows, index, row0=row0, rows=rows, frame_height=H, aov=True, engine=True)
    return f.engine["position"], f.engine["view_normal"], f.camera, f.prev_camera


def main_conventions(a):
    """A2 beside C2 (and A2 on --parent-lib); merged into --out under "conventions" """
    import multiprocessing as mp
    from rfx_amd.conventions import AovConventions
    run = Run(a.seed)
    ctx = run.ctx
    assert ctx.has_aov_conventions
    edges = [H * i // 16 for i in range(17)]
    frames, convs = [], []
    for i in range(2):
        pool = mp.get_context("fork").Pool(16, initializer=_pool_worker_init)
        try:
            parts = pool.map(_engine_band, [(a.seed, i, edges[k], edges[k + 1] - edges[k]) for k in range(16)])
            pool.close()
            pool.join()
        except BaseException:
            pool.terminate()
            raise
        a2 = run.frames["A2"][i]
        planes = {k: v for k, v in a2.aov.items() if k not in ("velocity", "normal")}
        for k, j, dt in (("position", 0, np.float32), ("normal", 1, np.float16)):
            src = np.concatenate([p[j] for p in parts], axis=0).astype(dt)
            planes[k] = ctx.host_alloc(src.shape, dt)
            planes[k][...] = src
        planes["direct"] = a2.direct
        frames.append(planes)
        convs.append(AovConventions.from_cameras(parts[0][2], parts[0][3], depth_kind="position", velocity_kind="cameras", normal_space="view", background_position=(0.0, 0.0, 0.0)))
    assert ctx.set_aov_conventions(convs[0]) is None and ctx.aov_stage_bytes(frames[0]) == BYTES_PER_PIXEL["A2"] * W * H
    ctx.set_aov_conventions(None)
    runs = {"A2": (ctx, run.fx, run.cam, run.scene)}
    if a.parent_lib:
        abi.set_library_path(a.parent_lib)
        pctx = Context(W, H)
        abi.set_library_path(None)
        assert not pctx.has_aov_conventions, "--parent-lib already has rfx_set_aov_conventions: not the parent"
        pscene = types.SimpleNamespace(frame=None)
        pcam = types.SimpleNamespace(**vars(run.cam))
        pfx = effect.SSGIEffect(None, pscene, pcam, dict(width=W, height=H, steps=20, refineSteps=5), seeds=dict(ssgi=11, denoise=22), half_store_rtz=True)
        runs["A2_parent"] = (pctx, pfx, pcam, pscene)
    runs["C2"] = runs["A2"]

    def stage(c, mode, i):
        if mode == "C2":
            c.set_aov_conventions(convs[i & 1])
            c.stage_aov(frames[i & 1])
        else:
            c.stage_frame(run.frames["A2"][i & 1])

    def loop(mode, n, draw=True):
        c, fx, cam, scene = runs[mode]
        if mode != "A2_parent":
            c.set_aov_conventions(None)
        stage(c, mode, 0)
        c.stage_flip()
        c.sync()
        t0 = time.perf_counter()
        for i in range(n):
            stage(c, mode, i + 1)
            if draw:
                f = run.frames["A2"][i & 1]
                scene.frame = f
                for k, v in vars(f.camera).items():
                    setattr(cam, k, v)
                fx.update(c, None)
            c.stage_flip()
        c.sync()
        return time.perf_counter() - t0

    order = [m for m in ("A2_parent", "A2", "C2") if m in runs]
    if a.kernel_only:  # under rocprofv3 --kernel-trace --stats: the pack kernel's default and converting instantiations, stage + flip alone
        for m in ("A2", "C2"):
            loop(m, 20, draw=False)
        ctx.close()
        return
    n = {}
    for m in order:
        loop(m, 5)
        n[m] = max(20, int(math.ceil(a.seconds / (loop(m, 20) / 20))))
    out = dict(width=W, height=H, seed=a.seed, seconds=a.seconds, bytes_per_frame=BYTES_PER_PIXEL["A2"] * W * H, kinds="position + cameras + view", frames=n, rounds=[], stage_only=[])
    for r in range(3):  # (the order rotates: no mode is always the first or the last of its round)
        row = {m: round(loop(m, n[m]) / n[m] * 1e3, 4) for m in order[r % len(order):] + order[:r % len(order)]}
        row = {m: row[m] for m in order}
        out["rounds"].append(row)
        print(json.dumps(row), flush=True)
    for r in range(3):
        row = {m: round(loop(m, 40, draw=False) / 40 * 1e3, 4) for m in order}
        out["stage_only"].append(row)
        print("stage_only", json.dumps(row), flush=True)
    base = "A2_parent" if "A2_parent" in runs else "A2"
    vals = [r[base] for r in out["rounds"]]
    out["baseline"], out["baseline_spread_ms"] = base, round(max(vals) - min(vals), 4)
    out["C2_minus_baseline_ms"] = [round(r["C2"] - r[base], 4) for r in out["rounds"]]
    for c, *_ in {id(v[0]): v for v in runs.values()}.values():
        assert c.halo_violations() == 0
        c.close()
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result["conventions"] = out
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def main_exr(a, modes):
    """E0 / E1 beside A2, per compression; merged into --out under "exr" """
    assert set(modes) <= set(EXR_MODES), "the EXR modes are measured on their own (with A2 beside them)"
    tmp = None if a.exr_dir else tempfile.TemporaryDirectory()
    have = a.exr_dir and all(os.path.exists(os.path.join(a.exr_dir, "frame%d_%s.exr" % (i, c))) for i in range(2) for c in EXR_COMPRESSIONS)
    run = Run(a.seed, modes, a.exr_dir or tmp.name, files_only=bool(a.kernel_only and have))
    if a.kernel_only:
        run.kernel_only(n=10, modes=["E1:" + c for c in EXR_COMPRESSIONS])
        run.ctx.close()
        return
    out = dict(width=W, height=H, seed=a.seed, seconds=a.seconds, compressions={})
    ok = True
    for comp in EXR_COMPRESSIONS:
        names = ["A2"] + [m + ":" + comp for m in modes]
        n = {}
        for mode in names:  # warm every mode, and size its loop from the warm rate (E0 takes seconds per frame: two frames are a loop)
            run.loop(mode, 2)
            per = run.loop(mode, 2) / 2
            n[mode] = max(2 if per > 0.25 else 20, int(math.ceil(a.seconds / per)))
        size = run.exr_bytes[comp][0]
        row0 = dict(file_bytes=run.exr_bytes[comp], file_bytes_per_pixel=round(size / (W * H), 3), ratio_to_typed_planes=round(size / (BYTES_PER_PIXEL["A2"] * W * H), 4),
                    staged_bytes=run.ctx.exr_aov_stage_bytes(*run_file(run, comp)), frames=n, rounds=[])
        for r in range(3):
            row = {mode.split(":")[0]: round(run.loop(mode, n[mode]) / n[mode] * 1e3, 4) for mode in names}
            if "E0" in row and "E1" in row:
                row["E1_below_E0"] = row["E1"] < row["E0"]
                ok = ok and row["E1_below_E0"]
            if "E1" in row:
                row["E1_over_A2"] = round(row["E1"] / row["A2"], 4)
            row0["rounds"].append(row)
            print(comp, json.dumps(row), flush=True)
        assert run.ctx.exr_aov_status()[0] == 0
        out["compressions"][comp] = row0
    out["required_E1_below_E0_every_round"] = ok
    run.ctx.close()
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result["exr"] = out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not ok:
        sys.exit("import_rate: the device decode is not faster than the host decode in every round")


def main_exr_blocks(a, modes):
    """E0 / E1 per --forms form, E1 of the ZIP scanline file beside them (all through stage_exr_blocks); merged into --out under "exr_blocks", or
    under "exr_piz" when a PIZ form is among them"""
    assert set(modes) <= set(EXR_MODES)
    forms = tuple(a.forms.split(","))
    assert forms and set(forms) <= set(BLOCK_FORMS), "--forms: any of " + ",".join(BLOCK_FORMS)
    tmp = None if a.exr_dir else tempfile.TemporaryDirectory()
    run = Run(a.seed, modes, a.exr_dir or tmp.name, forms=("zip",) + forms)
    out = dict(width=W, height=H, seed=a.seed, seconds=a.seconds, tiles=list(EXR_FORMS["tiled_zip"][1]), forms={})
    for form in ("zip",) + forms:
        names = [m + ":" + form for m in modes if not (m == "E0" and (form == "zip" or form in PIZ_FORMS))]
        n = {}
        for mode in names:
            if mode == "E0:rle":
                n[mode] = a.e0_frames
                continue
            run.loop(mode, 2)
            per = run.loop(mode, 2) / 2
            n[mode] = max(2 if per > 0.25 else 20, int(math.ceil(a.seconds / per)))
        size = run.exr_bytes[form][0]
        data = open(run.frames["E1:" + form][0].path, "rb").read()
        lay = imageio.exr_aov_layout(data, forms="blocks", piz=form in PIZ_FORMS)
        row0 = dict(file_bytes=run.exr_bytes[form], file_bytes_per_pixel=round(size / (W * H), 3), blocks=len(lay.blocks),
                    raw_blocks=int((lay.blocks["packed_bytes"] == block_raw_sizes(lay)).sum()), staged_bytes=run.ctx.exr_blocks_stage_bytes(data, lay), frames=n, rounds=[])
        if form in PIZ_FORMS:
            row0.update(piz_host_band(data, lay))
            row0.update(fast_bits=PIZ_FAST_BITS, wave_lds_bytes=PIZ_WAVE_LDS, waves_per_cu=CU_LDS // PIZ_WAVE_LDS,
                        table_scratch_bytes=(len(lay.blocks) - row0["raw_blocks"]) * PIZ_TABLE_BYTES)
        for r in range(1 if form == "rle" else 3):
            row = {mode.split(":")[0]: round(run.loop(mode, n[mode]) / n[mode] * 1e3, 4) for mode in names}
            if "E0" in row and "E1" in row:
                row["E0_over_E1"] = round(row["E0"] / row["E1"], 2)
            if "E0_band_scaled" in row0 and "E1" in row:
                row["E0_band_scaled_over_E1"] = round(row0["E0_band_scaled"] / row["E1"], 2)
            row0["rounds"].append(row)
            print(form, json.dumps(row), flush=True)
        assert run.ctx.exr_aov_status()[0] == 0
        out["forms"][form] = row0
    zip_e1 = min(r["E1"] for r in out["forms"]["zip"]["rounds"])
    for form in forms:
        out["forms"][form]["E1_over_E1_zip"] = round(min(r["E1"] for r in out["forms"][form]["rounds"]) / zip_e1, 4)
    run.ctx.close()
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result["exr_piz" if set(forms) & set(PIZ_FORMS) else "exr_blocks"] = out  # (a PIZ run is a run of its own: it does not replace the 4K figures)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def piz_host_band(data, lay):
    """the host's PIZ decode of the file's first block row — the blocks with y = 0 of every part —, in ms, and that scaled to the frame's rows"""
    first = [b for b in lay.blocks if int(b["y"]) == 0]
    rows = int(first[0]["rows"])
    assert all(int(b["rows"]) == rows for b in first)
    t0 = time.perf_counter()
    for b in first:
        chans = [(None, pt) for pt, _, _ in lay.parts[int(b["part"])][1]]
        raw = int(b["rows"]) * int(b["cols"]) * sum(2 if pt == 1 else 4 for _, pt in chans)
        imageio._exr_unpack_block(data[int(b["offset"]):int(b["offset"] + b["packed_bytes"])], imageio._COMP_PIZ, chans, int(b["cols"]), int(b["rows"]), raw)
    ms = (time.perf_counter() - t0) * 1e3
    return dict(E0_band_rows=rows, E0_band_blocks=len(first), E0_band_ms=round(ms, 1), E0_band_scaled=round(ms * H / rows, 1))


def block_raw_sizes(lay):
    texel = np.array([sum(2 if pt == 1 else 4 for pt, _, _ in chans) for _, chans in lay.parts])
    b = lay.blocks
    return b["rows"].astype(np.int64) * b["cols"] * texel[b["part"]]


def run_file(run, comp):
    """(the bytes of frame 0's file of this compression, its layout)"""
    data = open(run.frames["E1:" + comp][0].path, "rb").read()
    return data, imageio.exr_aov_layout(data)


if __name__ == "__main__":
    main()
