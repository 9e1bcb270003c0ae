#!/usr/bin/env python3
"""What per-frame output costs at 4K (GPU box; fails without a device): wall time per frame of the SSGI chain + the effect's own fragment with

    T0  no per-frame output
    T1  a blocking download(TEX_FINAL) every frame — RGBA32F, 133 MB, into a pinned buffer: the most a host could do before the export
    T2  stage_export U8_SRGB x 3 every frame into two alternating pinned buffers, export_wait one frame late (rfx_amd/frames.py's order)
    T2h T2, and the waited frame goes through the host's imageio.write_png (zlib level 6, one thread) to /dev/null: FrameExporter(encode="host")
    T3  stage_png (K8: the frame leaves the device as a PNG fragment), waited one frame late, wrapped by imageio.png_from_fragments and written
        to /dev/null: FrameExporter(encode="device")

each with the dump resident on the device and streamed (rfx_stage_upload / rfx_stage_flip from two pinned sets), in ONE process: every shape is
warmed first, then three alternating rounds of the three modes, each a steady state of at least --seconds with a device synchronise at the end.
(T2h takes seconds per frame at 4K: its loops are a few frames long.)  K7's and K8's own times come from rfx_profile, next to the bytes they
read and write; the fragment's size per frame is recorded with K8's.

    python tools/export_rate.py [--out profiles/export/rates.json] [--seconds 1.0]

--modes exr measures the HDR output instead, by the same protocol (T0 and the three modes below in alternating rounds), and ADDS its results to
--out under the key "exr" (the entries above stay):

    E1  stage_export F16 x 4, waited one frame late, written by the host's imageio.write_exr(compression="none", half=True) to /dev/null:
        FrameExporter("exr")
    E2  E1 with write_exr(compression="zips"): the host's own ZIPS writer (numpy + zlib level 4, one thread), a few frames
    E3  stage_exr (K8 behind the EXR predictor: the frame leaves the device as ZIPS chunks), waited one frame late, wrapped by
        imageio.exr_from_fragments and written to /dev/null: FrameExporter("exr", compression="zips")

and the EXR encode alone (rfx_profile, kind K8) next to the PNG encode measured in the same process.

--modes matches measures the device encode with run-length matches (rfx.h "Match form") against the one without, by the same protocol (T0, T3,
E3 and the two modes below in alternating rounds), and ADDS its results to --out under the key "matches":

    T3m  T3 with stage_png(matches=True)
    E3m  E3 with stage_exr(matches=True)

and the encode alone (rfx_profile, kind K8) for PNG and EXR with matches off and on, three alternating rounds of 20 launches each, so that the
spread from round to round stands next to the difference; the fragment bytes of the same frame off and on, and that frame through the host's
ZIPS writer.

--modes device measures the export that stays on the device (rfx.h "device images"), without the SSGI chain — a context with a 4K frame in
RFX_TEX_EFFECT_INPUT, images in hipMalloc'ed memory — and ADDS its results to --out under the key "device":

    kernels   for each of the eight K7 specialisations, the K7 time (rfx_profile, kind K7) of rfx_stage_export (the flat kernel into the staging
              buffer) and of rfx_export_device in its four forms — tight (the flat kernel on the caller's pointer), interleaved (rows padded to a
              multiple of four elements and four more), planar ((C, H, W) with padded rows and planes), element (a mirrored x) — in three
              alternating rounds of 20 launches each of the SAME run; per form the median, its ratio to the flat kernel's median, and the flat
              kernel's own spread between rounds to hold the difference against
    handover  the whole cost per frame of getting a frame to a consumer's stream, F16 x 4 and U8 x 3 ACES: D1, export_device(stream=) and
              the consumer's device-to-device copy of the image; H1, stage_export into pinned memory, export_wait, hipMemcpyAsync back up on
              the consumer's stream, the same device-to-device copy; three alternating rounds, the consumer's stream synchronised inside the clock

--modes matches --parent-lib PATH (a librfx_hip.so built from the parent commit) measures only those encodes alone, on that library and on
this tree's in alternating fresh processes of one session (--processes of each), and ADDS them to --out under --key with, per encode, the
parent's median and full range, the tree's median, and whether the tree's median is within the parent's median plus that range.
"""
import argparse
import copy
import ctypes as C
import json
import math
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))

from rfx_amd import abi, effect, imageio  # noqa: E402
from rfx_amd.context import Context  # noqa: E402
from rfx_amd.scene import synthetic_frame_parallel  # noqa: E402

W, H = 3840, 2160
HBM_PEAK = 8e12  # bytes / s
MODES = ("T0", "T1", "T2", "T2h", "T3")
EXR_MODES = ("T0", "E1", "E2", "E3")
MATCH_MODES = ("T0", "T3", "T3m", "E3", "E3m")
WARM = {"T2h": (1, 2), "E1": (1, 3), "E2": (1, 2)}   # frames of the two warming loops (default 5 and 20)
MIN_FRAMES = {"T2h": 3, "E1": 5, "E2": 3}            # ... and the fewest of a measured loop (default 20)


class Run:
    def __init__(self, seed):
        self.ctx = Context(W, H)  # raises without a device
        self.frames = [synthetic_frame_parallel(W, H, i, seed=seed, workers=16) for i in range(2)]
        self.scene = types.SimpleNamespace(frame=None)
        self.cam = types.SimpleNamespace(**vars(self.frames[0].camera))
        self.fx = effect.SSGIEffect(None, self.scene, self.cam, dict(width=W, height=H), seeds=dict(ssgi=11, denoise=22), half_store_rtz=True)
        ctx = self.ctx
        self.sets = []
        for f in self.frames:  # two pinned sets of the four planes: what a streamed run alternates between
            s = copy.copy(f)
            for k in ("depth", "gbuffer", "velocity", "direct"):
                p = ctx.host_alloc(getattr(f, k).shape, getattr(f, k).dtype)
                p[...] = getattr(f, k)
                setattr(s, k, p)
            s.static = "resident"  # the effect does not upload it again: it is staged, or already there
            self.sets.append(s)
        self.final = ctx.host_alloc((H, W, 4), np.float32)
        self.u8 = [ctx.host_alloc((H, W, 3), np.uint8) for _ in range(2)]
        self.png = [ctx.host_alloc((ctx.png_bound(3),), np.uint8) for _ in range(2)]
        self.fragment_bytes = []
        self.f16, self.exr, self.exr_file_bytes = None, None, []
        self.match_file_bytes = {}

    def alloc_exr(self):
        self.f16 = [self.ctx.host_alloc((H, W, 4), np.float16) for _ in range(2)]
        self.exr = [self.ctx.host_alloc((self.ctx.exr_bound(4),), np.uint8) for _ in range(2)]

    def write(self, mode, buf):
        """what the host does with a waited frame"""
        if mode == "T2h":
            imageio.write_png(os.devnull, buf)
        elif mode in ("T3", "T3m"):
            data = imageio.png_from_fragments(W, H, 3, [buf])
            (self.fragment_bytes if mode == "T3" else self.match_file_bytes.setdefault(mode, [])).append(len(data))
            with open(os.devnull, "wb") as f:
                f.write(data)
        elif mode in ("E1", "E2"):
            imageio.write_exr(os.devnull, {n: buf[..., k] for k, n in enumerate("RGBA")}, compression="none" if mode == "E1" else "zips", half=True)
        elif mode in ("E3", "E3m"):
            data = imageio.exr_from_fragments(W, H, 4, [buf])
            (self.exr_file_bytes if mode == "E3" else self.match_file_bytes.setdefault(mode, [])).append(len(data))
            with open(os.devnull, "wb") as f:
                f.write(data)

    def frame(self, f):
        self.scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(self.cam, k, v)
        self.fx.update(self.ctx, None)
        self.fx.mainImage(self.ctx)

    def loop(self, mode, streamed, n):
        """n frames; returns wall seconds, the last export waited for and the device synchronised inside the clock"""
        ctx, sets = self.ctx, self.sets
        pending = None
        if streamed:
            ctx.stage_frame(sets[0])
            ctx.stage_flip()
        else:
            ctx.upload_frame(self.frames[0])
        ctx.sync()
        t0 = time.perf_counter()
        for i in range(n):
            cur = sets[i & 1] if streamed else sets[0]
            if streamed:
                ctx.stage_frame(sets[(i + 1) & 1])
            self.frame(cur)
            if mode == "T1":
                ctx._chk(ctx.lib.rfx_download(ctx._h, abi.TEX_FINAL, self.final.ctypes.data_as(C.c_void_p), 0, H), "rfx_download")
            elif mode in ("T2", "T2h", "T3", "T3m", "E1", "E2", "E3", "E3m"):
                if mode in ("E3", "E3m"):
                    buf = self.exr[i & 1]
                    t = ctx.stage_exr(abi.TEX_FINAL, 4, out=buf, matches=mode == "E3m")
                elif mode in ("E1", "E2"):
                    buf = self.f16[i & 1]
                    t = ctx.stage_export(abi.TEX_FINAL, "f16", 4, out=buf)
                elif mode in ("T3", "T3m"):
                    buf = self.png[i & 1]
                    t = ctx.stage_png(abi.TEX_FINAL, 3, "aces", 1.0, out=buf, matches=mode == "T3m")
                else:
                    buf = self.u8[i & 1]
                    t = ctx.stage_export(abi.TEX_FINAL, "u8_srgb", 3, "aces", 1.0, out=buf)
                if pending is not None:
                    ctx.export_wait(pending[0])
                    self.write(mode, pending[1])
                pending = (t, buf)
            if streamed:
                ctx.stage_flip()
        if pending is not None:
            ctx.export_wait(pending[0])
            self.write(mode, pending[1])
        ctx.sync()
        return time.perf_counter() - t0


def main_exr(run, a):
    """--modes exr: T0 / E1 / E2 / E3 and the EXR encode alone, merged into the file under the key "exr" """
    import struct
    import tempfile
    run.alloc_exr()
    ctx = run.ctx
    result = dict(width=W, height=H, seed=a.seed, seconds=a.seconds, rounds={}, frames={})
    for streamed in (False, True):
        key = "streamed" if streamed else "resident"
        n = {}
        for mode in EXR_MODES:
            w0, w1 = WARM.get(mode, (5, 20))
            run.loop(mode, streamed, w0)
            per = run.loop(mode, streamed, w1) / w1
            n[mode] = max(MIN_FRAMES.get(mode, 20), int(math.ceil(a.seconds / per)))
        rounds = []
        for r in range(3):
            row = {}
            for mode in EXR_MODES:
                row[mode] = round(run.loop(mode, streamed, n[mode]) / n[mode] * 1e3, 4)
            row["E3_minus_T0"] = round(row["E3"] - row["T0"], 4)
            row["E3_minus_E1"] = round(row["E3"] - row["E1"], 4)
            row["E3_below_E2"] = row["E3"] < row["E2"]
            rounds.append(row)
            print(key, json.dumps(row), flush=True)
        result["rounds"][key] = rounds
        result["frames"][key] = n
    result["E3_below_E2_every_round"] = all(r["E3_below_E2"] for rs in result["rounds"].values() for r in rs)
    # the EXR encode alone (its four launches on the download stream), inside a loop of staged fragments; then the PNG encode the same way
    for _ in range(5):
        ctx.export_wait(ctx.stage_exr(abi.TEX_FINAL, 4, out=run.exr[0]))
    ctx.sync()
    ctx.profile(True)
    for i in range(20):
        ctx.export_wait(ctx.stage_exr(abi.TEX_FINAL, 4, out=run.exr[i & 1]))
    prof = ctx.profile_read()
    ctx.profile(False)
    ms, launches = prof["k8_png"]
    k7ms, k7n = prof["k7_export"]
    fragment, chunks, _, raw, raw_chunks, _ = struct.unpack("<QIIQII", run.exr[1][:32].tobytes())
    result["k8_exr_f16x4"] = dict(ms=round(ms / launches, 5), launches=launches, bytes_read=raw, bytes_written=fragment, fragment_of_raw=round(fragment / raw, 4),
                                  raw_form_chunks=raw_chunks, chunks=chunks, bound=int(ctx.exr_bound(4)), mb_per_ms=round(raw / 1e6 / (ms / launches), 2),
                                  pcie_bytes_a_fragment_only_copy_would_save=int(ctx.exr_bound(4)) - 32 - fragment)
    result["k7_f16x4"] = dict(ms=round(k7ms / k7n, 5), launches=k7n)
    print(json.dumps(result["k8_exr_f16x4"]), flush=True)
    for _ in range(5):
        ctx.export_wait(ctx.stage_png(abi.TEX_FINAL, 3, "aces", 1.0, out=run.png[0]))
    ctx.sync()
    ctx.profile(True)
    for i in range(20):
        ctx.export_wait(ctx.stage_png(abi.TEX_FINAL, 3, "aces", 1.0, out=run.png[i & 1]))
    ms, launches = ctx.profile_read()["k8_png"]
    ctx.profile(False)
    result["k8_png_u8x3_same_process"] = dict(ms=round(ms / launches, 5), launches=launches, bytes_read=W * H * 3, mb_per_ms=round(W * H * 3 / 1e6 / (ms / launches), 2))
    print(json.dumps(result["k8_png_u8x3_same_process"]), flush=True)
    # file bytes over raw: the frames E3 wrote, and one frame through both writers (outside every clock)
    halfs = ctx.export(abi.TEX_FINAL, "f16", 4)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "host_zips.exr")
        imageio.write_exr(path, {n: halfs[..., k] for k, n in enumerate("RGBA")}, compression="zips", half=True)
        host_bytes = os.path.getsize(path)
    device_bytes = len(imageio.exr_from_fragments(W, H, 4, [ctx.exr(abi.TEX_FINAL, 4)]))
    raw_frame = W * H * 8
    fb = run.exr_file_bytes
    result["file_bytes"] = dict(raw=raw_frame, E3_min=min(fb), E3_max=max(fb), E3_frames=len(fb), E3_min_of_raw=round(min(fb) / raw_frame, 4),
                                E3_max_of_raw=round(max(fb) / raw_frame, 4), same_frame_device=device_bytes, same_frame_host_zips_level4=host_bytes)
    print(json.dumps(result["file_bytes"]), flush=True)
    ctx.close()
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged["exr"] = result
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")


def encodes_alone(run):
    """the K8 encodes alone (rfx_profile) inside loops of staged fragments of ONE frame, PNG U8 x 3 and EXR F16 x 4 with matches off and on:
    the four alternate, three rounds of 20 launches each, so the spread is on record.  {"png_off": [ms per launch of each round], ...}"""
    ctx = run.ctx

    def stage(kind, matches, buf):
        if kind == "png":
            return ctx.stage_png(abi.TEX_FINAL, 3, "aces", 1.0, out=buf, matches=matches)
        return ctx.stage_exr(abi.TEX_FINAL, 4, out=buf, matches=matches)

    alone = {}
    for kind, bufs in (("png", run.png), ("exr", run.exr)):
        for matches in (False, True):
            for _ in range(5):
                ctx.export_wait(stage(kind, matches, bufs[0]))
    for r in range(3):
        for kind, bufs in (("png", run.png), ("exr", run.exr)):
            for matches in (False, True):
                ctx.sync()
                ctx.profile(True)
                for i in range(20):
                    ctx.export_wait(stage(kind, matches, bufs[i & 1]))
                ms, launches = ctx.profile_read()["k8_png"]
                ctx.profile(False)
                alone.setdefault("%s_%s" % (kind, "on" if matches else "off"), []).append(round(ms / launches, 5))
    return alone


def main_parent_against_tree(a):
    """--modes matches --parent-lib PATH: the encodes alone on the parent commit's library and on this tree's, in alternating fresh processes
    (--processes of each, this one opens no device), merged into the file under --key.  within: the tree's median is at most the parent's
    median plus the parent's own full range over all its rounds and processes."""
    import statistics
    import subprocess
    runs = {"parent": [], "tree": []}
    for p in range(a.processes):
        for name in ("parent", "tree"):
            cmd = [sys.executable, os.path.abspath(__file__), "--modes", "matches", "--encodes-only", "--size", a.size, "--seed", str(a.seed)]
            if name == "parent":
                cmd += ["--lib", a.parent_lib]
            out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout  # a failed or hung process ends the session
            runs[name].append(json.loads(out.strip().splitlines()[-1]))
            print(name, p, json.dumps(runs[name][-1]), flush=True)
    result = dict(what="the K8 encodes alone, the parent commit's library and this tree's in alternating processes of one session, three rounds "
                       "of 20 launches each, ms", width=W, height=H, seed=a.seed, parent=runs["parent"], tree=runs["tree"], summary={})
    for k in runs["parent"][0]:
        pv = [v for r in runs["parent"] for v in r[k]]
        tv = [v for r in runs["tree"] for v in r[k]]
        pm, tm, rng = statistics.median(pv), statistics.median(tv), max(pv) - min(pv)
        result["summary"][k] = dict(parent_median=round(pm, 5), parent_range=round(rng, 5), tree_median=round(tm, 5), within=bool(tm <= pm + rng))
    print(json.dumps(result["summary"]), flush=True)
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged[a.key] = result
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")


def main_matches(run, a):
    """--modes matches: T0 / T3 / T3m / E3 / E3m and the two encodes alone with matches off and on, merged into the file under the key "matches" """
    import struct
    import tempfile
    run.alloc_exr()
    ctx = run.ctx
    result = dict(width=W, height=H, seed=a.seed, seconds=a.seconds, rounds={}, frames={})
    for streamed in (False, True):
        key = "streamed" if streamed else "resident"
        n = {}
        for mode in MATCH_MODES:
            run.loop(mode, streamed, 5)
            per = run.loop(mode, streamed, 20) / 20
            n[mode] = max(20, int(math.ceil(a.seconds / per)))
        rounds = []
        for r in range(3):
            row = {}
            for mode in MATCH_MODES:
                row[mode] = round(run.loop(mode, streamed, n[mode]) / n[mode] * 1e3, 4)
            row["T3m_minus_T3"] = round(row["T3m"] - row["T3"], 4)
            row["E3m_minus_E3"] = round(row["E3m"] - row["E3"], 4)
            rounds.append(row)
            print(key, json.dumps(row), flush=True)
        result["rounds"][key] = rounds
        result["frames"][key] = n
    for k, v in encodes_alone(run).items():
        result["k8_" + k] = dict(ms_rounds=v, ms=round(sorted(v)[1], 5), spread=round(max(v) - min(v), 5), launches_per_round=20)
    print(json.dumps({k: v for k, v in result.items() if k.startswith("k8_")}), flush=True)
    # the fragments of that frame, off and on; the same frame through the host's ZIPS writer (outside every clock)
    sizes = {}
    for matches in (False, True):
        head = struct.unpack("<QIIQII", ctx.png(abi.TEX_FINAL, 3, "aces", 1.0, matches=matches)[:32].tobytes())
        sizes["png_on" if matches else "png_off"] = dict(fragment=head[0], raw=head[3], fragment_of_raw=round(head[0] / head[3], 4), match_form_chunks=head[4], chunks=H)
        head = struct.unpack("<QIIQII", ctx.exr(abi.TEX_FINAL, 4, matches=matches)[:32].tobytes())
        sizes["exr_on" if matches else "exr_off"] = dict(fragment=head[0], raw=head[3], fragment_of_raw=round(head[0] / head[3], 4), raw_form_chunks=head[4],
                                                         match_form_chunks=head[5], chunks=head[1])
    halfs = ctx.export(abi.TEX_FINAL, "f16", 4)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "host_zips.exr")
        imageio.write_exr(path, {n: halfs[..., k] for k, n in enumerate("RGBA")}, compression="zips", half=True)
        sizes["exr_same_frame_host_zips_level4_file"] = os.path.getsize(path)
    result["same_frame"] = sizes
    result["file_bytes_per_frame"] = {m: dict(min=min(v), max=max(v), frames=len(v)) for m, v in run.match_file_bytes.items()}
    result["file_bytes_per_frame"]["T3"] = dict(min=min(run.fragment_bytes), max=max(run.fragment_bytes), frames=len(run.fragment_bytes))
    result["file_bytes_per_frame"]["E3"] = dict(min=min(run.exr_file_bytes), max=max(run.exr_file_bytes), frames=len(run.exr_file_bytes))
    print(json.dumps(result["same_frame"]), flush=True)
    print(json.dumps(result["file_bytes_per_frame"]), flush=True)
    ctx.close()
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged["matches"] = result
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")


DEVICE_SPECS = (("f32", 3, "linear", 1.0), ("f32", 4, "linear", 1.0), ("f16", 3, "linear", 1.0), ("f16", 4, "linear", 1.0),
                ("u8_srgb", 3, "linear", 1.0), ("u8_srgb", 4, "linear", 1.0), ("u8_srgb", 3, "aces", 1.0), ("u8_srgb", 4, "aces", 1.0))
DEVICE_FORMS = ("tight", "interleaved", "planar", "element")


def device_image_of(form, base, ch, elem):
    """-> (abi.DeviceImage over the buffer at `base`, the bytes it spans) for a whole frame in one of the four store forms"""
    if form == "tight":
        return abi.DeviceImage(base, ch, W * ch, 1), W * H * ch * elem
    if form == "interleaved":
        pitch = W * ch + (-W * ch) % 4 + 4
        return abi.DeviceImage(base, ch, pitch, 1), H * pitch * elem
    if form == "planar":
        wp = W + (-W) % 4 + 4
        plane = H * wp + 8
        return abi.DeviceImage(base, 1, wp, plane), ch * plane * elem
    return abi.DeviceImage(base + (W - 1) * ch * elem, -ch, W * ch, 1), W * H * ch * elem  # element: x mirrored


def main_device(a):
    """--modes device: K7 per specialisation and store form next to the flat K7 of the same run, and the hand-over to a consumer's stream;
    merged into the file under the key "device" """
    import statistics
    ctx = Context(W, H)  # raises without a device
    if not ctx.has_export_device:
        raise SystemExit("this librfx_hip.so has no rfx_export_device")
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    hip = C.CDLL(paths[0])  # the runtime the library runs on
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rng = np.random.default_rng(a.seed)
    ctx.upload(abi.TEX_EFFECT_INPUT, rng.lognormal(-1.0, 1.5, (H, W, 4)).astype(np.float32))
    wp = W + (-W) % 4 + 4
    cap = 4 * (H * wp + 8) * 4 + 256  # the largest image: planar F32 x 4
    bufs = []
    for _ in range(2):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), cap) == 0
        bufs.append(p.value)
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0
    consumer = stream.value
    pinned = {}

    def host(fmt, ch):
        if (fmt, ch) not in pinned:
            pinned[(fmt, ch)] = [ctx.host_alloc((H, W, ch), abi.EXPORT_DTYPE[abi.EXPORT_FORMATS[fmt]]) for _ in range(2)]
        return pinned[(fmt, ch)]

    def k7(fn, n=20):
        ctx.sync()
        ctx.profile(True)
        for i in range(n):
            fn(i)
        ctx.sync()
        ms, launches = ctx.profile_read()["k7_export"]
        ctx.profile(False)
        assert launches == n, (launches, n)
        return round(ms / launches, 5)

    result = dict(width=W, height=H, seed=a.seed, launches_per_round=20, rounds=3, kernels={}, handover={})
    for fmt, ch, tm, ex in DEVICE_SPECS:
        elem = abi.EXPORT_DTYPE[abi.EXPORT_FORMATS[fmt]]().itemsize
        out = host(fmt, ch)
        images = {form: device_image_of(form, bufs[0], ch, elem)[0] for form in DEVICE_FORMS}
        runs = {"flat": lambda i: ctx.export_wait(ctx.stage_export(abi.TEX_EFFECT_INPUT, fmt, ch, tm, ex, out=out[i & 1]))}
        for form in DEVICE_FORMS:
            runs[form] = lambda i, form=form: ctx.export_device(abi.TEX_EFFECT_INPUT, fmt, ch, tm, ex, image=images[form])
        for fn in runs.values():  # warm every shape
            for i in range(3):
                fn(i)
        ms = {k: [] for k in runs}
        for r in range(3):
            for k, fn in runs.items():
                ms[k].append(k7(fn))
        flat = statistics.median(ms["flat"])
        row = dict(bytes_read=W * H * 16, bytes_written=W * H * ch * elem, flat_ms_rounds=ms["flat"], flat_ms=flat, flat_spread=round(max(ms["flat"]) - min(ms["flat"]), 5))
        for form in DEVICE_FORMS:
            med = statistics.median(ms[form])
            row[form] = dict(ms_rounds=ms[form], ms=med, of_flat=round(med / flat, 4), slower_than_flat_by_more_than_its_spread=bool(med - flat > row["flat_spread"]))
        result["kernels"]["%s_x%d_%s" % (fmt, ch, tm)] = row
        print(fmt, ch, tm, json.dumps(row), flush=True)
    # the hand-over: a frame on a consumer's stream, from the device image and through the host
    for fmt, ch, tm, ex in (("f16", 4, "linear", 1.0), ("u8_srgb", 3, "aces", 1.0)):
        elem = abi.EXPORT_DTYPE[abi.EXPORT_FORMATS[fmt]]().itemsize
        out = host(fmt, ch)
        image, nbytes = device_image_of("tight", bufs[0], ch, elem)

        def d1(n):
            t0 = time.perf_counter()
            for i in range(n):
                ctx.export_device(abi.TEX_EFFECT_INPUT, fmt, ch, tm, ex, image=image, stream=consumer)
                assert hip.hipMemcpyAsync(bufs[1], bufs[0], nbytes, 3, consumer) == 0  # the consumer reads the image
            assert hip.hipStreamSynchronize(consumer) == 0
            return (time.perf_counter() - t0) / n * 1e3

        def h1(n):
            t0 = time.perf_counter()
            for i in range(n):
                ctx.export_wait(ctx.stage_export(abi.TEX_EFFECT_INPUT, fmt, ch, tm, ex, out=out[i & 1]))
                assert hip.hipMemcpyAsync(bufs[0], out[i & 1].ctypes.data, nbytes, 1, consumer) == 0
                assert hip.hipMemcpyAsync(bufs[1], bufs[0], nbytes, 3, consumer) == 0
            assert hip.hipStreamSynchronize(consumer) == 0
            return (time.perf_counter() - t0) / n * 1e3

        d1(5), h1(5)
        rounds = []
        for r in range(3):
            row = dict(D1=round(d1(50), 4), H1=round(h1(50), 4))
            row["D1_of_H1"] = round(row["D1"] / row["H1"], 4)
            rounds.append(row)
        result["handover"]["%s_x%d_%s" % (fmt, ch, tm)] = dict(frame_bytes=nbytes, frames_per_round=50, rounds=rounds)
        print(fmt, ch, tm, json.dumps(rounds), flush=True)
    ctx.sync()
    ctx.close()
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged["device"] = result
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export", "rates.json"))
    ap.add_argument("--seconds", type=float, default=1.0, help="steady state per measurement, at least")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--size", default="3840x2160", help="frame size (the committed numbers are 4K; a small size checks the script itself)")
    ap.add_argument("--modes", default="png", choices=("png", "exr", "matches", "device"),
                    help='"exr": T0 / E1 / E2 / E3, added to --out under "exr"; "matches": T0 / T3 / T3m / E3 / E3m, added under "matches"; '
                         '"device": rfx_export_device per store form against the flat K7, and the hand-over to a consumer stream, added under "device"')
    ap.add_argument("--parent-lib", default=None, help="with --modes matches: a librfx_hip.so of the parent commit; only the encodes alone are measured, "
                                                       "on it and on this tree's library in alternating processes, and added to --out under --key")
    ap.add_argument("--processes", type=int, default=2, help="with --parent-lib: processes per library")
    ap.add_argument("--key", default="parent_against_tree", help="with --parent-lib: the key in --out")
    ap.add_argument("--encodes-only", action="store_true", help="with --modes matches: only the encodes alone, printed as one JSON line (what --parent-lib starts)")
    ap.add_argument("--lib", default=None, help="with --encodes-only: the librfx_hip.so to load instead of this tree's")
    a = ap.parse_args()
    global W, H
    W, H = (int(v) for v in a.size.split("x"))
    if a.modes == "matches" and a.parent_lib:
        return main_parent_against_tree(a)
    if a.lib:
        abi.set_library_path(a.lib)
    if a.modes == "device":
        return main_device(a)
    run = Run(a.seed)
    if a.modes == "matches" and a.encodes_only:
        run.alloc_exr()
        run.loop("T0", False, 5)  # a frame to encode
        print(json.dumps(encodes_alone(run)), flush=True)
        return run.ctx.close()
    if a.modes == "exr":
        return main_exr(run, a)
    if a.modes == "matches":
        return main_matches(run, a)
    result = dict(width=W, height=H, seed=a.seed, seconds=a.seconds, rounds={}, frames={})
    for streamed in (False, True):
        key = "streamed" if streamed else "resident"
        n = {}
        for mode in MODES:  # warm every shape, and size its loop from the warm rate
            w0, w1 = WARM.get(mode, (5, 20))
            run.loop(mode, streamed, w0)
            per = run.loop(mode, streamed, w1) / w1
            n[mode] = max(MIN_FRAMES.get(mode, 20), int(math.ceil(a.seconds / per)))
        rounds = []
        for r in range(3):
            row = {}
            for mode in MODES:
                row[mode] = round(run.loop(mode, streamed, n[mode]) / n[mode] * 1e3, 4)
            row["T2_minus_T0"] = round(row["T2"] - row["T0"], 4)
            row["T1_minus_T0"] = round(row["T1"] - row["T0"], 4)
            row["T2_below_T1"] = row["T2"] < row["T1"]
            row["T3_below_T2h"] = row["T3"] < row["T2h"]
            rounds.append(row)
            print(key, json.dumps(row), flush=True)
        result["rounds"][key] = rounds
        result["frames"][key] = n
    # K7 alone, inside a loop of exports
    ctx = run.ctx
    for _ in range(5):
        ctx.export_wait(ctx.stage_export(abi.TEX_FINAL, "u8_srgb", 3, "aces", 1.0, out=run.u8[0]))
    ctx.sync()
    ctx.profile(True)
    for i in range(20):
        ctx.export_wait(ctx.stage_export(abi.TEX_FINAL, "u8_srgb", 3, "aces", 1.0, out=run.u8[i & 1]))
    ms, launches = ctx.profile_read()["k7_export"]
    ctx.profile(False)
    moved = W * H * (16 + 3)
    result["k7_u8x3"] = dict(ms=round(ms / launches, 5), launches=launches, bytes=moved, ms_at_hbm_peak=round(moved / HBM_PEAK * 1e3, 5),
                             frac_of_hbm_peak=round(moved / HBM_PEAK * 1e3 / (ms / launches), 4))
    result["T2_below_T1_every_round"] = all(r["T2_below_T1"] for rs in result["rounds"].values() for r in rs)
    print(json.dumps(result["k7_u8x3"]), flush=True)
    # K8 alone (its three launches on the download stream), inside a loop of staged PNGs
    for _ in range(5):
        ctx.export_wait(ctx.stage_png(abi.TEX_FINAL, 3, "aces", 1.0, out=run.png[0]))
    ctx.sync()
    ctx.profile(True)
    for i in range(20):
        ctx.export_wait(ctx.stage_png(abi.TEX_FINAL, 3, "aces", 1.0, out=run.png[i & 1]))
    ms, launches = ctx.profile_read()["k8_png"]
    ctx.profile(False)
    fragment = int(np.frombuffer(run.png[1][:8].tobytes(), np.uint64)[0])
    stream = W * H * 3
    result["k8_png_u8x3"] = dict(ms=round(ms / launches, 5), launches=launches, bytes_read=stream, bytes_written=fragment, fragment_of_raw=round(fragment / stream, 4),
                                 bound=int(ctx.png_bound(3)), ms_at_hbm_peak=round((stream + fragment) / HBM_PEAK * 1e3, 5))
    result["fragment_bytes_per_frame"] = dict(min=min(run.fragment_bytes), max=max(run.fragment_bytes), frames=len(run.fragment_bytes)) if run.fragment_bytes else None
    result["T3_below_T2h_every_round"] = all(r["T3_below_T2h"] for rs in result["rounds"].values() for r in rs)
    print(json.dumps(result["k8_png_u8x3"]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
