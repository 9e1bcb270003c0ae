#!/usr/bin/env python3
"""What a change of scene.environment costs (GPU box; fails without a device): wall time per environment update through

    host    the blocking path: cube_to_equirect (upload, draw, read-back) + set_environment (upload again, mip chain) + envmap.build_importance on
            the host + set_environment_importance — every step with its own wait
    device  set_environment_cube / set_environment + build_environment_importance (K10): stream-ordered, the map never leaves the device

for two cases — `cube`: a 256 x 256 cube with mipmaps, converted to 1024 x 512; `equirect`: a 4096 x 2048 HalfFloatType equirectangular map with
flipY — and `chain`: milliseconds per frame of the 1080p SSGI chain (steps 20 / refineSteps 5) through SSGIEffect with a NEW cube every frame,
env_on_device off and on.  In ONE process: every mode is warmed first, then three alternating rounds, each mode a steady state of at least
--seconds (and at least two updates) with a device synchronise inside the clock.  Required: device < host in every round of every case.

    python tools/environment_rate.py [--out profiles/environment] [--seconds 1.0]            writes rates.json and README.md there
    rocprofv3 --kernel-trace --stats -d DIR -o k --output-format csv -- python tools/environment_rate.py --kernel-only cube|equirect
                                                                        (the kernels' own times: a run of its own per size)
    python tools/environment_rate.py --out profiles/environment --kernel-stats cube=DIR/.../k_kernel_stats.csv equirect=...   folds them in
"""
import argparse
import csv
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))

from rfx_amd import abi, effect  # noqa: E402
from rfx_amd.context import Context  # noqa: E402
from rfx_amd.envmap import build_importance  # noqa: E402
from rfx_amd.scene import synthetic_frame  # noqa: E402

CUBE, CUBE_TARGET, EQUIRECT = 256, (1024, 512), (4096, 2048)
CASES = ("cube", "equirect", "chain")
ROUNDS = 3


def hdr(seed, shape):
    return (10.0 ** np.random.RandomState(seed).uniform(-3.0, 3.0, shape)).astype(np.float32)


def cubes():
    return [hdr(s, (6, CUBE, CUBE, 4)) for s in (1, 2)]


def update_cube(ctx, faces, device):
    w, h = CUBE_TARGET
    if device:
        ctx.set_environment_cube(faces, w, h, generate_mipmaps=True)
        ctx.build_environment_importance(False)
    else:
        eq = ctx.cube_to_equirect(faces, w, h, generate_mipmaps=True)
        ctx.set_environment(eq, half_float_type=False, half_store_rtz=False)
        ctx.set_environment_importance(*build_importance(eq))


def update_equirect(ctx, data, device):
    ctx.set_environment(data, half_float_type=True, half_store_rtz=True)
    if device:
        ctx.build_environment_importance(True)
    else:  # effect.keepEnvMapUpdated's host path for a HalfFloatType map with flipY
        texels = data.astype(np.float16).astype(np.float32)
        ctx.set_environment_importance(*build_importance(texels[::-1], True))


def steady(step, sync, seconds):
    """milliseconds per call of step(i) over at least `seconds` and two calls, the device drained inside the clock"""
    sync()
    n, t0 = 0, time.perf_counter()
    while n < 2 or time.perf_counter() - t0 < seconds:
        step(n)
        n += 1
    sync()
    return (time.perf_counter() - t0) * 1e3 / n, n


def measure(modes, sync, seconds):
    """modes: {name: step}; warm each, then ROUNDS alternating rounds"""
    for step in modes.values():
        step(0)
        step(1)
    sync()
    rounds = []
    for _ in range(ROUNDS):
        row = {}
        for name, step in modes.items():
            row[name], row[name + "_updates"] = steady(step, sync, seconds)
        row["device_below_host"] = row["device"] < row["host"]
        rounds.append(row)
    return rounds


def case_updates(kind, seconds):
    ctx = Context(64, 64)
    items = cubes() if kind == "cube" else [hdr(s, (EQUIRECT[1], EQUIRECT[0], 4)) for s in (3, 4)]
    items = [np.minimum(a, np.float32(6e4)) for a in items]
    fn = update_cube if kind == "cube" else update_equirect
    rounds = measure({"host": lambda i: fn(ctx, items[i & 1], False), "device": lambda i: fn(ctx, items[i & 1], True)}, ctx.sync, seconds)
    ctx.close()
    return rounds


def case_chain(seconds):
    W, H = 1920, 1080
    f = synthetic_frame(W, H, 0)
    faces = cubes()
    modes, ctxs = {}, []
    for name, on in (("host", False), ("device", True)):
        ctx = Context(W, H)
        scene = types.SimpleNamespace(frame=f, environment=None)
        fx = effect.SSGIEffect(None, scene, types.SimpleNamespace(**vars(f.camera)), dict(width=W, height=H, steps=20, refineSteps=5, denoiseIterations=1),
                               seeds=dict(ssgi=11, denoise=22), env_on_device=on)

        def step(i, ctx=ctx, scene=scene, fx=fx):
            scene.environment = dict(isCubeTexture=True, faces=faces[i & 1])  # a new object: the environment changed
            fx.update(ctx, None)
        modes[name] = step
        ctxs.append(ctx)
    rounds = measure(modes, lambda: [c.sync() for c in ctxs], seconds)
    for c in ctxs:
        c.close()
    return rounds


def kernel_only(kind, n=10):
    """n builds (and, for the cube, n conversions) of one size, for rocprofv3"""
    ctx = Context(64, 64)
    if kind == "cube":
        for faces in cubes() * (n // 2):
            update_cube(ctx, faces, True)
    else:
        ctx.set_environment(np.minimum(hdr(3, (EQUIRECT[1], EQUIRECT[0], 4)), np.float32(6e4)), half_float_type=True, half_store_rtz=True)
        for _ in range(n):
            ctx.build_environment_importance(True)
    ctx.sync()
    ctx.close()


def read_stats(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if any(k in name for k in ("k10_", "k0_cube", "env_mip")):
            short = name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
            rows[short] = dict(calls=int(r["Calls"]), mean_ms=float(r["AverageNs"]) * 1e-6, min_ms=float(r["MinNs"]) * 1e-6, max_ms=float(r["MaxNs"]) * 1e-6)
    return rows


def fmt(rounds, key):
    return " / ".join("%.3f" % r[key] for r in rounds)


def write_readme(out, res):
    L = ["# profiles/environment — what a change of scene.environment costs", "",
         "`rates.json`: `python tools/environment_rate.py` on one MI355X; every mode warmed, then three alternating rounds, each mode a steady state of at",
         "least %.1f s (and at least two updates) with a device synchronise inside the clock.  `host`: `cube_to_equirect` + `set_environment` +" % res["seconds"],
         "`envmap.build_importance` + `set_environment_importance` (the blocking path, unchanged); `device`: `set_environment_cube` / `set_environment` +",
         "`build_environment_importance` (K10).  Both leave the same bytes on the device (tests/test_gpu_env_device.py).", "",
         "| case | host, ms (three rounds) | device, ms (three rounds) | host / device |", "|---|---|---|---|"]
    what = {"cube": "update: a %d² cube with mipmaps → %d × %d" % ((CUBE,) + CUBE_TARGET), "equirect": "update: a %d × %d HalfFloatType map with flipY" % EQUIRECT,
            "chain": "1080p SSGI chain (steps 20 / 5), a new cube every frame: ms per frame"}
    for k in CASES:
        if k in res["cases"]:
            r = res["cases"][k]
            L.append("| %s | %s | %s | %s |" % (what[k], fmt(r, "host"), fmt(r, "device"), " / ".join("%.1f" % (x["host"] / x["device"]) for x in r)))
    bad = [(k, i) for k, r in res["cases"].items() for i, x in enumerate(r) if not x["device_below_host"]]
    L += ["", "**Required: device < host in every round of every case — %s**" % ("holds" if not bad else "FAILS in " + ", ".join("%s round %d" % b for b in bad)) + ".", ""]
    if res.get("kernels"):
        L += ["Reported, no threshold — the kernels' own times (`rocprofv3 --kernel-trace --stats -- python tools/environment_rate.py --kernel-only <case>`,",
              "a run of its own per size; mean (min – max) per launch):", "", "| kernel | " + " | ".join("%s" % k for k in res["kernels"]) + " |", "|---|" + "---|" * len(res["kernels"])]
        names = sorted({n for v in res["kernels"].values() for n in v})
        for n in names:
            cells = []
            for v in res["kernels"].values():
                s = v.get(n)
                cells.append("%.4f ms (%.4f – %.4f), %d launches" % (s["mean_ms"], s["min_ms"], s["max_ms"], s["calls"]) if s else "—")
            L.append("| `%s` | %s |" % (n, " | ".join(cells)))
        L += ["", "`k10_total` is the serial chain over all W·H weights (one workgroup, one dependent double add per texel), the figure nobody had measured:",
              "it is the device path's time.  Its mean over the texels is the cost of one dependent `v_add_f64` in this loop.", ""]
    open(os.path.join(out, "README.md"), "w").write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "environment"))
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--kernel-only", choices=("cube", "equirect"))
    ap.add_argument("--kernel-stats", nargs="*", help="case=kernel_stats.csv of a --kernel-only run under rocprofv3: folded into rates.json and README.md")
    a = ap.parse_args()
    if a.kernel_only:
        return kernel_only(a.kernel_only)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "rates.json")
    if a.kernel_stats is not None:
        res = json.load(open(path))
        res["kernels"] = {"%s (%d × %d)" % ((k,) + (CUBE_TARGET if k == "cube" else EQUIRECT)): read_stats(p) for k, p in (s.split("=", 1) for s in a.kernel_stats)}
    else:
        probe = Context(16, 16)
        assert probe.has_env_device
        probe.close()
        res = dict(tool="tools/environment_rate.py", seconds=a.seconds, abi=abi.RFX_ABI_VERSION, cases={})
        for k in a.cases.split(","):
            res["cases"][k] = case_chain(a.seconds) if k == "chain" else case_updates(k, a.seconds)
            print(k, json.dumps(res["cases"][k]), flush=True)
        res["required_device_below_host_every_round"] = all(x["device_below_host"] for r in res["cases"].values() for x in r)
    json.dump(res, open(path, "w"), indent=1)
    write_readme(a.out, res)
    print(json.dumps({"required_device_below_host_every_round": res.get("required_device_below_host_every_round")}))


if __name__ == "__main__":
    main()
