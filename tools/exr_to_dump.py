#!/usr/bin/env python3
"""Convert a renderer's AOV EXR (+ side-car <file>.json with the cameras) into the dump directory both hosts read:
    python tools/exr_to_dump.py frame0001.exr dumps/f0001 [--map normal=N.X,N.Y,N.Z --map depth=Z.Z ...]
Layer names expected by default: rfx_amd.imageio.AOV_LAYOUT (diffuse.RGBA, normal.XYZ [world], roughness.Y, metalness.Y, emissive.RGB,
velocity.XY [uv units], depth.Z [gl_FragCoord.z], direct.RGBA).  The dump holds UNPACKED planes; the device packs them (rfx_pack_gbuffer, or
rfx_stage_aov when the dump is streamed).  --keep-half stores every layer the EXR holds as HALF channels as aov_<name>.f16.bin / direct.f16.bin
(two bytes per element on disk and on the bus, the same texels on the device; depth.bin stays float32)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))
from rfx_amd import dump  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("exr")
ap.add_argument("out")
ap.add_argument("--map", action="append", default=[], help="aov=chan0,chan1,... overrides a default layer mapping")
ap.add_argument("--keep-half", action="store_true", help="layers stored HALF in the EXR stay halves in the dump (*.f16.bin)")
a = ap.parse_args()
names = {m.split("=")[0]: tuple(m.split("=")[1].split(",")) for m in a.map}
f = dump.read_exr_dump(a.exr, names or None, typed=a.keep_half)
half = [k for k, v in dict(f.aov, direct=f.direct).items() if v.dtype == "float16"]
dump.write_dump(a.out, f, packed=False, half=half)
print("wrote", a.out, "%dx%d" % (f.width, f.height))
