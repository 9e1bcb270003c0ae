#!/usr/bin/env python3
"""Convert a renderer's AOV EXR (+ side-car <file>.json with the cameras) into the dump directory both hosts read:
    python tools/exr_to_dump.py frame0001.exr dumps/f0001 [--map normal=N.X,N.Y,N.Z --map depth=Z.Z ...]
Layer names expected by default: rfx_amd.imageio.AOV_LAYOUT (diffuse.RGBA, normal.XYZ [world], roughness.Y, metalness.Y, emissive.RGB,
velocity.XY [uv units], depth.Z [gl_FragCoord.z], direct.RGBA).  The dump holds UNPACKED planes; the device packs them (rfx_pack_gbuffer, or
rfx_stage_aov when the dump is streamed).  --keep-half stores every layer the EXR holds as HALF channels as aov_<name>.f16.bin / direct.f16.bin
(two bytes per element on disk and on the bus, the same texels on the device; depth.bin stays float32).
--conventions JSON: the EXR is in an engine's conventions (include/rfx.h "AOV conventions") — e.g. '{"depth_kind": "position", "velocity_kind":
"cameras", "normal_space": "view", "background_position": [0, 0, 0]}' with --map position=P.X,P.Y,P.Z --map velocity= (no velocity layer), or
'{"depth_kind": "view_z", "velocity_kind": "scaled", "velocity_scale": [0.00026, -0.00046]}' with --map view_z=Z.Z.  The matrices come from the
side-car's cameras unless the JSON carries them.  The planes are converted on the host (rfx_amd.imageio.aov_to_reference_conventions: the pack
kernel's arithmetic in numpy float32) and the dump is in the reference's form, as without the option."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))
from rfx_amd import dump, imageio  # noqa: E402
from rfx_amd.conventions import MATRICES, AovConventions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("exr")
ap.add_argument("out")
ap.add_argument("--map", action="append", default=[], help="aov=chan0,chan1,... overrides a default layer mapping")
ap.add_argument("--keep-half", action="store_true", help="layers stored HALF in the EXR stay halves in the dump (*.f16.bin)")
ap.add_argument("--conventions", default=None, help="JSON (or a file holding it): depth_kind, velocity_kind, normal_space, velocity_scale, background_position, matrices")
a = ap.parse_args()
names = {m.split("=")[0]: tuple(c for c in m.split("=")[1].split(",") if c) for m in a.map}
f = dump.read_exr_dump(a.exr, names or None, typed=a.keep_half)
if a.conventions:
    spec = json.loads(open(a.conventions).read() if os.path.exists(a.conventions) else a.conventions)
    conv = AovConventions.from_cameras(f.camera, f.prev_camera, **{k: (tuple(v) if isinstance(v, list) else v) for k, v in spec.items() if k not in MATRICES})
    for k in MATRICES:
        if k in spec:
            setattr(conv, k, np.asarray(spec[k], np.float32).reshape(16))
    key = {"fragcoord": "depth", "view_z": "view_z", "position": "position"}[conv.depth_kind]
    out = imageio.aov_to_reference_conventions(dict(f.aov, **{key: f.depth}), conv)
    f.depth = out.pop("depth")
    f.aov = out
half = [k for k, v in dict(f.aov, direct=f.direct).items() if v.dtype == "float16"]
dump.write_dump(a.out, f, packed=False, half=half)
print("wrote", a.out, "%dx%d" % (f.width, f.height))
