"""On-disk dump format shared by the Python and Node hosts: `frame.json` + raw little-endian
planes, row 0 = bottom (the "pre-dumped Float32/Uint8 arrays" of the north star).

  frame.json    {width, height, camera{...}, prevCamera{...}}  (matrices = 16 numbers, column-major)
  depth.bin     float32 W*H          gbuffer.bin   uint32 W*H*4 (bit patterns of the RGBA32F texels)
  velocity.bin  uint32  W*H*4        direct.bin    float32 W*H*4

An engine that exports UNPACKED attribute planes writes, instead of gbuffer.bin and velocity.bin (write_dump(..., packed=False)):
  aov_diffuse.bin float32 W*H*4   aov_normal.bin float32 W*H*3 (world space)   aov_roughness.bin / aov_metalness.bin float32 W*H
  aov_emissive.bin float32 W*H*3  aov_velocity.bin float32 W*H*2 (uv units)
and the device packs them (rfx_pack_gbuffer / rfx_pack_velocity, or rfx_stage_aov on the upload stream).  A plane whose values are halves may be
stored as such — aov_<name>.f16.bin / direct.f16.bin, IEEE binary16, instead of the .bin (write_dump(..., packed=False, half=(names))) — and is
read back as float16: the typed frame Context.stage_aov sends at two bytes per element.  diffuse and direct may have three channels (alpha 1):
the count follows from the file size.

A renderer's usual AOV container is one multi-layer OpenEXR per frame: read_exr_dump() / write_exr_dump() map it onto the same frame
object (layer names: rfx_amd.imageio.AOV_LAYOUT; the cameras travel in the EXR's side-car `<name>.json`, same fields as frame.json).
"""
from __future__ import annotations

import json
import os
import types

import numpy as np

_CAM_FIELDS = ("projectionMatrix", "projectionMatrixInverse", "matrixWorld", "matrixWorldInverse", "position", "quaternion")


def _cam_to_json(cam):
    d = {k: [float(x) for x in np.asarray(getattr(cam, k)).ravel()] for k in _CAM_FIELDS if hasattr(cam, k)}
    d.update(near=float(cam.near), far=float(cam.far), isPerspectiveCamera=bool(getattr(cam, "isPerspectiveCamera", True)))
    return d


def _cam_from_json(d):
    ns = types.SimpleNamespace(**{k: (np.asarray(v, np.float64) if k == "quaternion" else np.asarray(v, np.float32)) for k, v in d.items()
                                  if k in _CAM_FIELDS})
    ns.near, ns.far, ns.isPerspectiveCamera = d["near"], d["far"], d.get("isPerspectiveCamera", True)
    return ns


_AOV = (("diffuse", 4), ("normal", 3), ("roughness", 1), ("metalness", 1), ("emissive", 3), ("velocity", 2))


def _plane_file(dirname, stem, half=None):
    """(path, dtype) of a plane's file: `half` True / False names the one to write; None finds the one that exists (.f16.bin first)"""
    f16 = os.path.join(dirname, stem + ".f16.bin")
    if half or (half is None and os.path.exists(f16)):
        return f16, np.float16
    return os.path.join(dirname, stem + ".bin"), np.float32


_ENGINE_DEPTH = {"position": ("aov_position", 3), "view_z": ("aov_view_z", 1)}  # depth_kind -> (file stem, channels) of the plane that stands for depth.bin


def write_dump(dirname: str, frame, packed: bool = True, half=(), conventions=None) -> None:
    """`half` (unpacked dumps): the names among the AOV planes and "direct" to store as binary16 (the values are rounded if they are no halves).
    `conventions` (unpacked dumps; conventions.AovConventions): an ENGINE-FORM dump (rfx.h "AOV conventions") — frame.depth is the depth plane
    in the setting's kind and is written as aov_position(.f16).bin / aov_view_z(.f16).bin ("depth" in `half` stores it as halves), frame.aov
    holds the planes as the engine writes them (no "velocity" under velocity_kind "cameras"), frame.json carries the record."""
    os.makedirs(dirname, exist_ok=True)
    if conventions is not None and packed:
        raise ValueError("write_dump: conventions belong to an unpacked dump (packed=False)")
    if conventions is not None:
        return _write_engine_dump(dirname, frame, set(half), conventions)
    if packed and half:
        raise ValueError("write_dump: half planes belong to an unpacked dump (packed=False)")
    unknown = set(half) - {k for k, _ in _AOV} - {"direct"}
    if unknown:
        raise ValueError("write_dump: no such plane to store as half: %s" % sorted(unknown))
    meta = dict(width=int(frame.width), height=int(frame.height), camera=_cam_to_json(frame.camera),
                prevCamera=_cam_to_json(getattr(frame, "prev_camera", frame.camera)))
    with open(os.path.join(dirname, "frame.json"), "w") as f:
        json.dump(meta, f)
    np.ascontiguousarray(frame.depth, np.float32).tofile(os.path.join(dirname, "depth.bin"))
    if packed:
        np.ascontiguousarray(frame.gbuffer).view(np.uint32).tofile(os.path.join(dirname, "gbuffer.bin"))
        np.ascontiguousarray(frame.velocity).view(np.uint32).tofile(os.path.join(dirname, "velocity.bin"))
    else:
        for k, _ in _AOV:
            path, dt = _plane_file(dirname, "aov_" + k, k in half)
            np.ascontiguousarray(frame.aov[k], dt).tofile(path)
    path, dt = _plane_file(dirname, "direct", "direct" in half)
    np.ascontiguousarray(frame.direct, dt).tofile(path)


def _write_engine_dump(dirname, frame, half, conventions):
    meta = dict(width=int(frame.width), height=int(frame.height), camera=_cam_to_json(frame.camera),
                prevCamera=_cam_to_json(getattr(frame, "prev_camera", frame.camera)), aovConventions=json.loads(conventions.to_json()))
    with open(os.path.join(dirname, "frame.json"), "w") as f:
        json.dump(meta, f)
    stem = _ENGINE_DEPTH.get(conventions.depth_kind, ("depth", 1))[0]
    path, dt = _plane_file(dirname, stem, "depth" in half and stem != "depth")
    np.ascontiguousarray(frame.depth, dt).tofile(path)
    for k, _ in _AOV:
        if k == "velocity" and frame.aov.get(k) is None:
            continue
        path, dt = _plane_file(dirname, "aov_" + k, k in half)
        np.ascontiguousarray(frame.aov[k], dt).tofile(path)
    path, dt = _plane_file(dirname, "direct", "direct" in half)
    np.ascontiguousarray(frame.direct, dt).tofile(path)


def read_dump(dirname: str):
    """-> a frame namespace.  An engine-form directory (write_dump(..., conventions=)): frame.conventions is its AovConventions, frame.depth the
    position / view Z plane, and Context.stage_frame sets the one before it stages the other; else frame.conventions is None."""
    with open(os.path.join(dirname, "frame.json")) as f:
        meta = json.load(f)
    W, H = meta["width"], meta["height"]
    rd = lambda n, dt, shape: np.fromfile(os.path.join(dirname, n), dt).reshape(shape)  # noqa: E731

    def typed(stem, channels):  # .f16.bin or .bin, whichever exists; `channels`: the counts the plane may have
        path, dt = _plane_file(dirname, stem)
        a = np.fromfile(path, dt)
        ch = a.size // (W * H) if W * H else 0
        if ch not in channels or a.size != W * H * ch:
            raise ValueError("%s: %d elements do not make %s channel(s) of a %d x %d frame" % (path, a.size, " or ".join(map(str, channels)), W, H))
        return a.reshape((H, W, ch) if max(channels) > 1 else (H, W))

    has = lambda stem: any(os.path.exists(os.path.join(dirname, stem + e)) for e in (".bin", ".f16.bin"))  # noqa: E731
    engine = [v for v in _ENGINE_DEPTH.values() if has(v[0])]
    depth = typed(engine[0][0], (engine[0][1],)) if engine else rd("depth.bin", np.float32, (H, W))
    conv = None
    if meta.get("aovConventions"):
        from .conventions import MATRICES, AovConventions
        rec = dict(meta["aovConventions"])
        cams = AovConventions.from_cameras(_cam_from_json(meta["camera"]), _cam_from_json(meta["prevCamera"]))
        for k in MATRICES + ("near", "far", "perspective"):  # (a record without the cameras' part: from the frame's own cameras)
            rec.setdefault(k, getattr(cams, k))
        conv = AovConventions.from_json(rec)
    fr = types.SimpleNamespace(width=W, height=H, camera=_cam_from_json(meta["camera"]), prev_camera=_cam_from_json(meta["prevCamera"]),
                               depth=depth, direct=typed("direct", (3, 4)), gbuffer=None, velocity=None,
                               aov=None, conventions=conv)
    if os.path.exists(os.path.join(dirname, "gbuffer.bin")):
        fr.gbuffer, fr.velocity = rd("gbuffer.bin", np.uint32, (H, W, 4)), rd("velocity.bin", np.uint32, (H, W, 4))
    else:
        fr.aov = {k: typed("aov_" + k, (3, 4) if k == "diffuse" else (ch,)) for k, ch in _AOV if not (k == "velocity" and not has("aov_velocity"))}
    return fr


def write_exr_dump(path: str, frame, compression: str = "zip") -> None:
    """One multi-layer EXR (`path`) + side-car `path`.json (cameras) from a frame that carries unpacked attribute planes (frame.aov)."""
    from . import imageio
    ch = {}
    for key, names in imageio.AOV_LAYOUT.items():
        a = frame.depth if key == "depth" else (frame.direct if key == "direct" else frame.aov[key])
        a = np.asarray(a, np.float32)
        a = a[..., None] if a.ndim == 2 else a
        for i, n in enumerate(names):
            ch[n] = a[..., i]
    imageio.write_exr(path, ch, compression)
    meta = dict(width=int(frame.width), height=int(frame.height), camera=_cam_to_json(frame.camera),
                prevCamera=_cam_to_json(getattr(frame, "prev_camera", frame.camera)))
    with open(path + ".json", "w") as f:
        json.dump(meta, f)


def read_exr_dump(path: str, names: dict | None = None, typed: bool = False):
    """The inverse: a frame whose G-buffer / velocity come as unpacked attribute planes (frame.aov) for the device-side importer.  `typed`:
    layers stored HALF stay float16 (imageio.exr_to_typed_planes): the frame Context.stage_aov sends at two bytes per half element."""
    from . import imageio
    planes = (imageio.exr_to_typed_planes if typed else imageio.exr_to_dump_planes)(path, names)
    with open(path + ".json") as f:
        meta = json.load(f)
    H, W = planes["depth"].shape[:2]  # (a world position plane — names={"position": ...} — has three channels)
    if (W, H) != (meta["width"], meta["height"]):
        raise ValueError("%s: image is %dx%d, side-car says %dx%d" % (path, W, H, meta["width"], meta["height"]))
    return types.SimpleNamespace(width=W, height=H, camera=_cam_from_json(meta["camera"]), prev_camera=_cam_from_json(meta["prevCamera"]),
                                 depth=planes["depth"], direct=planes["direct"], gbuffer=None, velocity=None, aov=planes["aov"])
