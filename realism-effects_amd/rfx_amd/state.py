"""Checkpoint and resume of the temporal state (Node twin: ../js/state.js; the two hosts read each other's checkpoints).

Everything the chain carries from one frame to the next is either a device slot a later frame reads before writing — or leaves partly
unwritten: K2, K3 and K4 discard background texels, which keep the target's previous contents — or a handful of host-side numbers (the
blue-noise recurrences, keepData, the previous camera, frame counters).  save_state() writes both down at a frame boundary;
load_state() puts them back into fresh effects on a fresh context, and the frames that follow are byte-identical to an uninterrupted run.

A checkpoint is a directory:

  state.json              the header, written LAST (to a temporary name, then renamed over the previous one)
  <slot>.<generation>.plane   one raw whole-frame plane per saved slot: all H rows in frame order, the bytes rfx_download returns

The planes are whole-frame whatever the tiling: a row tile writes its own rows at their offset, one rank writes the header, and any
rank count loads the result — each tile takes the rows it holds, halo included, slots held whole (the composed GI) whole, so no exchange
is needed after a load.  Which slots are saved is asked of the effect objects (`state_slots()`); input planes (depth, G-buffer, velocity,
direct light, environment) are not state: the caller provides them every frame or at set-up.

Every save uses a new generation number in the plane names, so an interrupted save never touches the files the existing header names:
the previous checkpoint stays loadable until the new header has replaced it, and planes without a header are never read.  The header
carries each plane's size and SHA-256; a load validates the header, the planes and the fit to the running effects (class, texture count,
target type, denoiseMode, resolutionScale) BEFORE it touches an effect or the device, and names the field it refuses.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

from . import abi
from .effect import StateError

FORMAT = "rfx-temporal-state"
VERSION = 1
HEADER = "state.json"

__all__ = ["save_state", "load_state", "read_header", "state_slots", "StateError", "FORMAT", "VERSION"]


# ---- the two file operations of a save (tests make them fail part-way)
def _io_write(path: str, offset: int, data: bytes) -> None:
    """Write `data` at `offset` of `path` (created if missing, never truncated: other ranks write other rows of the same plane)."""
    fd = os.open(path, os.O_RDWR | os.O_CREAT, 0o644)
    try:
        view = memoryview(data)
        while len(view):
            n = os.pwrite(fd, view, offset)
            view, offset = view[n:], offset + n
        os.fsync(fd)
    finally:
        os.close(fd)


def _io_replace(src: str, dst: str) -> None:
    os.replace(src, dst)


def _texel_bytes(tex: int) -> int:
    dtype, ch = abi.TEX_FORMAT[tex]
    return np.dtype(dtype).itemsize * ch


def _effects(effects):
    return list(effects) if isinstance(effects, (list, tuple)) else [effects]


def state_slots(effects) -> list:
    """The slots a checkpoint of these effects holds, in a fixed order (each effect's `state_slots()`, first mention wins)."""
    slots = []
    for e in _effects(effects):
        for t in e.state_slots():
            if t not in slots:
                slots.append(t)
    return slots


def _geometry(renderer):
    H = int(renderer.H)
    y0 = int(getattr(renderer, "tile_y0", 0))
    rows = int(getattr(renderer, "tile_rows", H - y0))
    return int(renderer.W), H, y0, rows, int(getattr(renderer, "rank", 0)), int(getattr(renderer, "world", 1))


def _barrier(renderer, world):
    if world > 1:
        b = getattr(renderer, "state_barrier", None)
        if b is None:
            raise RuntimeError("save_state: a row-tiled renderer needs state_barrier() (TiledRenderer / CommTiledRenderer have one)")
        b()


def _settle(renderer):
    """Frame boundary: no overlapped gather or halo exchange in flight, every draw finished."""
    for name in ("finish_pending", "finish_halo"):
        f = getattr(renderer, name, None)
        if f:
            f()
    renderer.sync()


def read_header(directory: str) -> dict:
    """The parsed header of the checkpoint in `directory`, its format and version checked."""
    path = os.path.join(directory, HEADER)
    try:
        with open(path, "r") as f:
            header = json.load(f)
    except OSError as e:
        raise StateError("header", "no checkpoint in %s (%s)" % (directory, e))
    except ValueError as e:
        raise StateError("header", "%s is not JSON (%s)" % (path, e))
    if not isinstance(header, dict) or header.get("format") != FORMAT:
        raise StateError("format", "%r, expected %r" % (header.get("format") if isinstance(header, dict) else None, FORMAT))
    if header.get("version") != VERSION:
        raise StateError("version", "%r, this build reads version %d" % (header.get("version"), VERSION))
    return header


def _previous_generation(directory: str) -> int:
    try:
        g = read_header(directory).get("generation")
        return g if isinstance(g, int) and not isinstance(g, bool) and g >= 0 else 0
    except StateError:
        return 0


def save_state(directory: str, renderer, effects) -> dict:
    """Write the temporal state of `effects` on `renderer` into `directory` and return the header.  Call it between frames.  On a
    row-tiled renderer every rank calls it: each writes its own rows, rank 0 the header."""
    effects = _effects(effects)
    W, H, y0, rows, rank, world = _geometry(renderer)
    _settle(renderer)
    os.makedirs(directory, exist_ok=True)
    generation = _previous_generation(directory) + 1  # (the header does not change before the barrier below)
    slots = state_slots(effects)
    names = {t: "%s.%d.plane" % (abi.TEX_NAMES[t], generation) for t in slots}
    digests = {}
    for t in slots:
        band = np.ascontiguousarray(renderer.download(t, y0, rows))
        row_bytes = W * _texel_bytes(t)
        if band.nbytes != rows * row_bytes:
            raise RuntimeError("save_state: %s rows [%d, %d) came back as %d bytes, expected %d" % (abi.TEX_NAMES[t], y0, y0 + rows, band.nbytes, rows * row_bytes))
        _io_write(os.path.join(directory, names[t]), y0 * row_bytes, band.view(np.uint8).reshape(-1).data)
        if rows == H:  # the whole plane went through this rank's hands: no need to read it back
            digests[t] = hashlib.sha256(band.view(np.uint8).reshape(-1).data).hexdigest()
    _barrier(renderer, world)  # every rank's rows are on disk
    header = dict(format=FORMAT, version=VERSION, generation=generation, width=W, height=H, planes=[], effects=[e.get_state() for e in effects])
    if rank == 0:
        for t in slots:
            path, size = os.path.join(directory, names[t]), H * W * _texel_bytes(t)
            os.truncate(path, size)  # (a longer leftover of an interrupted save at another frame size)
            header["planes"].append(dict(slot=abi.TEX_NAMES[t], file=names[t], texelBytes=_texel_bytes(t), rows=H, sha256=digests.get(t) or _sha256(path)))
        tmp = os.path.join(directory, HEADER + ".tmp")
        if os.path.exists(tmp):
            os.unlink(tmp)
        _io_write(tmp, 0, json.dumps(header, indent=1, sort_keys=True).encode())
        _io_replace(tmp, os.path.join(directory, HEADER))  # the checkpoint exists from here on
        for name in os.listdir(directory):  # the planes of earlier generations
            if name.endswith(".plane") and name not in names.values():
                try:
                    os.unlink(os.path.join(directory, name))
                except OSError:
                    pass
    _barrier(renderer, world)  # nobody returns (to load, or to save again) before the header is there
    return header if rank == 0 else read_header(directory)


def _sha256(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def load_state(directory: str, renderer, effects) -> dict:
    """Restore the checkpoint in `directory` into `effects` and `renderer` (fresh or running) and return its header.  Everything is
    validated first: a refusal raises StateError naming the field and leaves the effects and the device untouched."""
    effects = _effects(effects)
    W, H = int(renderer.W), int(renderer.H)
    header = read_header(directory)
    for key, have in (("width", W), ("height", H)):
        if header.get(key) != have:
            raise StateError(key, "saved %r, the renderer has %d" % (header.get(key), have))
    saved = header.get("effects")
    if not isinstance(saved, list) or len(saved) != len(effects):
        raise StateError("effects", "%s saved, %d given" % (len(saved) if isinstance(saved, list) else "none", len(effects)))
    for i, (e, s) in enumerate(zip(effects, saved)):
        if not isinstance(s, dict):
            raise StateError("effects[%d]" % i, "not a record")
        e.check_state(s, "effects[%d]" % i)
    # the slots the RESTORED effects will keep (TRAAEffect builds its pass from the record): ask for them after the checks, from the records
    want = _slots_after_load(effects, saved)
    planes = header.get("planes")
    if not isinstance(planes, list) or not all(isinstance(p, dict) for p in planes):
        raise StateError("planes", "missing")
    have = [p.get("slot") for p in planes]
    if sorted(have) != sorted(abi.TEX_NAMES[t] for t in want):
        raise StateError("planes", "saved %s, the running effects keep %s" % (sorted(have), sorted(abi.TEX_NAMES[t] for t in want)))
    data = {}
    for p in planes:
        slot = p["slot"]
        t, field = abi.TEX_NAMES.index(slot), "planes[%s]" % slot
        if p.get("texelBytes") != _texel_bytes(t):
            raise StateError(field + ".texelBytes", "saved %r, the slot has %d" % (p.get("texelBytes"), _texel_bytes(t)))
        if p.get("rows") != H:
            raise StateError(field + ".rows", "saved %r, the frame has %d" % (p.get("rows"), H))
        name = p.get("file")
        if not isinstance(name, str) or os.path.basename(name) != name:
            raise StateError(field + ".file", "%r is not a file name" % (name,))
        try:
            raw = np.fromfile(os.path.join(directory, name), np.uint8)
        except OSError as e:
            raise StateError(field + ".file", str(e))
        if raw.size != H * W * _texel_bytes(t):
            raise StateError(field + ".size", "%d bytes, expected %d" % (raw.size, H * W * _texel_bytes(t)))
        if hashlib.sha256(raw.data).hexdigest() != p.get("sha256"):
            raise StateError(field + ".sha256", "the plane does not match its checksum")
        dtype, ch = abi.TEX_FORMAT[t]
        data[t] = raw.view(dtype).reshape((H, W, ch) if ch > 1 else (H, W))
    # ---- everything fits: apply
    _settle(renderer)
    for t, plane in data.items():
        _upload_held(renderer, t, plane)
        if t == abi.TEX_COMPOSE and getattr(renderer, "gather_history_rgb", False):
            # a row-tiled run hands K1 the .rgb twin of the composed GI (tiling.py); it is not a plane of its own
            _upload_held(renderer, abi.TEX_COMPOSE_RGB, np.ascontiguousarray(plane[..., :3]))
    for e, s in zip(effects, saved):
        e.set_state(s)
    renderer.sync()
    return header


def _upload_held(renderer, tex, plane):
    r0, n = renderer.held_rows(tex)
    renderer.upload(tex, np.ascontiguousarray(plane[r0:r0 + n]), r0, n)


def _slots_after_load(effects, saved):
    slots = []
    for e, s in zip(effects, saved):
        f = getattr(e, "state_slots_of", None)
        for t in (f(s) if f else e.state_slots()):
            if t not in slots:
                slots.append(t)
    return slots
