"""Per-frame output of an offline run through the streamed export (include/rfx.h "streamed frame export"): the Python twin of js/frames.js.

    png -> EXPORT_U8_SRGB x 3 (tonemap / exposure)     exr -> EXPORT_F16 x 4     pfm -> EXPORT_F32 x 3

submit(source) is called once per frame AFTER the frame's draws are enqueued: it stages this frame's export into one of two pinned buffers,
then waits for the PREVIOUS frame's ticket — which has had this frame's draws to hide behind — and hands its bytes to `write`.  At most two
exports are in flight; finish() waits for the last one.

compression="zips" (exr only; default "none"): the frame leaves the device as finished ZIPS chunks (Context.stage_exr, include/rfx.h "EXR
fragments") and the host only wraps them; "none" is the uncompressed file written from the staged halfs.

matches=True (with encode="device" or compression="zips" only): the device encode with run-length matches (include/rfx.h "Match form"); the
files are smaller where pixels repeat exactly and wrap the same way."""
from __future__ import annotations

import os

import numpy as np

from . import abi, imageio

FRAME_FORMATS = {"png": ("u8_srgb", 3), "exr": ("f16", 4), "pfm": ("f32", 3)}


class FrameExporter:
    def __init__(self, ctx, directory: str, format: str = "png", tonemap: str = "aces", exposure: float = 1.0, write=None, encode: str = "host",
                 filter="adaptive", compression: str = "none", matches: bool = False):
        if format not in FRAME_FORMATS:
            raise ValueError('format: "png", "exr" or "pfm"')
        if encode not in ("host", "device"):
            raise ValueError('encode: "host" or "device"')
        if encode == "device" and format != "png":
            raise ValueError('encode "device" is for format "png" only')
        if compression not in ("none", "zips"):
            raise ValueError('compression: "none" or "zips"')
        if compression == "zips" and format != "exr":
            raise ValueError('compression "zips" is for format "exr" only')
        if matches and encode != "device" and compression != "zips":
            raise ValueError('matches is for encode "device" or compression "zips" only')
        if matches and not ctx.has_export_matches:
            raise ValueError("matches: this librfx_hip.so has no rfx_stage_png_ex (Context.has_export_matches)")
        self.encode, self.filter, self.compression, self.matches = encode, filter, compression, bool(matches)
        self.ctx, self.dir, self.format = ctx, directory, format
        self.kind, self.channels = FRAME_FORMATS[format]
        u8 = self.kind == "u8_srgb"
        self.tonemap, self.exposure = (tonemap if u8 else "linear"), (float(exposure) if u8 else 1.0)
        dtype = abi.EXPORT_DTYPE[abi.EXPORT_FORMATS[self.kind]]
        if encode == "device":  # the payload is a PNG fragment (Context.stage_png): the host wraps it and writes
            self.buffers = [ctx.host_alloc((ctx.png_bound(self.channels),), np.uint8) for _ in range(2)]
        elif compression == "zips":  # the payload is an EXR fragment (Context.stage_exr)
            self.buffers = [ctx.host_alloc((ctx.exr_bound(self.channels),), np.uint8) for _ in range(2)]
        else:
            self.buffers = [ctx.host_alloc((ctx.tile_rows, ctx.W, self.channels), dtype) for _ in range(2)]
        self.write = write or self.write_frame
        self.count, self.pending = 0, None

    def write_frame(self, index: int, data: np.ndarray):
        path = os.path.join(self.dir, "frame_%05d.%s" % (index, self.format))
        if self.encode == "device":
            with open(path, "wb") as f:
                f.write(imageio.png_from_fragments(self.ctx.W, self.ctx.tile_rows, self.channels, [data]))
        elif self.compression == "zips":
            with open(path, "wb") as f:
                f.write(imageio.exr_from_fragments(self.ctx.W, self.ctx.tile_rows, self.channels, [data]))
        elif self.format == "png":
            imageio.write_png(path, data)
        elif self.format == "exr":
            imageio.write_exr(path, {n: data[..., k] for k, n in enumerate("RGBA")}, compression="none", half=True)
        else:
            imageio.write_pfm(path, data)

    def submit(self, source: int):
        index, self.count = self.count, self.count + 1
        buf = self.buffers[index & 1]
        if self.encode == "device":
            ticket = self.ctx.stage_png(source, self.channels, self.tonemap, self.exposure, self.filter, out=buf, **self._matches_kw())
        elif self.compression == "zips":
            ticket = self.ctx.stage_exr(source, self.channels, out=buf, **self._matches_kw())
        else:
            ticket = self.ctx.stage_export(source, self.kind, self.channels, self.tonemap, self.exposure, out=buf)
        self._retire()
        self.pending = (ticket, index, buf)

    def _matches_kw(self):
        return {"matches": True} if self.matches else {}  # (off: the call as it was, for a ctx that predates the keyword)

    def _retire(self):
        if self.pending is None:
            return
        (ticket, index, buf), self.pending = self.pending, None
        self.ctx.export_wait(ticket)
        self.write(index, buf)

    def finish(self):
        self._retire()


class ExrSequence:
    """Per-frame input of an offline run through the device EXR decode (include/rfx.h "streamed EXR frames"): the AOV EXR files of a directory, or
    a list of paths, read with readinto() into two alternating pinned buffers and staged with Context.stage_exr_device (the EXR blocks where the
    library has them: scanline and tiled parts, NONE / RLE / ZIPS / ZIP / PXR24).

        seq = ExrSequence(ctx, directory);  seq.stage(0); ctx.stage_flip()
        for i in range(len(seq)):  seq.stage(i + 1) if i + 1 < len(seq) else None;  <draws of frame i>;  ctx.stage_flip()

    Buffer k & 1 is refilled for frame k when the flip after frame k - 1's has returned: rfx_stage_flip's back pressure says the copies out of
    it have executed.  A file the device decode does not take (imageio.ExrNotStreamable) is read on the host (Context.stage_exr_frame): a PIZ
    file too, unless piz=True and the library has the PIZ entry points (Context.has_exr_piz)."""
    def __init__(self, ctx, source, names: dict | None = None, piz: bool = False, conventions=None):
        """conventions: the files are in an engine's conventions (rfx.h "AOV conventions") — one conventions.AovConventions for every frame, a
        list of them (one per frame: the cameras move), or a callable index -> AovConventions; set on the context before each frame is staged."""
        self.ctx, self.names, self.piz, self.conventions = ctx, names, piz, conventions
        self.paths = sorted(os.path.join(source, f) for f in os.listdir(source) if f.lower().endswith(".exr")) if isinstance(source, str) else list(source)
        self.buffers = [None, None]

    def __len__(self):
        return len(self.paths)

    def stage(self, index: int) -> str:
        """stage frame `index` (published by the next stage_flip) -> "device" or "host": the way it went"""
        path = self.paths[index]
        size = os.path.getsize(path)
        buf = self.buffers[index & 1]
        if buf is None or buf.size < size:  # grown with some room: frames of a sequence differ by a few per cent
            buf = self.buffers[index & 1] = self.ctx.host_alloc((size + size // 8,), np.uint8)
        with open(path, "rb", buffering=0) as f:
            got = f.readinto(memoryview(buf)[:size])
        if got != size:
            raise IOError("%s: read %d of %d bytes" % (path, got, size))
        conv = self.conventions
        if conv is not None:
            conv = conv(index) if callable(conv) else conv[index] if isinstance(conv, (list, tuple)) else conv
            self.ctx.set_aov_conventions(conv)
        try:
            self.ctx.stage_exr_device(buf[:size], self.names, self.piz)  # (the blocks form where the library has it: tiled, RLE and PXR24 files too)
            return "device"
        except imageio.ExrNotStreamable:
            return self.ctx.stage_exr_frame(path, "host", self.names)
