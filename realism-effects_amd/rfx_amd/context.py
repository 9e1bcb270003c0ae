"""Thin object wrapper over the C ABI (include/rfx.h): one `Context` = one `rfx_ctx` =
the device-side state of the pass chain on one GPU (or one row tile of it)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "data")


class RfxError(RuntimeError):
    pass


def load_blue_noise_table() -> np.ndarray:
    """128x128 RGBA8 table, decoded once from the reference's PNG asset, already flipY'd
    (tools/make_blue_noise_table.py; src/utils/BlueNoiseUtils.js:9-15)."""
    t = np.fromfile(os.path.join(DATA_DIR, "blue_noise_128_rgba8.bin"), np.uint8)
    assert t.size == 128 * 128 * 4
    return t.reshape(128, 128, 4)


_TENSOR_PLANE_TYPES = {"torch.float32": (abi.PLANE_F32, 4), "torch.float16": (abi.PLANE_F16, 2)}


def device_plane(tensor, rows: int, width: int, origin: str = "bottom") -> abi.DevicePlane:
    """A (rows, width, C) or (rows, width) tensor, float32 or float16, with ANY strides -> the abi.DevicePlane that addresses it where it lies:
    a permuted (C, H, W) tensor, a slice of a pitched buffer, an `expand`ed constant (strides 0).  origin "bottom": the tensor's row 0 is the
    band's first frame row (row 0 of the frame is its bottom row); "top": row 0 is the band's LAST frame row, as images are kept — a negative
    stride_y from the tensor's last row.  A pure function of the tensor's shape, strides, dtype and data_ptr(): it runs on CPU tensors too."""
    if origin not in ("bottom", "top"):
        raise ValueError("origin: \"bottom\" or \"top\"")
    shape, strides = tuple(int(n) for n in tensor.shape), tuple(int(s) for s in tensor.stride())
    if len(shape) == 2:
        shape, strides = shape + (1,), strides + (0,)
    if len(shape) != 3 or shape[:2] != (int(rows), int(width)):
        raise ValueError("device plane: a tensor of shape (%d, %d[, C]), got %s" % (rows, width, tuple(tensor.shape)))
    if str(tensor.dtype) not in _TENSOR_PLANE_TYPES:
        raise TypeError("device plane: a float32 or float16 tensor, got %s" % (tensor.dtype,))
    kind, elem = _TENSOR_PLANE_TYPES[str(tensor.dtype)]
    sy, sx, sc = strides
    ptr = int(tensor.data_ptr())
    if origin == "top":
        ptr, sy = ptr + (shape[0] - 1) * sy * elem, -sy
    return abi.DevicePlane(ptr, kind, shape[2], sx, sy, sc)


_TENSOR_IMAGE_FORMATS = {"torch.float32": (abi.EXPORT_F32, 4), "torch.float16": (abi.EXPORT_F16, 2), "torch.uint8": (abi.EXPORT_U8_SRGB, 1)}


def device_image(tensor, rows: int, width: int, origin: str = "bottom") -> abi.DeviceImage:
    """device_plane's twin for the way out: a WRITABLE (rows, width, C) tensor — float32, float16 or uint8, C = 3 or 4, ANY strides: a permuted
    (C, H, W) tensor, a slice of a pitched buffer — -> the abi.DeviceImage that Context.export_device writes where the tensor lies.  origin
    "bottom": the tensor's row 0 is the tile's first frame row (row 0 of the frame is its bottom row); "top": row 0 is the tile's LAST frame
    row, as images are kept — a negative stride_y from the tensor's last row.  The format an image is written in is export_device's `format`;
    the record remembers the tensor's (`image.format`) and export_device refuses another.  Whether the strides can be written without the
    image aliasing itself (an `expand`ed tensor cannot) is the library's rule: the call refuses.  A pure function of the tensor's shape,
    strides, dtype and data_ptr(): it runs on CPU tensors too."""
    if origin not in ("bottom", "top"):
        raise ValueError("origin: \"bottom\" or \"top\"")
    shape, strides = tuple(int(n) for n in tensor.shape), tuple(int(s) for s in tensor.stride())
    if len(shape) != 3 or shape[:2] != (int(rows), int(width)) or shape[2] not in (3, 4):
        raise ValueError("device image: a tensor of shape (%d, %d, 3 or 4), got %s" % (rows, width, tuple(tensor.shape)))
    if str(tensor.dtype) not in _TENSOR_IMAGE_FORMATS:
        raise TypeError("device image: a float32, float16 or uint8 tensor, got %s" % (tensor.dtype,))
    fmt, elem = _TENSOR_IMAGE_FORMATS[str(tensor.dtype)]
    sy, sx, sc = strides
    ptr = int(tensor.data_ptr())
    if origin == "top":
        ptr, sy = ptr + (shape[0] - 1) * sy * elem, -sy
    image = abi.DeviceImage(ptr, sx, sy, sc)
    image.format, image.channels = fmt, shape[2]  # (python attributes, not fields: what export_device holds its arguments against)
    return image


class Context:
    def __init__(self, width: int, height: int, device: int = 0, tile_y0: int = 0, tile_rows: int | None = None, halo_rows: int = 0):
        self.lib = abi.load_library()
        self.W, self.H = int(width), int(height)
        self.tile_y0 = int(tile_y0)
        self.tile_rows = int(tile_rows if tile_rows is not None else height - tile_y0)
        self.halo = int(halo_rows)
        self._h = self.lib.rfx_create(int(device), self.W, self.H, self.tile_y0, self.tile_rows, self.halo)
        if not self._h:
            raise RfxError("rfx_create failed: %s" % self.lib.rfx_last_error(None).decode())
        self.upload(abi.TEX_BLUE_NOISE, load_blue_noise_table(), 0, 128)

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self.lib.rfx_destroy(self._h)
            self._h = None
            self.__dict__.pop("_staged_keepalive", None)
            self.__dict__.pop("_export_keepalive", None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise RfxError("%s failed (%d): %s" % (what, rc, self.lib.rfx_last_error(self._h).decode()))

    # -- textures
    def held_rows(self, tex: int):
        r0, n = C.c_int(), C.c_int()
        self._chk(self.lib.rfx_tex_held_rows(self._h, tex, C.byref(r0), C.byref(n)), "rfx_tex_held_rows")
        return r0.value, n.value

    def upload(self, tex: int, array: np.ndarray, row0: int | None = None, rows: int | None = None):
        """Upload rows [row0, row0+rows) (FRAME rows; default = everything the context holds).
        `array` holds exactly those rows."""
        dtype, ch = abi.TEX_FORMAT[tex]
        h0, hn = self.held_rows(tex)
        row0 = h0 if row0 is None else row0
        rows = hn if rows is None else rows
        a = np.ascontiguousarray(array)
        if a.dtype != dtype:
            if a.dtype.itemsize == np.dtype(dtype).itemsize:
                a = a.view(dtype)
            else:
                raise TypeError("texture %s wants %s, got %s" % (abi.TEX_NAMES[tex], np.dtype(dtype), a.dtype))
        width = 128 if tex == abi.TEX_BLUE_NOISE else self.W
        if a.size != rows * width * ch:
            raise ValueError("texture %s: expected %d x %d x %d elements, got %s" % (abi.TEX_NAMES[tex], rows, width, ch, a.shape))
        self._chk(self.lib.rfx_upload(self._h, tex, a.ctypes.data_as(C.c_void_p), row0, rows), "rfx_upload")

    def download(self, tex: int, row0: int | None = None, rows: int | None = None) -> np.ndarray:
        dtype, ch = abi.TEX_FORMAT[tex]
        h0, hn = self.held_rows(tex)
        row0 = h0 if row0 is None else row0
        rows = hn if rows is None else rows
        width = 128 if tex == abi.TEX_BLUE_NOISE else self.W
        out = np.empty((rows, width, ch) if ch > 1 else (rows, width), dtype)
        self._chk(self.lib.rfx_download(self._h, tex, out.ctypes.data_as(C.c_void_p), row0, rows), "rfx_download")
        return out

    # -- streaming dumps (rfx.h "streaming dumps"): the next frame's planes cross PCIe while the current frame is drawn
    def host_alloc(self, shape, dtype) -> np.ndarray:
        """A pinned (hipHostMalloc) numpy array: what makes rfx_stage_upload asynchronous.  The memory lives as long as the array (or any
        view of it) does: it is freed by a finalizer of the buffer object the array is built on, not with the context."""
        import weakref
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.lib.rfx_host_alloc(n)
        if not p:
            raise RfxError("rfx_host_alloc(%d bytes) failed" % n)
        buf = (C.c_char * n).from_address(p)
        weakref.finalize(buf, self.lib.rfx_host_free, p)  # numpy keeps `buf` alive as the base of every view
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def stage_upload(self, tex: int, array: np.ndarray, row0: int | None = None, rows: int | None = None):
        """Asynchronous upload of rows [row0, row0+rows) into the slot's BACK buffer; published by stage_flip()."""
        h0, hn = self.held_rows(tex)
        row0 = h0 if row0 is None else row0
        rows = hn if rows is None else rows
        dtype, ch = abi.TEX_FORMAT[tex]
        a = array if array.flags["C_CONTIGUOUS"] else np.ascontiguousarray(array)
        if a.nbytes != rows * self.W * ch * np.dtype(dtype).itemsize:
            raise ValueError("texture %s: %d bytes do not cover %d rows" % (abi.TEX_NAMES[tex], a.nbytes, rows))
        self._keep_until_flip(a)
        self._chk(self.lib.rfx_stage_upload(self._h, tex, a.ctypes.data_as(C.c_void_p), row0, rows), "rfx_stage_upload")

    def stage_frame(self, frame):
        """Stage a whole dumped frame: its packed planes, or — a frame with `aov` instead of `gbuffer` — its attribute planes (stage_aov)."""
        if getattr(frame, "gbuffer", None) is None:
            conv = getattr(frame, "conventions", None)  # an engine-form frame (dump.read_dump): its conventions hold for this call
            if conv is not None:
                self.set_aov_conventions(conv)
                self.__dict__["_frame_conventions"] = True
            elif self.__dict__.pop("_frame_conventions", False):
                self.set_aov_conventions(None)
            planes = dict(frame.aov)
            planes["depth"] = frame.depth
            if getattr(frame, "direct", None) is not None:
                planes["direct"] = frame.direct
            if any(isinstance(v, abi.DevicePlane) for v in planes.values()):  # a frame that lives on the device
                self.stage_aov_device(planes)
            else:
                self.stage_aov(planes)
            return
        for tex, plane in ((abi.TEX_DEPTH, frame.depth), (abi.TEX_GBUFFER, frame.gbuffer), (abi.TEX_VELOCITY, frame.velocity),
                           (abi.TEX_DIRECT_LIGHT, frame.direct)):
            r0, n = self.held_rows(tex)
            self.stage_upload(tex, plane[r0:r0 + n] if plane.shape[0] != n else plane, r0, n)

    # -- streamed AOV frames (rfx.h "streamed AOV frames"): the importer's planes staged once and packed on the upload stream
    def _aov_frame(self, planes: dict, row0, rows):
        """-> (abi.AovFrame, row0, rows, the arrays it points into).  `planes`: name -> array of the band's rows; the type comes from the
        dtype (float32 / float16), the channel count from the size."""
        row0 = 0 if row0 is None else int(row0)
        rows = self.H - row0 if rows is None else int(rows)
        planes = self._aov_named(planes)
        f, keep = abi.AovFrame(), []
        texels = max(rows, 0) * self.W
        for name in abi.AOV_PLANES:
            a = planes.get(name)
            if a is None:
                continue
            if not isinstance(a, np.ndarray) or a.dtype not in abi.PLANE_TYPES:
                raise TypeError("AOV plane %s: a float32 or float16 ndarray, got %s" % (name, getattr(a, "dtype", type(a))))
            a = a if a.flags["C_CONTIGUOUS"] else np.ascontiguousarray(a)
            if texels == 0 or a.size % texels:
                raise ValueError("AOV plane %s: %s does not cover %d rows of %d texels" % (name, a.shape, rows, self.W))
            keep.append(a)
            setattr(f, name, abi.Plane(a.ctypes.data, abi.PLANE_TYPES[a.dtype], a.size // texels))
        return f, row0, rows, keep

    @staticmethod
    def _aov_named(planes: dict) -> dict:
        """the planes under rfx_aov_frame's names: `position` / `view_z` are the depth plane under the conventions set"""
        alias = [k for k in ("depth", "position", "view_z") if planes.get(k) is not None]
        if len(alias) > 1:
            raise ValueError("AOV frame: %s are one plane (the depth plane under the conventions set)" % " and ".join(alias))
        if alias and alias[0] != "depth":  # set_aov_conventions says which of the three the library takes the depth plane for
            planes = {("depth" if k == alias[0] else k): v for k, v in planes.items() if k not in ("depth", "position", "view_z") or k == alias[0]}
        unknown = set(planes) - set(abi.AOV_PLANES)
        if unknown:
            raise ValueError("AOV frame: unknown planes %s" % sorted(unknown))
        return planes

    # -- device planes (rfx.h "device planes"): the AOV frame of a renderer on the same device, read where it lies
    @property
    def has_stage_aov_device(self) -> bool:
        """the library exports rfx_stage_aov_device (additive to ABI 21)"""
        return hasattr(self.lib, "rfx_stage_aov_device")

    def _aov_device_frame(self, planes: dict, row0, rows):
        """-> (abi.AovDeviceFrame, row0, rows).  `planes`: name -> abi.DevicePlane of the band's rows"""
        row0, rows = self._band(row0, rows)
        planes = self._aov_named(planes)
        f = abi.AovDeviceFrame()
        for name in abi.AOV_PLANES:
            v = planes.get(name)
            if v is None:
                continue
            if not isinstance(v, abi.DevicePlane):
                raise TypeError("device AOV plane %s: an abi.DevicePlane (context.device_plane makes one of a tensor), got %s" % (name, type(v)))
            setattr(f, name, v)
        return f, row0, rows

    def stage_aov_device(self, planes: dict, row0: int | None = None, rows: int | None = None, *, producer: int | None = None):
        """rfx_stage_aov_device: stage_aov for planes that already live on the device — nothing crosses PCIe, the pack kernel reads them where
        they lie.  Values: abi.DevicePlane records (a device address and element strides of any sign, 0 for a broadcast); device_plane() makes
        one of a torch tensor of shape (rows, W, C) or (rows, W) with any strides.  `position=` / `view_z=` as in stage_aov.  The planes are
        complete when the call is made (synchronise the stream that produced them) — or `producer=` names the stream that writes them (an
        integer hipStream_t handle, non-zero): queue_wait_stream(QUEUE_UPLOAD, producer) runs first and the host does not wait.  The caller
        keeps the planes alive and unchanged until the flip after the publishing one has returned (stream_wait_queue(QUEUE_UPLOAD, producer)
        orders the producer's next writes behind the pack kernel)."""
        if not self.has_stage_aov_device:
            raise RfxError("this librfx_hip.so has no rfx_stage_aov_device")
        if producer is not None:
            producer = self._stream_handle("stage_aov_device(producer=)", producer)
        f, row0, rows = self._aov_device_frame(planes, row0, rows)
        if producer is not None:
            self.queue_wait_stream(abi.QUEUE_UPLOAD, producer)
        self._chk(self.lib.rfx_stage_aov_device(self._h, C.byref(f), row0, rows, None), "rfx_stage_aov_device")

    # -- device images and stream ordering (rfx.h): the export that stays on the device, the context's queues against a caller's stream
    @property
    def has_export_device(self) -> bool:
        """the library exports rfx_export_device, rfx_queue_wait_stream and rfx_stream_wait_queue (additive to ABI 21)"""
        return hasattr(self.lib, "rfx_export_device")

    @staticmethod
    def _stream_handle(what, stream) -> int:
        """a hipStream_t as an integer, e.g. torch.cuda.current_stream().cuda_stream; 0 is the legacy default stream, which cannot be named"""
        if isinstance(stream, bool) or not isinstance(stream, int):
            raise TypeError("%s: an integer hipStream_t handle, got %s" % (what, type(stream)))
        if stream == 0:
            raise ValueError("%s: 0 is the legacy default stream, which cannot be named: create a stream" % what)
        return stream

    def _need_export_device(self, what):
        if not self.has_export_device:
            raise RfxError("%s: this librfx_hip.so has no rfx_export_device (Context.has_export_device)" % what)

    def queue_wait_stream(self, queue: int, stream: int):
        """rfx_queue_wait_stream: the context's queue (abi.QUEUE_DRAW / QUEUE_UPLOAD) waits for what `stream` holds now; the host does not"""
        self._need_export_device("queue_wait_stream")
        self._chk(self.lib.rfx_queue_wait_stream(self._h, int(queue), C.c_void_p(self._stream_handle("queue_wait_stream", stream))), "rfx_queue_wait_stream")

    def stream_wait_queue(self, queue: int, stream: int):
        """rfx_stream_wait_queue: `stream` waits for what the context's queue holds now; the host does not"""
        self._need_export_device("stream_wait_queue")
        self._chk(self.lib.rfx_stream_wait_queue(self._h, int(queue), C.c_void_p(self._stream_handle("stream_wait_queue", stream))), "rfx_stream_wait_queue")

    def export_device(self, source: int, format, channels: int = 3, tonemap="linear", exposure: float = 1.0, *, image: abi.DeviceImage, stream: int | None = None):
        """rfx_export_device: export()'s elements, bit for bit, encoded on the draw stream straight into `image` — an abi.DeviceImage (a device
        address and element strides of any sign; device_image() makes one of a writable torch tensor).  Nothing crosses PCIe, no ticket is taken
        and the host does not wait: the image is complete once the draw stream has run the encode.  `stream=` (an integer hipStream_t handle,
        non-zero) names the consumer's stream: the encode waits for what that stream holds now (its last reads of the image) and the stream
        waits for the encode — queue_wait_stream(QUEUE_DRAW, stream) before, stream_wait_queue(QUEUE_DRAW, stream) after."""
        self._need_export_device("export_device")
        if not isinstance(image, abi.DeviceImage):
            raise TypeError("export_device: image must be an abi.DeviceImage (context.device_image makes one of a tensor), got %s" % (type(image),))
        p = self.export_params(source, format, channels, tonemap, exposure)
        if getattr(image, "format", p.format) != p.format or getattr(image, "channels", p.channels) != p.channels:
            raise ValueError("export_device: the image was made of a tensor of another dtype or channel count than format %r, channels %d" % (format, channels))
        if stream is not None:
            stream = self._stream_handle("export_device(stream=)", stream)
            self.queue_wait_stream(abi.QUEUE_DRAW, stream)
        self._chk(self.lib.rfx_export_device(self._h, C.byref(p), C.byref(image)), "rfx_export_device")
        if stream is not None:
            self.stream_wait_queue(abi.QUEUE_DRAW, stream)

    # -- AOV conventions (rfx.h "AOV conventions"): the planes as engines write them, converted by the pack kernel
    @property
    def has_aov_conventions(self) -> bool:
        """the library exports rfx_set_aov_conventions (additive to ABI 21)"""
        return hasattr(self.lib, "rfx_set_aov_conventions")

    def set_aov_conventions(self, conv=None):
        """rfx_set_aov_conventions: what the next stage_aov / stage_exr_aov / stage_exr_blocks calls take their depth, velocity and normal planes
        for (conventions.AovConventions, or an abi.AovConventions); None: the default.  Set per frame: the matrices change."""
        if not self.has_aov_conventions:
            raise RfxError("this librfx_hip.so has no rfx_set_aov_conventions")
        c = conv.to_abi() if hasattr(conv, "to_abi") else conv
        self._chk(self.lib.rfx_set_aov_conventions(self._h, None if c is None else C.byref(c)), "rfx_set_aov_conventions")

    def aov_stage_bytes(self, planes: dict, row0: int | None = None, rows: int | None = None) -> int:
        """rfx_aov_stage_bytes: the bytes stage_aov(planes, row0, rows) copies host -> device (0: the library would refuse the frame)"""
        f, row0, rows, _ = self._aov_frame(planes, row0, rows)
        return int(self.lib.rfx_aov_stage_bytes(self._h, C.byref(f), row0, rows))

    def stage_aov(self, planes: dict, row0: int | None = None, rows: int | None = None):
        """rfx_stage_aov: the attribute planes of rows [row0, row0+rows) of the FRAME (default: all of it) -> the back buffers of DEPTH and of
        the slots the planes name (GBUFFER: diffuse, normal, roughness, metalness, emissive; VELOCITY: velocity, normal; DIRECT_LIGHT: direct);
        published by stage_flip().  host_alloc() planes make the copies asynchronous.  With set_aov_conventions the depth plane may be given
        as `position` (3 channels, depth_kind "position") or `view_z` (depth_kind "view_z") instead of `depth`."""
        f, row0, rows, keep = self._aov_frame(planes, row0, rows)
        self._keep_until_flip(*keep)
        self._chk(self.lib.rfx_stage_aov(self._h, C.byref(f), row0, rows), "rfx_stage_aov")

    # -- streamed EXR frames (rfx.h "streamed EXR frames"): the file's chunks cross PCIe packed and are decoded on the device
    # -- EXR blocks (rfx.h "EXR blocks"): the same for tiled parts, RLE and PXR24, a moved data window
    _EXR_FORMS = {"chunks": (abi.EXR_CHUNK_DTYPE, abi.ExrChunk, abi.ExrFrame), "blocks": (abi.EXR_BLOCK_DTYPE, abi.ExrBlock, abi.ExrBlockFrame)}

    def _exr_frame(self, buf, layout, form="chunks"):
        """-> (abi.ExrFrame — abi.ExrBlockFrame for form "blocks" —, the objects it points into).  `buf`: the file's bytes (bytes, or a uint8
        array — host_alloc() makes the copies asynchronous); `layout`: imageio.exr_aov_layout of the same bytes, with forms="blocks" for "blocks"."""
        if (layout.width, layout.height) != (self.W, self.H):
            raise ValueError("EXR frame of %d x %d on a context of %d x %d" % (layout.width, layout.height, self.W, self.H))
        a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
        if not a.flags["C_CONTIGUOUS"] or a.nbytes < layout.file_bytes:
            raise ValueError("EXR frame: a contiguous buffer of the file's %d bytes" % layout.file_bytes)
        dtype, record, frame = self._EXR_FORMS[form]
        # (built per call from what the layout holds now: the part list is a few words, the chunk / block records are handed over as they are)
        chans = [(abi.ExrChannel * len(ch))(*[abi.ExrChannel(pt, pl, comp) for pt, pl, comp in ch]) for _, ch in layout.parts]
        parts = (abi.ExrPart * len(layout.parts))(*[abi.ExrPart(comp, len(ch), arr) for (comp, ch), arr in zip(layout.parts, chans)])
        records = np.ascontiguousarray(getattr(layout, form), dtype)
        f = frame(a.ctypes.data, layout.file_bytes, len(parts), len(records), parts, records.ctypes.data_as(C.POINTER(record)))
        return f, (a, (chans, parts, records))

    def _exr_block_frame(self, buf, layout):
        """_exr_frame for a layout of blocks (imageio.exr_aov_layout(..., forms="blocks")): the name the descriptor of the blocks calls keeps"""
        return self._exr_frame(buf, layout, "blocks")

    def _band(self, row0, rows):
        row0 = 0 if row0 is None else int(row0)
        return row0, (self.H - row0 if rows is None else int(rows))

    def _keep_until_flip(self, *objects):
        """what the staged copies of this batch read: alive until they have executed (stage_flip keeps this batch and the one before)"""
        self.__dict__.setdefault("_staged_now", []).extend(objects)

    def exr_aov_stage_bytes(self, buf, layout, row0: int | None = None, rows: int | None = None) -> int:
        """rfx_exr_aov_stage_bytes: the bytes stage_exr_aov(buf, layout, row0, rows) copies host -> device (0: the library would refuse the frame)"""
        f, _ = self._exr_frame(buf, layout)
        return int(self.lib.rfx_exr_aov_stage_bytes(self._h, C.byref(f), *self._band(row0, rows)))

    def stage_exr_aov(self, buf, layout, row0: int | None = None, rows: int | None = None):
        """rfx_stage_exr_aov: stage_aov for a frame that is still an OpenEXR file — the chunks of rows [row0, row0+rows) of the FRAME (default:
        all of it) are copied as they sit in `buf` and inflated, unpredicted and scattered on the device; published by stage_flip()."""
        f, keep = self._exr_frame(buf, layout)
        self._keep_until_flip(keep[0])
        self._chk(self.lib.rfx_stage_exr_aov(self._h, C.byref(f), *self._band(row0, rows)), "rfx_stage_exr_aov")

    def exr_aov_status(self):
        """rfx_exr_aov_status -> (bad chunks, index of the first bad chunk in layout.chunks or -1, its k9_inflate.h error code or 0); waits for
        the decode of the most recent stage_exr_aov"""
        bad, first, code = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.rfx_exr_aov_status(self._h, C.byref(bad), C.byref(first), C.byref(code)), "rfx_exr_aov_status")
        return bad.value, first.value, code.value

    @property
    def has_exr_blocks(self) -> bool:
        """the library exports rfx_stage_exr_blocks (additive to ABI 21)"""
        return hasattr(self.lib, "rfx_stage_exr_blocks")

    @property
    def has_exr_piz(self) -> bool:
        """the library exports rfx_stage_exr_blocks_piz (additive to ABI 21): PIZ parts in a layout of blocks"""
        return hasattr(self.lib, "rfx_stage_exr_blocks_piz")

    def _blocks_symbol(self, layout, plain: str, piz: str) -> str:
        """`piz` for a layout with a PIZ part on a library that has the entry points, else `plain`"""
        return piz if self.has_exr_piz and any(comp == abi.EXR_PIZ for comp, _ in layout.parts) else plain

    def exr_blocks_stage_bytes(self, buf, layout, row0: int | None = None, rows: int | None = None) -> int:
        """rfx_exr_blocks_stage_bytes (rfx_exr_blocks_piz_stage_bytes for a layout with a PIZ part): the bytes stage_exr_blocks(buf, layout, row0,
        rows) copies host -> device (0: the library would refuse the frame)"""
        f, _ = self._exr_block_frame(buf, layout)
        name = self._blocks_symbol(layout, "rfx_exr_blocks_stage_bytes", "rfx_exr_blocks_piz_stage_bytes")
        return int(getattr(self.lib, name)(self._h, C.byref(f), *self._band(row0, rows)))

    def stage_exr_blocks(self, buf, layout, row0: int | None = None, rows: int | None = None):
        """rfx_stage_exr_blocks: stage_exr_aov for a layout of blocks — scanline chunks and tiles, NONE / RLE / ZIPS / ZIP / PXR24; exr_aov_status()
        reports on the most recent call of either.  A layout with a PIZ part (imageio.exr_aov_layout(..., forms="blocks", piz=True)) goes through
        rfx_stage_exr_blocks_piz where the library has it (has_exr_piz)."""
        f, keep = self._exr_block_frame(buf, layout)
        self._keep_until_flip(keep[0])
        name = self._blocks_symbol(layout, "rfx_stage_exr_blocks", "rfx_stage_exr_blocks_piz")
        self._chk(getattr(self.lib, name)(self._h, C.byref(f), *self._band(row0, rows)), name)

    def stage_exr_device(self, buf, names: dict | None = None, piz: bool = False, conventions=None):
        """One whole AOV EXR file held in `buf` through the device decode: the blocks form where the library has it, else the scanline form.
        piz=True: PIZ parts too, where the library has rfx_stage_exr_blocks_piz.  imageio.ExrNotStreamable: the file is one neither takes.
        conventions: this frame's conventions.AovConventions, set before the call (the context keeps them until the next set)."""
        from . import imageio
        if conventions is not None:
            self.set_aov_conventions(conventions)
        if self.has_exr_blocks:
            self.stage_exr_blocks(buf, imageio.exr_aov_layout(buf, names, forms="blocks", piz=piz and self.has_exr_piz))
        else:
            self.stage_exr_aov(buf, imageio.exr_aov_layout(buf, names))

    def stage_exr_frame(self, path: str, decode: str = "host", names: dict | None = None, piz: bool = False, conventions=None):
        """Stage a whole AOV EXR file.  decode="host" (the default): imageio.exr_to_typed_planes + stage_aov.  decode="device": the file's bytes
        + stage_exr_blocks (stage_exr_aov on a library without it); a file the device decode does not take (imageio.ExrNotStreamable: PIZ, deep
        data, UINT channels, ...) goes the host's way.  piz=True (with decode="device"): a PIZ file is decoded on the device too where the library
        has the entry points (has_exr_piz); the default keeps it on the host.
        conventions: this frame's conventions.AovConventions (names= then maps `position` / `view_z`), set before the planes are staged.
        -> the way taken, "host" or "device"."""
        from . import imageio
        if decode not in ("host", "device"):
            raise ValueError("decode: \"host\" or \"device\"")
        if conventions is not None:
            self.set_aov_conventions(conventions)
        if decode == "device":
            with open(path, "rb") as f:
                data = f.read()
            try:
                self.stage_exr_device(data, names, piz)
                return "device"
            except imageio.ExrNotStreamable:
                pass
        t = imageio.exr_to_typed_planes(path, names)
        self.stage_aov(dict(t["aov"], depth=t["depth"], direct=t["direct"]))
        return "host"

    def stage_flip(self):
        self._chk(self.lib.rfx_stage_flip(self._h), "rfx_stage_flip")
        # rfx_stage_flip returns when the copies published by the PREVIOUS flip have executed: keep this batch's planes and the one before
        gens = self.__dict__.setdefault("_staged_keepalive", [])
        gens.append(self.__dict__.pop("_staged_now", []))
        del gens[:-2]

    # -- streamed frame export (rfx.h "streamed frame export"): the encode runs on the device, only the encoded bytes cross PCIe
    @staticmethod
    def export_params(source: int, format, channels: int = 3, tonemap="linear", exposure: float = 1.0) -> abi.ExportParams:
        """`format`: "f32" / "f16" / "u8_srgb" or abi.EXPORT_*; `tonemap`: "linear" / "aces" (imageio.tonemap's operators) or 0 / 1"""
        return abi.ExportParams(int(source), int(abi.EXPORT_FORMATS.get(format, format)), int(channels), int(abi.EXPORT_TONEMAP.get(tonemap, tonemap)),
                                float(exposure))

    def export_bytes(self, p: abi.ExportParams) -> int:
        return int(self.lib.rfx_export_bytes(self._h, C.byref(p)))

    @staticmethod
    def _out_buffer(what, out, n, dtype, shape):
        """The result buffer of an encode call: a new array of `shape` and `dtype`, or the caller's `out` checked to be `n` bytes of `dtype`.
        n == 0 (bad params): any non-empty buffer will do, the library names the fault."""
        if out is None:
            return np.empty(shape if n else (1,), dtype)
        if not isinstance(out, np.ndarray) or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise TypeError("%s: out must be a writeable C-contiguous ndarray" % what)
        if n and (out.dtype != dtype or out.nbytes != n):
            raise ValueError("%s: out must hold %d bytes of %s, got %d of %s" % (what, n, np.dtype(dtype), out.nbytes, out.dtype))
        return out

    def _keep_until_retired(self, ticket: int, out):
        """the copy of a staged export writes `out` until its ticket retires (export_wait), or two later tickets exist"""
        keep = self.__dict__.setdefault("_export_keepalive", {})
        keep[ticket] = out
        for old in [k for k in keep if k <= ticket - 2]:
            del keep[old]

    _ENCODE_BOUND = {"export": "rfx_export_bytes", "png": "rfx_png_bound", "exr": "rfx_exr_bound"}

    def _encode(self, kind: str, p: abi.ExportParams, out, staged: bool, filter=None, matches: bool = False):
        """export / png / exr and their stage_ forms: rfx_[stage_]<kind>[_ex].  -> the result buffer, or the ticket of a staged call.
        Only png's symbols take `filter`, only the _ex ones (matches=True: rfx.h "Match form") the flags."""
        what = ("stage_" if staged else "") + kind
        n = int(getattr(self.lib, self._ENCODE_BOUND[kind])(self._h, C.byref(p)))
        if kind == "export":
            out = self._out_buffer(what, out, n, abi.EXPORT_DTYPE.get(p.format, np.uint8), (self.tile_rows, self.W, p.channels))
        else:
            out = self._out_buffer(what, out, n, np.uint8, (n,))
        if matches:
            self._need_matches(what)
        name = "rfx_" + what + ("_ex" if matches else "")
        args, ticket = [self._h, C.byref(p)], C.c_int(0)
        if kind == "png":
            args.append(int(abi.PNG_FILTERS.get(filter, filter)))
        if matches:
            args.append(abi.ENCODE_MATCHES)
        args += [out.ctypes.data_as(C.c_void_p), n]
        if staged:
            args.append(C.byref(ticket))
        self._chk(getattr(self.lib, name)(*args), name)
        if not staged:
            return out
        self._keep_until_retired(ticket.value, out)
        return int(ticket.value)

    def export(self, source: int, format, channels: int = 3, tonemap="linear", exposure: float = 1.0, out=None) -> np.ndarray:
        """rfx_export: the context's tile rows of `source`, encoded on the device -> (rows, W, channels) uint8 / float16 / float32, row 0 =
        bottom (the order download() uses).  Blocks until the bytes are there."""
        p = self.export_params(source, format, channels, tonemap, exposure)
        return self._encode("export", p, out, False).reshape(self.tile_rows, self.W, p.channels)

    def stage_export(self, source: int, format, channels: int = 3, tonemap="linear", exposure: float = 1.0, *, out: np.ndarray) -> int:
        """rfx_stage_export: enqueue the encode (after every draw enqueued so far) and the copy into `out` — a host_alloc() array for an
        asynchronous copy — and return the ticket.  `out` is complete once export_wait(ticket) has returned; the call itself returns only when
        the export two tickets earlier has completed (alternate two buffers)."""
        return self._encode("export", self.export_params(source, format, channels, tonemap, exposure), out, True)

    def export_wait(self, ticket: int):
        self._chk(self.lib.rfx_export_wait(self._h, int(ticket)), "rfx_export_wait")
        self.__dict__.get("_export_keepalive", {}).pop(int(ticket), None)

    # -- rfx.h "Match form": the device encode with run-length matches, per call (matches=True on png / stage_png / exr / stage_exr)
    @property
    def has_export_matches(self) -> bool:
        """the library exports rfx_stage_png_ex and its three companions (additive to ABI 21)"""
        return hasattr(self.lib, "rfx_stage_png_ex")

    def _need_matches(self, what):
        if not self.has_export_matches:
            raise RuntimeError("%s(matches=True): this librfx_hip.so has no rfx_stage_png_ex (Context.has_export_matches)" % what)

    # -- PNG fragments (rfx.h "PNG fragments"): the same export, encoded on the device as the IDAT chunks of the tile rows
    def png_bound(self, channels: int = 3) -> int:
        """rfx_png_bound: the bytes of a result buffer (32-byte header + the fragment at its largest)"""
        return int(self.lib.rfx_png_bound(self._h, C.byref(self.export_params(abi.TEX_FINAL, "u8_srgb", channels))))

    def png(self, source: int, channels: int = 3, tonemap="linear", exposure: float = 1.0, filter=0, out=None, matches: bool = False) -> np.ndarray:
        """rfx_png: the tile rows of `source` as a PNG fragment -> the result buffer (png_bound() bytes of uint8: header, fragment, slack);
        imageio.png_from_fragments wraps one or more of them into a file.  `filter`: "adaptive" / "none" / "sub" / "up" / "paeth" or 0..4.
        matches=True: rfx_png_ex with RFX_ENCODE_MATCHES (rfx.h "Match form").  Blocks until the bytes are there."""
        return self._encode("png", self.export_params(source, "u8_srgb", channels, tonemap, exposure), out, False, filter, matches)

    def stage_png(self, source: int, channels: int = 3, tonemap="linear", exposure: float = 1.0, filter=0, *, out: np.ndarray, matches: bool = False) -> int:
        """rfx_stage_png: stage_export's contract with a PNG fragment as the payload; the ticket is one of the same sequence and
        export_wait(ticket) retires it.  matches=True: rfx_stage_png_ex with RFX_ENCODE_MATCHES."""
        return self._encode("png", self.export_params(source, "u8_srgb", channels, tonemap, exposure), out, True, filter, matches)

    # -- EXR fragments (rfx.h "EXR fragments"): the F16 export, encoded on the device as the ZIPS chunks of the tile rows
    def exr_bound(self, channels: int = 4) -> int:
        """rfx_exr_bound: the bytes of a result buffer (32-byte header + the fragment at its largest)"""
        return int(self.lib.rfx_exr_bound(self._h, C.byref(self.export_params(abi.TEX_FINAL, "f16", channels))))

    def exr(self, source: int, channels: int = 4, out=None, matches: bool = False) -> np.ndarray:
        """rfx_exr: the tile rows of `source` as an EXR fragment -> the result buffer (exr_bound() bytes of uint8: header, fragment, slack);
        imageio.exr_from_fragments wraps one or more of them into a file.  matches=True: rfx_exr_ex with RFX_ENCODE_MATCHES (rfx.h "Match form").
        Blocks until the bytes are there."""
        return self._encode("exr", self.export_params(source, "f16", channels), out, False, matches=matches)

    def stage_exr(self, source: int, channels: int = 4, *, out: np.ndarray, matches: bool = False) -> int:
        """rfx_stage_exr: stage_export's contract with an EXR fragment as the payload; the ticket is one of the same sequence and
        export_wait(ticket) retires it.  matches=True: rfx_stage_exr_ex with RFX_ENCODE_MATCHES."""
        return self._encode("exr", self.export_params(source, "f16", channels), out, True, matches=matches)

    def clear(self, tex: int):
        self._chk(self.lib.rfx_clear(self._h, tex), "rfx_clear")

    def device_ptr(self, tex: int) -> int:
        p = self.lib.rfx_tex_device_ptr(self._h, tex)
        if not p:
            raise RfxError("rfx_tex_device_ptr: %s" % self.lib.rfx_last_error(self._h).decode())
        return p

    def bind_external(self, tex: int, device_ptr: int):
        self._chk(self.lib.rfx_bind_external(self._h, tex, C.c_void_p(device_ptr)), "rfx_bind_external")

    def set_stream(self, hip_stream: int | None):
        self._chk(self.lib.rfx_set_stream(self._h, C.c_void_p(hip_stream or 0)), "rfx_set_stream")

    def upload_frame(self, frame):
        """Upload a dumped frame (rfx_amd.scene.Frame or any object with depth/gbuffer/velocity/direct)
        whose planes cover the FULL frame; each slot takes the band it holds."""
        for tex, plane in ((abi.TEX_DEPTH, frame.depth), (abi.TEX_GBUFFER, frame.gbuffer), (abi.TEX_VELOCITY, frame.velocity),
                           (abi.TEX_DIRECT_LIGHT, frame.direct)):
            r0, n = self.held_rows(tex)
            self.upload(tex, plane[r0:r0 + n], r0, n)

    # -- importer: engine-side attribute planes -> packed render targets, on the device
    @staticmethod
    def _plane(a, ch, rows, width):
        a = np.ascontiguousarray(a, np.float32)  # (a float16 plane of a typed frame is widened here: exact)
        if ch == 4 and a.size == rows * width * 3:  # an rgb diffuse plane: alpha 1 (imageio.exr_to_dump_planes' rule)
            a = np.concatenate([a.reshape(rows, width, 3), np.ones((rows, width, 1), np.float32)], -1)
        if a.size != rows * width * ch:
            raise ValueError("AOV plane: expected %d x %d x %d floats, got %s" % (rows, width, ch, a.shape))
        return a

    def pack_gbuffer(self, aov: dict, depth=None, row0: int | None = None, rows: int | None = None):
        """rfx_pack_gbuffer: `aov` holds diffuse (RGBA), normal (xyz, world), roughness, metalness, emissive (rgb) planes of the band
        [row0, row0+rows) (default: everything the context holds); `depth` (1.0 = not covered) may be None."""
        h0, hn = self.held_rows(abi.TEX_GBUFFER)
        row0, rows = (h0 if row0 is None else row0), (hn if rows is None else rows)
        keep = [self._plane(aov[k], ch, rows, self.W) for k, ch in (("diffuse", 4), ("normal", 3), ("roughness", 1), ("metalness", 1), ("emissive", 3))]
        d = self._plane(depth, 1, rows, self.W) if depth is not None else None
        ptr = lambda a: a.ctypes.data_as(abi.FP) if a is not None else None
        s = abi.AovGBuffer(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), ptr(d))
        self._chk(self.lib.rfx_pack_gbuffer(self._h, C.byref(s), row0, rows), "rfx_pack_gbuffer")

    def pack_velocity(self, aov: dict, depth, row0: int | None = None, rows: int | None = None):
        h0, hn = self.held_rows(abi.TEX_VELOCITY)
        row0, rows = (h0 if row0 is None else row0), (hn if rows is None else rows)
        v, n, d = self._plane(aov["velocity"], 2, rows, self.W), self._plane(aov["normal"], 3, rows, self.W), self._plane(depth, 1, rows, self.W)
        s = abi.AovVelocity(v.ctypes.data_as(abi.FP), n.ctypes.data_as(abi.FP), d.ctypes.data_as(abi.FP))
        self._chk(self.lib.rfx_pack_velocity(self._h, C.byref(s), row0, rows), "rfx_pack_velocity")

    def set_environment(self, rgba, half_float_type=True, half_store_rtz=True):
        """scene.environment: an (H, W, 4) float32 equirectangular map (row 0 = bottom), or None to remove it."""
        if rgba is None:
            self._chk(self.lib.rfx_set_environment(self._h, None, 0, 0, 0, 0), "rfx_set_environment")
            self._env_size = None
            return
        a = np.ascontiguousarray(rgba, np.float32)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("environment map must be (H, W, 4)")
        self._chk(self.lib.rfx_set_environment(self._h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0], 1 if half_float_type else 0,
                                               1 if half_store_rtz else 0), "rfx_set_environment")
        self._env_size = (a.shape[1], a.shape[0])  # (download_environment_importance)

    def set_environment_importance(self, marginal, conditional, total_sum: float):
        """The tables of EquirectHdrInfoUniform.updateFrom (rfx_amd.envmap.build_importance) for importanceSampling; totalSumValue is split the
        way the reference splits it for its uniform struct (`~~total` and the rest, :391-394)."""
        m = np.ascontiguousarray(marginal, np.float32)
        c = np.ascontiguousarray(conditional, np.float32)
        whole = float(int(total_sum))
        # the library checks the counts against the environment's size (height / width*height floats)
        self._chk(self.lib.rfx_set_environment_importance(self._h, m.ctypes.data_as(C.c_void_p), m.size, c.ctypes.data_as(C.c_void_p), c.size, whole,
                                                          float(total_sum - whole)), "rfx_set_environment_importance")

    def download_environment(self, level: int, size) -> np.ndarray:
        """Mip level `level` of the environment; `size` = (width, height) of the base level."""
        w, h = max(size[0] >> level, 1), max(size[1] >> level, 1)
        out = np.empty((h, w, 4), np.float32)
        self._chk(self.lib.rfx_download_environment(self._h, level, out.ctypes.data_as(C.c_void_p), None), "rfx_download_environment")
        return out

    def cube_to_equirect(self, faces, width: int, height: int, generate_mipmaps: bool = False) -> np.ndarray:
        """CubeToEquirectEnvPass's draw + read-back (rfx_cube_to_equirect): faces (6, S, S, 4) float32 (+X -X +Y -Y +Z -Z, row j = t as
        uploaded) -> (height, width, 4) float32, row 0 = bottom."""
        faces = np.ascontiguousarray(faces, np.float32)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 4:
            raise ValueError("cube_to_equirect: faces must be (6, S, S, 4) float32")
        out = np.empty((int(height), int(width), 4), np.float32)
        self._chk(self.lib.rfx_cube_to_equirect(self._h, faces.ctypes.data_as(C.c_void_p), faces.shape[1], 1 if generate_mipmaps else 0,
                                                out.ctypes.data_as(C.c_void_p), int(width), int(height)), "rfx_cube_to_equirect")
        return out

    @property
    def has_env_device(self) -> bool:
        """the library keeps environment updates on the device (rfx_set_environment_cube / rfx_build_environment_importance: additive to ABI 21)"""
        return hasattr(self.lib, "rfx_build_environment_importance")

    def _need_env_device(self, what):
        if not self.has_env_device:
            raise RuntimeError("%s: this librfx_hip.so has no rfx_build_environment_importance (Context.has_env_device)" % what)

    def set_environment_cube(self, faces, width: int, height: int, generate_mipmaps: bool = False):
        """cube_to_equirect + set_environment(..., half_float_type=False, half_store_rtz=False) with the equirectangular map never leaving the
        device (rfx_set_environment_cube): stream-ordered, `faces` may be reused on return.  Invalidates the importance tables."""
        self._need_env_device("set_environment_cube")
        faces = np.ascontiguousarray(faces, np.float32)
        if faces.ndim != 4 or faces.shape[0] != 6 or faces.shape[1] != faces.shape[2] or faces.shape[3] != 4:
            raise ValueError("set_environment_cube: faces must be (6, S, S, 4) float32")
        self._chk(self.lib.rfx_set_environment_cube(self._h, faces.ctypes.data_as(C.c_void_p), faces.shape[1], 1 if generate_mipmaps else 0,
                                                    int(width), int(height)), "rfx_set_environment_cube")
        self._env_size = (int(width), int(height))

    def build_environment_importance(self, flip_y: bool = False):
        """The tables and sums of rfx_amd.envmap.build_importance, built on the device from level 0 of the held environment (K10), bit for bit;
        `flip_y`: the texture's flipY (what the hosts pass build_importance as `texels[::-1], True`).  Stream-ordered."""
        self._need_env_device("build_environment_importance")
        self._chk(self.lib.rfx_build_environment_importance(self._h, 1 if flip_y else 0), "rfx_build_environment_importance")

    def download_environment_importance(self):
        """(marginalWeights float32[H], conditionalWeights float32[H, W], totalSumValue, whole, decimal) as the context holds them.  Synchronises."""
        self._need_env_device("download_environment_importance")
        size = self.__dict__.get("_env_size")
        if size is None:
            raise RfxError("download_environment_importance: no environment set")
        m, c = np.empty(int(size[1]), np.float32), np.empty((int(size[1]), int(size[0])), np.float32)
        total, whole, dec = C.c_double(), C.c_float(), C.c_float()
        self._chk(self.lib.rfx_download_environment_importance(self._h, m.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), C.byref(total),
                                                               C.byref(whole), C.byref(dec)), "rfx_download_environment_importance")
        return m, c, total.value, np.float32(whole.value), np.float32(dec.value)

    def environment_levels(self) -> int:
        n = C.c_int()
        self._chk(self.lib.rfx_download_environment(self._h, 0, None, C.byref(n)), "rfx_download_environment")
        return n.value

    def set_row_window(self, y0: int = 0, y1: int = 0):
        """Restrict the rows the following draws produce to [y0, y1); no arguments (or y1 <= y0) resets (rfx_set_row_window)."""
        self._chk(self.lib.rfx_set_row_window(self._h, int(y0), int(y1)), "rfx_set_row_window")

    def set_uv_model(self, model="reference_gl"):
        """Which vUv the following draws' fragments see: "ideal" = (i + 0.5) / n; "reference_gl" = the reference GL's rasteriser value, bit
        for bit (include/rfx.h rfx_set_uv_model; what the parity tests against the reference GLSL on llvmpipe are tightest under)."""
        m = {"ideal": abi.RFX_UV_IDEAL, "reference_gl": abi.RFX_UV_REFERENCE_GL}.get(model, model)
        self._chk(self.lib.rfx_set_uv_model(self._h, int(m)), "rfx_set_uv_model")

    def ssgi_march(self, p: abi.SsgiParams):
        self._chk(self.lib.rfx_ssgi_march(self._h, C.byref(p)), "rfx_ssgi_march")

    def ssgi_trace(self, p: abi.SsgiParams):
        """First half of ssgi_march (up to the end of the ray march); see rfx.h."""
        self._chk(self.lib.rfx_ssgi_trace(self._h, C.byref(p)), "rfx_ssgi_trace")

    def ssgi_shade(self, p: abi.SsgiParams):
        """Second half: shades the traced rays; the only part that reads last frame's composed GI."""
        self._chk(self.lib.rfx_ssgi_shade(self._h, C.byref(p)), "rfx_ssgi_shade")

    def temporal_reproject(self, p: abi.TemporalParams):
        self._chk(self.lib.rfx_temporal_reproject(self._h, C.byref(p)), "rfx_temporal_reproject")

    def copy_framebuffer(self, dst: int):
        self._chk(self.lib.rfx_copy_framebuffer(self._h, dst), "rfx_copy_framebuffer")

    def poisson_denoise(self, p: abi.DenoiseParams):
        self._chk(self.lib.rfx_poisson_denoise(self._h, C.byref(p)), "rfx_poisson_denoise")

    def compose(self, p: abi.ComposeParams):
        self._chk(self.lib.rfx_compose(self._h, C.byref(p)), "rfx_compose")

    def final_compose(self, p: abi.FinalParams):
        self._chk(self.lib.rfx_final_compose(self._h, C.byref(p)), "rfx_final_compose")

    def motion_blur(self, p: abi.MotionBlurParams):
        """MotionBlurEffect's mainImage (K6, include/rfx.h rfx_motion_blur) -> abi.TEX_MOTION_BLUR"""
        self._chk(self.lib.rfx_motion_blur(self._h, C.byref(p)), "rfx_motion_blur")

    def motion_blur_reach_mask(self, p: abi.MotionBlurParams) -> np.ndarray:
        """rfx_motion_blur_reach_mask: one uint32 per frame row — bit b set when motion_blur(p) loads a texel of `p.source` in column block b
        of that row (32 blocks across the frame) for this context's tile rows (row window honoured)."""
        m = np.zeros(self.H, np.uint32)
        self._chk(self.lib.rfx_motion_blur_reach_mask(self._h, C.byref(p), m.ctypes.data_as(C.POINTER(C.c_uint32)), self.H), "rfx_motion_blur_reach_mask")
        return m

    def motion_blur_stage(self, p: abi.MotionBlurParams):
        """rfx_motion_blur_stage: the tile rows of `p.source` into abi.TEX_BLUR_SOURCE; arms the row-tiled motion_blur for that source."""
        self._chk(self.lib.rfx_motion_blur_stage(self._h, C.byref(p)), "rfx_motion_blur_stage")

    def motion_blur_gather(self, p: abi.MotionBlurParams) -> int:
        """rfx_motion_blur_gather: stage + reach mask + the exchange of the named column blocks over the context's communicator (comm_wait
        before the draw).  Returns the bytes this rank receives."""
        n = C.c_size_t(0)
        self._chk(self.lib.rfx_motion_blur_gather(self._h, C.byref(p), None, C.byref(n)), "rfx_motion_blur_gather")
        return int(n.value)

    def sync(self):
        self._chk(self.lib.rfx_sync(self._h), "rfx_sync")

    # -- row-tiled runs: RCCL exchanges behind the C ABI (rfx.h "row-tiled runs")
    @staticmethod
    def split_rows(height: int, nranks: int, rank: int):
        y0, n = C.c_int(), C.c_int()
        if abi.load_library().rfx_split_rows(int(height), int(nranks), int(rank), C.byref(y0), C.byref(n)) != 0:
            raise ValueError("rfx_split_rows(%d, %d, %d)" % (height, nranks, rank))
        return y0.value, n.value

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = abi.load_library().rfx_comm_unique_id(buf)
        if rc != 0:
            raise RfxError("rfx_comm_unique_id failed (%d): RCCL not loadable on this host?" % rc)
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, nranks: int):
        assert len(unique_id) == 128
        self._chk(self.lib.rfx_comm_init(self._h, C.c_char_p(unique_id), int(rank), int(nranks)), "rfx_comm_init")
        self.comm_rank, self.comm_nranks = int(rank), int(nranks)

    def comm_destroy(self):
        self._chk(self.lib.rfx_comm_destroy(self._h), "rfx_comm_destroy")

    def halo_exchange(self, tex: int, up_rank: int, down_rank: int):
        self._chk(self.lib.rfx_halo_exchange(self._h, tex, None, int(up_rank), int(down_rank)), "rfx_halo_exchange")

    def allgather_history(self, tex: int):
        self._chk(self.lib.rfx_allgather_history(self._h, tex, None), "rfx_allgather_history")

    def ssgi_hit_rows(self):
        """rfx_ssgi_hit_rows: after ssgi_trace, the inclusive (lo, hi) range of history rows the shade will read (hi < lo: none)."""
        lo, hi = C.c_int(0), C.c_int(0)
        self._chk(self.lib.rfx_ssgi_hit_rows(self._h, C.byref(lo), C.byref(hi)), "rfx_ssgi_hit_rows")
        return int(lo.value), int(hi.value)

    def ssgi_target_rows(self, resolution_scale: float = 1.0):
        """rfx_ssgi_target_rows: (row0, rows) of the K1 target this context's TEX_SSGI holds after a draw at that resolutionScale — every row
        of the (W*s) x (H*s) target on a whole-frame context, the rows K2's staging of the tile addresses on a row tile (include/rfx.h);
        the held band at scale 1."""
        r0, n = C.c_int(0), C.c_int(0)
        self._chk(self.lib.rfx_ssgi_target_rows(self._h, float(resolution_scale), C.byref(r0), C.byref(n)), "rfx_ssgi_target_rows")
        return int(r0.value), int(n.value)

    def download_ssgi_target(self, resolution_scale: float):
        """The target rows of a draw at resolutionScale != 1 as (row0, array of (rows, W*s, 4) uint32): the first rows * W*s texels of TEX_SSGI."""
        r0, n = self.ssgi_target_rows(resolution_scale)
        ws = int(np.float32(self.W) * np.float32(resolution_scale))  # (float)W * s, as the library forms it
        return r0, np.ascontiguousarray(self.download(abi.TEX_SSGI)).reshape(-1)[:n * ws * 4].reshape(n, ws, 4).copy()

    def ssgi_hit_mask(self) -> np.ndarray:
        """rfx_ssgi_hit_mask: after ssgi_trace, one uint32 per frame row — bit b set when the shade reads a history texel of that row in column
        block b (32 blocks across the frame); 0 = the row is not read."""
        m = np.zeros(self.H, np.uint32)
        self._chk(self.lib.rfx_ssgi_hit_mask(self._h, m.ctypes.data_as(C.POINTER(C.c_uint32)), self.H), "rfx_ssgi_hit_mask")
        return m

    def gather_history_rows(self, tex: int) -> int:
        """rfx_gather_history_rows (between ssgi_trace and ssgi_shade): only the rows of last frame's composed GI that some tile's rays
        will read travel, from their owners.  Returns the bytes this rank receives."""
        n = C.c_size_t(0)
        self._chk(self.lib.rfx_gather_history_rows(self._h, tex, None, C.byref(n)), "rfx_gather_history_rows")
        return int(n.value)

    # -- the device-driven history gather (rfx_peer_*: peer loads through IPC mappings, no RCCL)
    def peer_export(self, tex: int) -> bytes:
        """rfx_peer_export: the blob (IPC handles of the plane and of this rank's flag block) every other rank needs"""
        b = C.create_string_buffer(abi.PEER_BLOB_BYTES)
        self._chk(self.lib.rfx_peer_export(self._h, tex, b), "rfx_peer_export")
        return b.raw

    def peer_open(self, tex: int, blobs, rank: int, nranks: int):
        """rfx_peer_open: `blobs` = every rank's peer_export() in rank order"""
        raw = b"".join(blobs)
        assert len(raw) == nranks * abi.PEER_BLOB_BYTES
        self._chk(self.lib.rfx_peer_open(self._h, tex, raw, rank, nranks), "rfx_peer_open")

    def peer_gather_history(self, tex: int) -> int:
        """rfx_peer_gather_history (between ssgi_trace and ssgi_shade, on every rank): this rank's kernel pulls the column blocks its rays will
        read out of their owners' planes.  Returns the bytes the PREVIOUS call's kernel moved (nothing waits on the host)."""
        n = C.c_size_t(0)
        self._chk(self.lib.rfx_peer_gather_history(self._h, tex, C.byref(n)), "rfx_peer_gather_history")
        return int(n.value)

    def peer_close(self):
        self._chk(self.lib.rfx_peer_close(self._h), "rfx_peer_close")

    def comm_wait(self):
        self._chk(self.lib.rfx_comm_wait(self._h), "rfx_comm_wait")

    def time_begin(self):
        self._chk(self.lib.rfx_time_begin(self._h), "rfx_time_begin")

    def time_end(self) -> float:
        ms = C.c_float()
        self._chk(self.lib.rfx_time_end(self._h, C.byref(ms)), "rfx_time_end")
        return ms.value


    def profile(self, enable=True):
        """Per-draw device timing inside a frame loop (include/rfx.h rfx_profile): True resets the sums and starts, False stops."""
        self._chk(self.lib.rfx_profile(self._h, 1 if enable else 0), "rfx_profile")

    def profile_read(self):
        """-> {kind: (summed ms, launches)} since the last profile(True), for the kinds that launched (abi.PROF_KINDS_ALL)"""
        n = len(abi.PROF_KINDS_ALL)
        ms, cnt = (C.c_float * n)(), (C.c_int * n)()
        self._chk(self.lib.rfx_profile_read_n(self._h, ms, cnt, n), "rfx_profile_read_n")
        return {abi.PROF_KINDS_ALL[k]: (float(ms[k]), int(cnt[k])) for k in range(n) if cnt[k]}

    def halo_violations(self) -> int:
        return int(self.lib.rfx_halo_violations(self._h))
