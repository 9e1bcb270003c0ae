"""Shared by the tests of the streamed EXR frames (rfx.h rfx_stage_exr_aov): seeded AOV channels, and `repack`, which rewrites the chunks of a
compression="none" file in a chosen compression with a chosen deflate call — the deflate form inside the file is under the test's control, and
the pixels stay those of the file it started from."""
import struct
import zlib

import numpy as np

from rfx_amd import imageio

NONE, ZIPS, ZIP = 0, 2, 3
PER_CHUNK = {NONE: 1, ZIPS: 1, ZIP: 16}


def channels(W, H, seed=3, planes=None, steps=64, noise=False):
    """{layer.channel: (H, W) float32}: every value a multiple of 1 / steps (so a half holds it and deflate finds matches), a unit-length-ish
    normal, depth 1 on a seeded tenth of the texels; noise=True: seeded finite halves with every bit random (deflate cannot shrink them)"""
    rng = np.random.default_rng(seed)
    out = {}
    for key, names in imageio.AOV_LAYOUT.items():
        if planes is not None and key not in planes:
            continue
        for n in names:
            if noise:
                bits = rng.integers(0, 1 << 16, (H, W)).astype(np.uint16)
                bits[(bits & 0x7c00) == 0x7c00] ^= 0x0400  # (no infinity, no NaN)
                v = bits.view(np.float16).astype(np.float32)
            else:
                v = np.round(rng.random((H, W)) * steps) / steps
                if key == "normal":
                    v = v * 2 - 1 + 1 / (2 * steps)
                if key == "velocity":
                    v = (v - 0.5) / 8
                if key == "emissive":
                    v = v * (rng.random((H, W)) < 0.25) * 4
            out[n] = v.astype(np.float32)
    if "depth.Z" in out and not noise:
        d = out["depth.Z"] * 0.9
        d[rng.random((H, W)) < 0.1] = 1.0
        d.flat[0] = 1.0
        out["depth.Z"] = d.astype(np.float32)
    return out


def as_parts(ch):
    """one part per layer: {layer: {channel: plane}} for imageio.write_exr_multipart"""
    parts = {}
    for name, v in ch.items():
        layer, c = name.split(".")
        parts.setdefault(layer, {})[c] = v
    return parts


def repack(src, dst, compression, deflate=None, line_order=0, writer_rule=False):
    """The compression="none" scanline file `src` -> `dst` with the same headers and pixels, its scanlines regrouped into chunks of `compression`
    (NONE / ZIPS / ZIP) and each chunk's predicted bytes coded by deflate(bytes) -> a zlib stream.  A chunk whose stream has exactly the raw size
    cannot be told from the raw block and is refused here; otherwise the stream is stored whatever its size (a stream longer than the raw block
    is something only this helper writes: OpenEXR's writers store the raw block instead — writer_rule=True does that, deflate=None does it for
    every chunk).  line_order=1:
    the chunks lie in the file bottom scanline first, as a decreasing-Y file's do.  -> the records of the chunks, in offset-table order."""
    d = open(src, "rb").read()
    lay = imageio.exr_aov_layout(d)
    version = struct.unpack("<i", d[4:8])[0]
    multipart = bool(version & 0x1000)
    headers, pos = [], 8
    while True:
        attrs, pos = imageio._exr_parse_header(d, pos)
        headers.append(attrs)
        if not multipart or d[pos] == 0:
            break
    H, per = lay.height, PER_CHUNK[compression]
    head, bodies = d[:8], []
    for k, attrs in enumerate(headers):
        assert attrs[b"compression"][1] == b"\0", "repack starts from an uncompressed file"
        rows = {int(c["y"]): d[int(c["offset"]):int(c["offset"] + c["packed_bytes"])] for c in lay.chunks[lay.chunks["part"] == k]}
        chunks = []
        for y0 in range(0, H, per):
            raw = b"".join(rows[y] for y in range(y0, min(H, y0 + per)))
            data = raw
            if compression != NONE and deflate is not None:
                data = deflate(imageio._exr_predict(raw))
                if writer_rule and len(data) >= len(raw):
                    data = raw
                assert data is raw or len(data) != len(raw), "a stream of exactly the raw size reads as the raw block"
            chunks.append((y0, data))
        bodies.append(chunks)
        for name, (typ, payload) in attrs.items():
            if name == b"compression":
                payload = bytes([compression])
            elif name == b"chunkCount":
                payload = struct.pack("<i", len(chunks))
            elif name == b"lineOrder":
                payload = bytes([line_order])
            head += imageio._exr_attr(name, typ, payload)
        head += b"\0"
    if multipart:
        head += b"\0"
    pos = len(head) + 8 * sum(len(c) for c in bodies)
    table, blob, records = b"", b"", []
    for k, chunks in enumerate(bodies):
        offs = {}
        for y0, data in (chunks[::-1] if line_order else chunks):
            offs[y0] = pos
            rec = (struct.pack("<i", k) if multipart else b"") + struct.pack("<ii", y0, len(data)) + data
            blob += rec
            pos += len(rec)
        for y0, data in chunks:
            table += struct.pack("<Q", offs[y0])
            records.append((k, y0, min(per, H - y0), offs[y0] + (12 if multipart else 8), len(data)))
    with open(dst, "wb") as f:
        f.write(head + table + blob)
    return records


def flip_adler_byte(path, record):
    """flip one bit of the last byte (the Adler-32 trailer) of the chunk `record` (one of repack's) in place"""
    d = bytearray(open(path, "rb").read())
    d[record[3] + record[4] - 1] ^= 0x10
    open(path, "wb").write(bytes(d))


def zlib_form(level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    def deflate(data):
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        if not flush_every:
            return c.compress(data) + c.flush()
        out = b""
        for i in range(0, len(data), flush_every):
            out += c.compress(data[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
        return out + c.flush()
    return deflate
