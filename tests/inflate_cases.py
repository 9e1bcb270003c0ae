"""The deflate corpus of the K9 tests (csrc/k9_inflate.h): how zlib is asked to code a run of bytes, the classes of input that reach every
part of a decoder, and hand-made invalid streams.  tests/test_inflate_core_cpu.py feeds all of it to the decoder core on the CPU;
tests/test_gpu_exr_import.py re-packs the chunks of an EXR file with the same forms."""
import struct
import zlib

import numpy as np

# name -> (level, strategy)
FORMS = {
    "level0": (0, zlib.Z_DEFAULT_STRATEGY), "level1": (1, zlib.Z_DEFAULT_STRATEGY), "level6": (6, zlib.Z_DEFAULT_STRATEGY),
    "level9": (9, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED), "huffman_only": (6, zlib.Z_HUFFMAN_ONLY), "rle": (6, zlib.Z_RLE),
    "filtered": (6, zlib.Z_FILTERED),
}


def deflate(data: bytes, form: str, flush_every: int = 0) -> bytes:
    """one zlib stream of `data` in the given form; flush_every > 0 cuts it into blocks with Z_FULL_FLUSH (empty stored blocks in between)"""
    level, strategy = FORMS[form]
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for i in range(0, len(data), flush_every):
        out += c.compress(data[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def predicted_scanline(width: int = 257, seed: int = 5) -> bytes:
    """the predicted bytes (OpenEXR's ZIP pre-transform) of one scanline of a four-channel half AOV: smooth ramps with a little noise"""
    from rfx_amd import imageio
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 1.0, width, dtype=np.float32)
    rows = [(0.2 + 0.7 * x * (k + 1) / 4 + 0.01 * rng.random(width, dtype=np.float32)).astype("<f2").tobytes() for k in range(4)]
    return imageio._exr_predict(b"".join(rows))


def input_classes() -> dict:
    rng = np.random.default_rng(11)
    period = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    return {
        "empty": b"",
        "one_byte": b"\x5a",
        "all_equal": b"\x07" * 5000,                                   # distance 1, length 258
        "two_stored_blocks": rng.integers(0, 4, 70000, dtype=np.uint8).tobytes(),  # 70 000 bytes: level 0 needs two stored blocks
        "period_32768": (period * 3)[:70001],                           # the maximum distance
        "random": rng.integers(0, 256, 3001, dtype=np.uint8).tobytes(),
        "aov_scanline": predicted_scanline(),
    }


class Bits:
    """deflate's bit order: fields least significant bit first, Huffman codes most significant bit first"""
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, bits):
        for k in range(bits - 1, -1, -1):
            self.put((value >> k) & 1, 1)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")


def _zlib_wrap(body: bytes, raw: bytes) -> bytes:
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(raw))


def _dynamic_header(b: Bits, nlit: int):
    """a final dynamic block whose code-length code is {0: '0', 1: '1'}: every later length costs one bit"""
    b.put(1, 1); b.put(2, 2)
    b.put(nlit - 257, 5); b.put(0, 5); b.put(18 - 4, 4)
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1):
        b.put(1 if sym in (0, 1) else 0, 3)


def handmade_invalid() -> dict:
    """name -> (stream, raw size the caller would expect): each must be refused by zlib and by K9"""
    out = {}
    b = Bits()  # fixed block: literal 'a', then length 3 at distance 2 with one byte produced
    b.put(1, 1); b.put(1, 2)
    b.code(0x30 + 0x61, 8); b.code(1, 7); b.code(1, 5); b.code(0, 7)
    out["distance_too_far"] = (_zlib_wrap(b.bytes(), b"aaaa"), 4)
    b = Bits()  # 19 code-length codes of one bit each
    b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(15, 4)
    for _ in range(19):
        b.put(1, 3)
    out["oversubscribed_code_length_code"] = (_zlib_wrap(b.bytes() + b"\0" * 8, b""), 0)
    b = Bits()  # 257 literal codes of one bit each
    _dynamic_header(b, 257)
    for _ in range(258):
        b.put(1, 1)
    out["oversubscribed_literal_set"] = (_zlib_wrap(b.bytes() + b"\0" * 8, b""), 0)
    b = Bits()  # a complete literal set {0, 1} that has no end-of-block code
    _dynamic_header(b, 257)
    b.put(1, 1); b.put(1, 1)
    for _ in range(256):
        b.put(0, 1)
    out["no_end_of_block_code"] = (_zlib_wrap(b.bytes() + b"\0" * 8, b""), 0)
    good = zlib.compress(b"the trailer of this stream is changed", 6)
    out["wrong_adler32"] = (good[:-1] + bytes([good[-1] ^ 1]), 37)
    body = zlib.compress(b"header", 6)[2:]
    out["header_fcheck"] = (b"\x78\x02" + body, 6)
    out["header_method_7"] = (bytes([0x77, 31 - (0x7700 % 31)]) + body, 6)
    out["header_window_64k"] = (bytes([0x88, 31 - (0x8800 % 31)]) + body, 6)
    flg = 0x20
    flg += 31 - ((0x7800 + flg) % 31)
    out["header_preset_dictionary"] = (bytes([0x78, flg]) + body, 6)
    return out
