"""NumPy restatement of the device EXR coder (include/rfx.h "EXR fragments", K8's second pre-transform in csrc/k8_exr.h): the raw block, the
predicted bytes, the two data forms, the chunk, the fragment and its result buffer, line by line as the header states them.  The code-length
rule, the canonical codes, the header tokens and the bit packing are png_device_ref's, by import: the header says "word for word".  Shared by
tests/test_exr_device_cpu.py, tests/test_gpu_exr_device.py and tests/test_node_exr.py; the device's result must equal result_prefix() byte for
byte.  A pure function: halfs (as uint16 bit patterns) -> bytes."""
import struct
import zlib

import numpy as np

import png_device_ref as R

HEADER_BYTES = 32


def as_bits(tile):
    """(rows, W, channels) float16 or uint16 -> the halfs' bit patterns, uint16"""
    a = np.ascontiguousarray(tile)
    return a.view(np.uint16) if a.dtype == np.float16 else a.astype(np.uint16)


def raw_blocks(tile):
    """tile: (rows, W, channels), row 0 = bottom -> the scanlines' raw blocks, top first: the channels in alphabetical order (A, B, G, R or
    B, G, R: the export's R, G, B(, A) backwards), each as W little-endian halfs"""
    bits = as_bits(tile)[::-1]  # top first
    return [np.ascontiguousarray(row.T[::-1]).astype("<u2").tobytes() for row in bits]


def predict(raw):
    """even-indexed bytes then odd-indexed ones; each byte but the first replaced by its difference to its predecessor + 128"""
    a = np.frombuffer(raw, np.uint8)
    t = np.concatenate([a[0::2], a[1::2]]).astype(np.int32)
    d = t.copy()
    d[1:] = t[1:] - t[:-1] + 128
    return (d & 255).astype(np.uint8)


def zlib_stream(d):
    """form (a): 78 01, one FINAL dynamic block of the literals d + end of block padded to a byte, the Adler-32 of d big-endian"""
    freq = np.bincount(d, minlength=257).astype(np.int64)
    freq[256] = 1
    lens = R.code_lengths(freq, R.MAXBITS)
    codes = R.canonical_codes(lens, R.MAXBITS)
    tokens = R.length_tokens(lens + [0])  # 257 literal/length codes, one (unused) distance code
    clfreq = [0] * 19
    for t in tokens:
        clfreq[t[0]] += 1
    cllens = R.code_lengths(clfreq, R.CL_MAXBITS)
    clcodes = R.canonical_codes(cllens, R.CL_MAXBITS)
    hclen = max(4, max(i + 1 for i, s in enumerate(R.CL_ORDER) if cllens[s]))
    v, n = [5, 0, 0, hclen - 4], [3, 5, 5, 4]  # BFINAL 1 + BTYPE 2 (bits 1 0 1); HLIT = 257 - 257; HDIST = 1 - 1
    for s in R.CL_ORDER[:hclen]:
        v.append(cllens[s])
        n.append(3)
    for sym, eb, ev in tokens:
        v.append(clcodes[sym])
        n.append(cllens[sym])
        if eb:
            v.append(ev)
            n.append(eb)
    la, ca = np.asarray(lens, np.int64), np.asarray(codes, np.int64)
    v = np.concatenate([np.asarray(v, np.int64), ca[d], [codes[256]]])
    n = np.concatenate([np.asarray(n, np.int64), la[d], [lens[256]]])
    body, bits = R.pack_bits(v, n)
    assert len(body) == (bits + 7) // 8
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(d.tobytes()) & 0xFFFFFFFF)


def min_stream_bytes(n):
    """a lower bound on form (a) for n literals, so that data() need not build it for a block too short to gain: png_device_ref's bound
    without the stored block's 3 bits and 4 bytes, plus the two header bytes and the Adler-32"""
    zero_tokens = max(0, -(-(257 - n) // 138))
    return 2 + (17 + 12 + zero_tokens + 2 + (n + 1) + 7) // 8 + 4


def data(raw):
    """form (a) only when strictly smaller than the raw block, else the raw block (b)"""
    if min_stream_bytes(len(raw)) >= len(raw):
        return raw
    a = zlib_stream(predict(raw))
    return a if len(a) < len(raw) else raw


def bound(W, rows, channels):
    return HEADER_BYTES + rows * (8 + 2 * W * channels)


def fragment(tile, first_y):
    """tile: (rows, W, channels) halfs, row 0 = bottom; first_y: the EXR y of its top scanline -> (fragment bytes, the chunks' data)"""
    datas = [data(raw) for raw in raw_blocks(tile)]
    return b"".join(struct.pack("<ii", first_y + s, len(d)) + d for s, d in enumerate(datas)), datas


def result_prefix(tile, first_y=0):
    """the result buffer up to the fragment's end: the 32-byte header and the fragment"""
    rows, W, ch = np.asarray(tile).shape
    frag, datas = fragment(tile, first_y)
    n = 2 * W * ch
    return struct.pack("<QIIQII", len(frag), rows, first_y, rows * n, sum(1 for d in datas if len(d) == n), 0) + frag


def header_of(result):
    """(fragment_bytes, chunks, first_y, raw_bytes, raw_form_chunks, zero)"""
    return struct.unpack("<QIIQII", bytes(result[:HEADER_BYTES]))


def chunks_of(result):
    """the chunks of a result buffer -> [(y, data)]"""
    nbytes, chunks = header_of(result)[:2]
    body, out, at = bytes(result[HEADER_BYTES:HEADER_BYTES + nbytes]), [], 0
    for _ in range(chunks):
        y, size = struct.unpack("<ii", body[at:at + 8])
        out.append((y, body[at + 8:at + 8 + size]))
        at += 8 + size
    assert at == nbytes
    return out


def tiles_top_first(img, n):
    """`img` (row 0 = bottom) cut into n row tiles -> [(tile, first_y)], top tile first"""
    H = img.shape[0]
    edges = [H * k // n for k in range(n + 1)]
    return [(img[edges[k]:edges[k + 1]], H - edges[k + 1]) for k in reversed(range(n))]


def smooth_noisy_halfs(W, H, channels=4, seed=1):
    """the issue's synthetic frame: smooth shading plus 1 % multiplicative noise, as halfs (float16)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.6 + 0.5 * np.sin(x / W * 3.0 + k) * np.cos(y / H * 2.0 - k) for k in range(channels)], -1)
    return (base * (1.0 + 0.01 * rng.standard_normal(base.shape))).astype(np.float16)


def random_halfs(W, H, channels, seed):
    """uniformly random non-NaN half bit patterns (float16): no scanline shrinks"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 65536, (H, W, channels)).astype(np.uint16)
    nan = ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)
    bits[nan] &= 0xFC00  # a NaN becomes the infinity of its sign
    return bits.view(np.float16)
