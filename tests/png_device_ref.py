"""NumPy restatement of the device PNG coder (include/rfx.h "PNG fragments", K8 in csrc/k8_png.h): the filter choice, the code-length rule,
the block header, the two payload forms, the chunk, the fragment and its result buffer, line by line as the header states them.  Shared by
tests/test_png_device_cpu.py and tests/test_gpu_png.py; the device's fragment must equal fragment() byte for byte."""
import struct
import zlib

import numpy as np

ADLER_MOD = 65521
MAXBITS, CL_MAXBITS = 15, 7
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FILTER_TYPES = (0, 1, 2, 4)  # rfx_stage_png's filter 1..4 -> PNG filter type None, Sub, Up, Paeth
HEADER_BYTES = 32
STORED_MAX = 65535


# ---------------------------------------------------------------- filters
def residuals(cur, up, bpp, ftype):
    """cur, up: uint8 with the row's bytes along the last axis (up None = the tile's first scanline); -> the residual bytes of PNG filter
    type `ftype`"""
    x = cur.astype(np.int32)
    a = np.zeros_like(x)
    a[..., bpp:] = x[..., :-bpp]
    b = np.zeros_like(x) if up is None else up.astype(np.int32)
    c = np.zeros_like(x)
    c[..., bpp:] = b[..., :-bpp]
    if ftype == 0:
        p = 0
    elif ftype == 1:
        p = a
    elif ftype == 2:
        p = b
    elif ftype == 4:
        pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
        p = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    else:
        raise ValueError(ftype)
    return ((x - p) & 255).astype(np.uint8)


def cost(res):
    """the sum of |residual as int8| along the last axis: an int for one row, an array for a stack of rows"""
    r = res.astype(np.int64)
    k = np.minimum(r, 256 - r).sum(-1)
    return int(k) if k.ndim == 0 else k


def choose_filter(cur, up, bpp, filt):
    """filt 0: the smallest sum of |residual as int8| (ties: lowest type number), None / Sub only on the first scanline; 1..4 forced, Up and
    Paeth falling back to Sub on the first scanline"""
    first = up is None
    if filt:
        t = FILTER_TYPES[filt - 1]
        return 1 if (first and t in (2, 4)) else t
    best, best_cost = None, None
    for t in ((0, 1) if first else FILTER_TYPES):
        k = cost(residuals(cur, up, bpp, t))
        if best is None or k < best_cost:
            best, best_cost = t, k
    return best


def filtered_rows(tile, filt):
    """tile: (rows, W, channels) uint8, row 0 = bottom -> the filtered scanlines, top first: a list of 1-D uint8 (type byte + residuals).
    choose_filter's rule for every scanline, evaluated for all of them at once (a tile of 32768 rows would otherwise take its time)"""
    rows, W, ch = tile.shape
    cur = np.ascontiguousarray(tile).reshape(rows, W * ch)[::-1]  # top first
    up = np.concatenate([np.zeros_like(cur[:1]), cur[:-1]])  # (zeros above the first scanline: what residuals() takes for up = None)
    if filt:
        t = FILTER_TYPES[filt - 1]
        types = np.full(rows, t)
        types[0] = 1 if t in (2, 4) else t
        wanted = sorted(set(types.tolist()))
    else:
        wanted = list(FILTER_TYPES)
    res = {t: residuals(cur, up, ch, t) for t in wanted}
    if not filt:
        costs = np.stack([cost(res[t]) for t in FILTER_TYPES])
        types = np.asarray(FILTER_TYPES)[np.argmin(costs, 0)]  # (argmin: the first of equal costs, so the lowest type number)
        types[0] = FILTER_TYPES[int(np.argmin(costs[:2, 0]))]  # None / Sub only
    return [np.concatenate([np.array([t], np.uint8), res[int(t)][s]]) for s, t in enumerate(types)]


# ---------------------------------------------------------------- the code-length rule
def code_lengths(freq, maxbits):
    """The rule of rfx.h: rank the used symbols by (frequency descending, symbol ascending); Moffat-Katajainen's in-place minimum-redundancy
    lengths over the ascending frequencies (an internal node before a leaf of equal weight); lengths above `maxbits` counted at `maxbits`;
    while the Kraft sum is too large, drop one code from `maxbits` and split the deepest shorter code into two; hand the lengths out again by
    rank, shortest first."""
    n = len(freq)
    order = sorted((s for s in range(n) if freq[s] > 0), key=lambda s: (-int(freq[s]), s))
    m = len(order)
    lens = [0] * n
    if m == 0:
        return lens
    if m == 1:
        lens[order[0]] = 1
        return lens
    A = [int(freq[s]) for s in reversed(order)]
    A[0] += A[1]
    root, leaf = 0, 2
    for nxt in range(1, m - 1):
        if leaf >= m or A[root] <= A[leaf]:
            A[nxt] = A[root]
            A[root] = nxt
            root += 1
        else:
            A[nxt] = A[leaf]
            leaf += 1
        if leaf >= m or (root < nxt and A[root] <= A[leaf]):
            A[nxt] += A[root]
            A[root] = nxt
            root += 1
        else:
            A[nxt] += A[leaf]
            leaf += 1
    A[m - 2] = 0
    for nxt in range(m - 3, -1, -1):
        A[nxt] = A[A[nxt]] + 1
    avbl, used, dpth, root, nxt = 1, 0, 0, m - 2, m - 1
    while avbl > 0:
        while root >= 0 and A[root] == dpth:
            used += 1
            root -= 1
        while avbl > used:
            A[nxt] = dpth
            nxt -= 1
            avbl -= 1
        avbl, dpth, used = 2 * used, dpth + 1, 0
    count = [0] * (maxbits + 1)
    for d in A:
        count[min(d, maxbits)] += 1
    total = sum(count[i] << (maxbits - i) for i in range(1, maxbits + 1))
    while total > (1 << maxbits):
        count[maxbits] -= 1
        for i in range(maxbits - 1, 0, -1):
            if count[i]:
                count[i] -= 1
                count[i + 1] += 2
                break
        total -= 1
    k = 0
    for i in range(1, maxbits + 1):
        for _ in range(count[i]):
            lens[order[k]] = i
            k += 1
    return lens


def canonical_codes(lens, maxbits):
    """deflate's canonical codes, bit-reversed (the stream is packed from the least significant bit)"""
    count = [0] * (maxbits + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (maxbits + 2), 0
    for b in range(1, maxbits + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            c, nxt[l] = nxt[l], nxt[l] + 1
            out[s] = int(format(c, "0%db" % l)[::-1], 2)
    return out


def length_tokens(seq):
    """the code-length sequence -> (symbol, extra bits, extra value): zero runs as 18 (11..138) while 11 or more remain, then 17 (3..10), then
    single zeros; a non-zero run as the length once, then 16 (3..6) while 3 or more remain, then single lengths"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        r = j - i
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, 7, k - 11))
                r -= k
            if r >= 3:
                out.append((17, 3, r - 3))
                r = 0
            out += [(0, 0, 0)] * r
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, 2, k - 3))
                r -= k
            out += [(v, 0, 0)] * r
        i = j
    return out


def pack_bits(values, nbits):
    """LSB-first packing of values[i] in nbits[i] bits -> (bytes padded with zero bits, bit count)"""
    values, nbits = np.asarray(values, np.int64), np.asarray(nbits, np.int64)
    start = np.concatenate([[0], np.cumsum(nbits)])
    total = int(start[-1])
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    for k in range(int(nbits.max()) if nbits.size else 0):
        m = nbits > k
        bits[start[:-1][m] + k] = (values[m] >> k) & 1
    return np.packbits(bits, bitorder="little").tobytes(), total


def compressed_payload(line):
    """form (a): one non-final dynamic block of literals + end of block, then the empty non-final stored block after padding to a byte"""
    freq = np.bincount(line, minlength=257).astype(np.int64)
    freq[256] = 1
    lens = code_lengths(freq, MAXBITS)
    codes = canonical_codes(lens, MAXBITS)
    tokens = length_tokens(lens + [0])  # 257 literal/length codes, one (unused) distance code
    clfreq = [0] * 19
    for t in tokens:
        clfreq[t[0]] += 1
    cllens = code_lengths(clfreq, CL_MAXBITS)
    clcodes = canonical_codes(cllens, CL_MAXBITS)
    hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cllens[s]))
    v, n = [4, 0, 0, hclen - 4], [3, 5, 5, 4]  # BFINAL 0 + BTYPE 2; HLIT = 257 - 257; HDIST = 1 - 1
    for s in CL_ORDER[:hclen]:
        v.append(cllens[s])
        n.append(3)
    for sym, eb, ev in tokens:
        v.append(clcodes[sym])
        n.append(cllens[sym])
        if eb:
            v.append(ev)
            n.append(eb)
    la, ca = np.asarray(lens, np.int64), np.asarray(codes, np.int64)
    v = np.concatenate([np.asarray(v, np.int64), ca[line], [codes[256], 0]])
    n = np.concatenate([np.asarray(n, np.int64), la[line], [lens[256], 3]])
    body, _ = pack_bits(v, n)
    return body + b"\x00\x00\xff\xff"


def stored_payload(line):
    raw, out = line.tobytes(), b""
    for o in range(0, len(raw), STORED_MAX):
        part = raw[o:o + STORED_MAX]
        out += b"\x00" + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part
    return out


def min_compressed_bytes(n):
    """A lower bound on form (a) for a line of n bytes, so that payload() need not build it for a line too short to gain (n <= 5).  17 bits
    stand in front of the code-length code's lengths, and at least four of those follow (12).  The 258 code lengths hold at most n + 1 used
    symbols, so at least 257 - n zeros; a token spells at most 138 of them and costs at least one bit.  The used symbols (two or more: a
    byte and the end of block) take at least two tokens more.  Every literal and the end of block cost a bit or more (n + 1); then the
    stored block's 3 bits, the padding, and its 4 bytes."""
    zero_tokens = max(0, -(-(257 - n) // 138))
    return (17 + 12 + zero_tokens + 2 + (n + 1) + 3 + 7) // 8 + 4


def payload(line):
    """the smaller of the two forms; a tie goes to the compressed one"""
    b = stored_payload(line)
    if len(b) < min_compressed_bytes(len(line)):
        return b
    a = compressed_payload(line)
    return a if len(a) <= len(b) else b


def chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


# ---------------------------------------------------------------- fragment, result buffer, file
def bound(W, rows, channels):
    n = 1 + W * channels
    return HEADER_BYTES + rows * (12 + 5 * ((n + STORED_MAX - 1) // STORED_MAX) + n)


def fragment(tile, filt=0):
    """tile: (rows, W, channels) uint8, row 0 = bottom -> (fragment bytes, adler_a, adler_b, raw_bytes, payloads)"""
    lines = filtered_rows(np.asarray(tile, np.uint8), filt)
    payloads = [payload(l) for l in lines]
    raw = b"".join(l.tobytes() for l in lines)
    ad = zlib.adler32(raw) & 0xFFFFFFFF
    return b"".join(chunk(b"IDAT", p) for p in payloads), ad & 0xFFFF, ad >> 16, len(raw), payloads


def result_prefix(tile, filt=0):
    """the result buffer up to the fragment's end: the 32-byte header and the fragment"""
    frag, a, b, raw, _ = fragment(tile, filt)
    return struct.pack("<QIIQQ", len(frag), a, b, raw, 0) + frag


def adler_combine(parts):
    """parts: (adler_a, adler_b, raw_bytes) per tile, top first -> the Adler-32 of the concatenation"""
    A, B = 1, 0
    for a2, b2, n2 in parts:
        B = (B + b2 + n2 % ADLER_MOD * (A - 1 + ADLER_MOD)) % ADLER_MOD
        A = (A + a2 - 1 + ADLER_MOD) % ADLER_MOD
    return (B << 16) | A


def png_file(W, H, channels, results):
    """results: the tiles' result buffers (or prefixes), top tile first -> the PNG file's bytes"""
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if channels == 3 else 6, 0, 0, 0)) + chunk(b"IDAT", b"\x78\x01")
    parts = []
    for r in results:
        r = bytes(r)
        n, a, b, raw, _ = struct.unpack("<QIIQQ", r[:HEADER_BYTES])
        out += r[HEADER_BYTES:HEADER_BYTES + n]
        parts.append((a, b, raw))
    return out + chunk(b"IDAT", b"\x03\x00" + struct.pack(">I", adler_combine(parts))) + chunk(b"IEND", b"")


def noisy_frame(W, H, channels=3, seed=1):
    """the issue's synthetic frame: smooth shading plus sigma = 2 code values of noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(x / W * 3.0 + k) * np.cos(y / H * 2.0 - k) for k in range(channels)], -1)
    return np.clip(np.rint(base + rng.normal(0.0, 2.0, base.shape)), 0, 255).astype(np.uint8)
