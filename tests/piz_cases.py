"""A PIZ block writer for the tests, independent of every decoder: known channel planes -> the bytes of one OpenEXR PIZ block, by forward
operations alone (the channel-planar word order, the bitmap and the forward lookup, the forward wavelet, the code lengths, the canonical codes,
the bits), with switches for the forms a block may legally take that the library's own writer never emits.  The planes a block was made from
are the expected result of decoding it: nothing here reads a block back.  imageio._wav2 (forward) and imageio._huf_canonical are called;
neither is code under test.

Which rule of OpenEXR's reader (ImfPizCompressor / ImfHuf, and the same steps in OpenEXRCore) makes each form legal:
  bitmap     the reader builds its reverse table from EVERY set bit of the bytes minNonZero .. maxNonZero (zero elsewhere), and puts value 0 in
             it whether bit 0 is set or not.  It never compares the bitmap with the data, so a SUPERSET (bits of values that do not occur), the FULL
             bitmap (8192 bytes of 0xff: the table is the identity, maxValue = 65535 and the wavelet runs modulo 2^16 however small the data),
             bit 0 SET or CLEAR, and a range PADDED with zero bytes on both sides all decode.  With minNonZero > maxNonZero no byte is read at
             all: the writer spells the empty bitmap (8191, 0), and (1, 0) is the same to the reader.
  lengths    the decoding tables are built from the code lengths of the packed table, 0 .. 58 bits, whatever tree they came from: the canonical
             codes need the lengths alone.  `chain` and `flat` are Kraft-complete sets like the writer's; in `flat` symbols that never occur carry
             codes as well, and iM — which the reader takes from the header as the run escape — is larger than the largest word.  `single` is
             one symbol of length 1 and an escape without a code.
  runs       the escape (the code of symbol iM, then an 8-bit count) repeats the previous word count times, 0 .. 255; the reader asks that a
             word precedes it and that the run stays inside the block, not that the writer's cost rule chose it.
  framing    the code bits are nBits bits, any number, the last byte filled up; the block holds them if nBits <= 8 x the bytes left, so bytes
             behind them, counted by hlen, are not looked at.
  tableLength padded with zero bytes is NOT known to be a form OpenEXR's reader accepts: as far as its source is recalled (it is not at hand to
             check), hufUncompress ignores the field and reads the code bits from where the unpacking of the length table stopped, so it would
             read the padding as codes.  This project's readers, host and device, find the code bits by the field.  The case pins that place
             where they differ from OpenEXR — no writer pads, so no file shows it — and not a legal form.

Also here: the bit writer and the hand-made Huffman blocks of tests/test_piz_core_cpu.py, and the frames — parts, block rectangles, seeded
contents and options — that tests/test_piz_cases_cpu.py checks on the host and tests/test_gpu_exr_piz_edges.py sends to the device."""
import heapq
import struct

import numpy as np

from rfx_amd import imageio

HALF, FLOAT = imageio._PT_HALF, imageio._PT_FLOAT
MAX_LEN, FAST_BITS = 58, 12  # csrc/k9_piz.h K9_PIZ_MAX_LEN, K9_PIZ_FAST_BITS


# ---------------------------------------------------------------- hand-made Huffman blocks
class Bits:
    """the test's own bit writer: MSB first"""

    def __init__(self):
        self.bits = []

    def put(self, n, v):
        assert 0 <= v < (1 << n)
        self.bits += [(v >> (n - 1 - k)) & 1 for k in range(n)]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))


def canonical(lengths):
    """{symbol: length} -> {symbol: code}: ascending within a length, longer codes first"""
    count = [0] * 60
    for ln in lengths.values():
        count[ln] += 1
    start, c = [0] * 60, 0
    for ln in range(58, 0, -1):
        start[ln] = c
        c = (c + count[ln]) >> 1
    codes, nxt = {}, list(start)
    for s in sorted(lengths):
        codes[s] = nxt[lengths[s]]
        nxt[lengths[s]] += 1
    full = np.zeros(imageio._HUF_ENCSIZE, np.int64)
    for s, ln in lengths.items():
        full[s] = ln
    theirs = imageio._huf_canonical(full)
    assert all(int(theirs[s]) == codes[s] for s in lengths)
    return codes


def table_bits(lengths, im, iM):
    """the packed length table of symbols im .. iM, zero runs collapsed as the format allows"""
    t, i = Bits(), im
    while i <= iM:
        if i in lengths:
            t.put(6, lengths[i])
            i += 1
            continue
        run = 1
        while i + run <= iM and (i + run) not in lengths and run < 261:
            run += 1
        if run >= 6:
            t.put(6, 63).put(8, run - 6)
        elif run >= 2:
            t.put(6, 59 + run - 2)
        else:
            t.put(6, 0)
        i += run
    return t


def huffman_block(lengths, im, iM, stream, table=None, nbits=None, tlen=None):
    """stream: [symbol | ("run", count)] -> the Huffman block"""
    codes = canonical(lengths)
    d = Bits()
    for s in stream:
        if isinstance(s, tuple):
            d.put(lengths[iM], codes[iM]).put(8, s[1])
        else:
            d.put(lengths[s], codes[s])
    t = (table or table_bits(lengths, im, iM)).bytes()
    return struct.pack("<IIIII", im, iM, len(t) if tlen is None else tlen, len(d.bits) if nbits is None else nbits, 0) + t + d.bytes()


SKEW = {s: s + 1 for s in range(58)}  # lengths 1 .. 58, and the run escape 58 bits too: a complete set
SKEW[58] = 58
GAPS = {0: 2, 4: 2, 105: 2, 300: 2}  # 3, 100 and 194 symbols without a code between them: the short and the long zero run


# ---------------------------------------------------------------- the forward side
def pack_tokens(codes, lens):
    """(code, length) pairs, each MSB first, one behind the other -> (the bytes, the last one filled up with zeros; the number of bits)"""
    codes, lens = np.asarray(codes, np.uint64), np.asarray(lens, np.int64)
    if lens.size == 0:
        return b"", 0
    assert lens.min() >= 1 and lens.max() <= 64
    ends = np.cumsum(lens)
    starts, total = ends - lens, int(ends[-1])
    bits = np.zeros(total + (-total % 8), np.uint8)
    for k in range(int(lens.max())):
        m = lens > k
        bits[starts[m] + k] = ((codes[m] >> (lens[m] - 1 - k).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits).tobytes(), total


def block_words(planes, chans):
    """{name: (rows, cols) float array} -> the block's 16-bit words, channel-planar: per channel its rows, a FLOAT sample as two words, the low
    one first"""
    return np.concatenate([np.ascontiguousarray(planes[name].astype("<f2" if pt == HALF else "<f4")).view("<u2").reshape(-1) for name, pt in chans])


def word_planes(words, chans, cols, rows):
    """the (rows, cols) word planes inside a channel-planar buffer, as views: one per HALF channel, two interleaved in x per FLOAT channel"""
    out, p = [], 0
    for _, pt in chans:
        size = 1 if pt == HALF else 2
        rect = words[p:p + rows * cols * size].reshape(rows, cols * size)
        out += [rect[:, j::size] for j in range(size)]
        p += rows * cols * size
    return out


def bitmap_and_lut(words, form="exact", bit0=False, pad=0, empty=(8191, 0), extra=256, seed=1):
    """-> (the block's first bytes: u16 min, max and the bitmap bytes between them; the forward lookup table; mx).  form: "exact" | "superset"
    (`extra` seeded values that do not occur) | "full"; bit0: bit 0 of byte 0 as stored (value 0 is in the table either way); pad: zero bytes
    on either side of the range; empty: (min, max) when no byte is nonzero"""
    stored = np.zeros(65536, bool)
    stored[words] = True
    if form == "superset":
        absent = np.flatnonzero(~stored)[1:] if not stored[0] else np.flatnonzero(~stored)  # (value 0 is in the table anyway)
        stored[np.random.default_rng(seed).choice(absent, min(extra, absent.size), replace=False)] = True
    elif form == "full":
        stored[:] = True
    else:
        assert form == "exact"
    table = stored.copy()
    table[0] = True
    lut = (np.cumsum(table) - 1).astype(np.uint16)
    lut[~table] = 0
    stored[0] = bit0 or form == "full"
    packed = np.packbits(stored.reshape(8192, 8)[:, ::-1], axis=1).reshape(-1)  # bit v & 7 of byte v >> 3
    nz = np.flatnonzero(packed)
    if nz.size == 0:
        assert empty[0] > empty[1]
        return struct.pack("<HH", *empty), lut, 0
    mn, mxb = max(int(nz[0]) - pad, 0), min(int(nz[-1]) + pad, 8191)
    return struct.pack("<HH", mn, mxb) + packed[mn:mxb + 1].tobytes(), lut, int(table.sum()) - 1


def huffman_lengths(freq):
    """{symbol: count} -> {symbol: length}: the writer's — join the two rarest subtrees until one is left"""
    if len(freq) == 1:
        return {s: 1 for s in freq}
    lengths = dict.fromkeys(freq, 0)
    heap = [(n, s, [s]) for s, n in freq.items()]
    heapq.heapify(heap)
    while len(heap) > 1:
        fa, ka, la = heapq.heappop(heap)
        fb, kb, lb = heapq.heappop(heap)
        for s in la + lb:
            lengths[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), la + lb))
    assert max(lengths.values()) <= MAX_LEN
    return lengths


def chain_lengths(freq, escape):
    """lengths 1, 2, 3, .. k down a chain for the k most frequent symbols; the R symbols left and the escape are a complete subtree of depth j
    under the chain's last node, k + j = 58: 2^j - R of them one level higher, the escape among the deepest"""
    order = sorted((s for s in freq if s != escape), key=lambda s: (-freq[s], s)) + [escape]
    n = len(order)
    for j in range(1, 17):
        k, r = MAX_LEN - j, n - (MAX_LEN - j)
        if (1 << j) // 2 < r <= (1 << j):
            break
    else:
        raise AssertionError("a chain to 58 bits needs 59 symbols or more, not %d" % n)
    short = (1 << j) - r
    lengths = {s: i + 1 for i, s in enumerate(order[:k])}
    lengths.update({s: k + j - 1 for s in order[k:k + short]})
    lengths.update({s: k + j for s in order[k + short:]})
    return lengths


def flat_lengths(freq, escape):
    """-> (lengths, iM): 2^L codes of L >= 13 bits each: the symbols that occur, the escape, and the lowest symbols that do not occur; the escape
    moves up to 2^L - 1 where the words leave it lower"""
    L = max(FAST_BITS + 1, int(np.ceil(np.log2(len(freq)))))
    iM = max(escape, (1 << L) - 1)
    assert iM < imageio._HUF_ENCSIZE
    lengths = {s: L for s in freq if s != escape}
    lengths[iM] = L
    s = 0
    while len(lengths) < (1 << L):
        if s not in lengths:
            lengths[s] = L
        s += 1
    assert max(lengths) == iM
    return lengths, iM


def length_table(lengths, im, iM):
    """table_bits(lengths, im, iM) as (bytes, bits), without a Python step per symbol"""
    vals, nb, at = [], [], im
    for s in sorted(lengths) + [iM + 1]:
        gap = s - at
        while gap > 0:
            run = min(gap, 261)
            if run >= 6:
                vals += [63, run - 6]
                nb += [6, 8]
            else:
                vals.append(59 + run - 2 if run >= 2 else 0)
                nb.append(6)
            gap -= run
        if s <= iM:
            vals.append(lengths[s])
            nb.append(6)
        at = s + 1
    return pack_tokens(vals, nb)


def huffman_stream(words, lengths="huffman", runs="greedy", planted=(), table_pad=0, odd_nbits=False):
    """the words of a block (after lookup and wavelet) -> the Huffman block.  lengths: "huffman" | "chain" | "single" | "flat"; runs: "none" |
    "greedy" | "planted" with planted = [(position, count)]: the escape at that word position stands for words[position : position + count],
    which must repeat words[position - 1]; every other word is coded on its own"""
    words = np.asarray(words, np.int64)
    vals, counts = np.unique(words, return_counts=True)
    im, iM = int(vals[0]), int(vals[-1]) + 1
    freq = dict(zip(vals.tolist(), counts.tolist()))
    freq[iM] = 1  # the run escape
    if lengths == "huffman":
        lens = huffman_lengths(freq)
    elif lengths == "chain":
        lens = chain_lengths(freq, iM)
        assert max(lens.values()) == MAX_LEN == lens[iM]
    elif lengths == "flat":
        lens, iM = flat_lengths(freq, iM)
        im = min(lens)
    else:
        assert lengths == "single" and vals.size == 1 and runs == "none"
        lens = {im: 1}
    assert len(lens) == 1 or sum(1 << (MAX_LEN - v) for v in lens.values()) == 1 << MAX_LEN  # complete
    codes = canonical(lens)
    len_of, code_of = np.zeros(imageio._HUF_ENCSIZE, np.int64), np.zeros(imageio._HUF_ENCSIZE, np.uint64)
    for s, ln in lens.items():
        len_of[s], code_of[s] = ln, codes[s]
    n = words.size
    key = np.arange(n, dtype=np.float64)           # where a token stands: a word at its position, an escape and its count just before
    tok_code, tok_len = code_of[words], len_of[words]
    if runs == "greedy":  # OpenEXR's writer: a word and up to 255 repeats; the escape where it is cheaper than the repeats written out
        cut = np.flatnonzero(np.diff(words)) + 1
        starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [n]])
        pieces = (ends - starts + 255) // 256
        first = np.repeat(starts, pieces) + 256 * (np.arange(int(pieces.sum())) - np.repeat(np.cumsum(pieces) - pieces, pieces))
        cs = np.minimum(np.repeat(ends, pieces) - first - 1, 255)
        ln = len_of[words[first]]
        esc = ln + len_of[iM] + 8 < ln * cs
        planted = list(zip((first[esc] + 1).tolist(), cs[esc].tolist()))
    elif runs == "none":
        planted = []
    else:
        assert runs == "planted"
    keep = np.ones(n, bool)
    last = 1
    for pos, count in sorted(planted):
        assert last <= pos and pos + count <= n and 0 <= count <= 255 and (words[pos:pos + count] == words[pos - 1]).all(), (pos, count)
        keep[pos:pos + count] = False
        last = pos + count
    if planted:
        at = np.array([p for p, _ in planted], np.float64)
        key = np.concatenate([key[keep], at - 0.5, at - 0.25])
        tok_code = np.concatenate([tok_code[keep], np.full(at.size, codes[iM], np.uint64), np.array([c for _, c in planted], np.uint64)])
        tok_len = np.concatenate([tok_len[keep], np.full(at.size, lens[iM], np.int64), np.full(at.size, 8, np.int64)])
        order = np.argsort(key, kind="stable")
        tok_code, tok_len = tok_code[order], tok_len[order]
    if odd_nbits:  # escapes of 0 repeats behind the last word until the bits stop short of a byte's end
        while int(tok_len.sum()) % 8 == 0:
            assert iM in lens and lens[iM] % 8
            tok_code, tok_len = np.concatenate([tok_code, [np.uint64(codes[iM]), np.uint64(0)]]), np.concatenate([tok_len, [lens[iM], 8]])
    assert tok_len.min() >= 1
    data, nbits = pack_tokens(tok_code, tok_len)
    table, _ = length_table(lens, im, iM)
    table += b"\0" * table_pad
    return struct.pack("<IIIII", im, iM, len(table), nbits, 0) + table + data


def piz_block(planes, chans, bitmap="exact", bit0=False, bitmap_pad=0, empty=(8191, 0), lengths="huffman", runs="greedy", planted=(), table_pad=0,
              hlen_pad=0, odd_nbits=False, seed=1):
    """{name: (rows, cols) float array}, [(name, pixel type)] -> the PIZ block.  A block that comes out at exactly the raw size, which means "stored
    raw" to every reader, gets one more unused byte behind its code bits."""
    rows, cols = planes[chans[0][0]].shape
    words = block_words(planes, chans)
    head, lut, mx = bitmap_and_lut(words, bitmap, bit0, bitmap_pad, empty, seed=seed)
    words = lut[words]
    for pl in word_planes(words, chans, cols, rows):
        imageio._wav2(pl, mx, False)
    huf = huffman_stream(words, lengths, runs, planted, table_pad, odd_nbits)
    if len(head) + 4 + len(huf) + hlen_pad == 2 * words.size:
        hlen_pad += 1
    huf += b"\xa5" * hlen_pad
    return head + struct.pack("<i", len(huf)) + huf


def coded_words(planes, chans, bitmap="exact", bit0=False, seed=1, **_):
    """the words piz_block hands to huffman_stream: what a planted run is placed in"""
    rows, cols = planes[chans[0][0]].shape
    words = block_words(planes, chans)
    _, lut, mx = bitmap_and_lut(words, bitmap, bit0, seed=seed)
    words = lut[words]
    for pl in word_planes(words, chans, cols, rows):
        imageio._wav2(pl, mx, False)
    return words


# ---------------------------------------------------------------- frames
NAMES = [n for v in imageio.AOV_LAYOUT.values() for n in v]
FLOAT_LAYERS = ("velocity", "depth")
# What the tests compare is the four slots AFTER the pack kernel (k0_import.hip), which keeps the bits of direct, velocity and depth (velocity
# only where depth != 1) but squeezes the G-buffer layers: diffuse to floor((x + 1e-4) * 255) per channel, roughness and metalness to
# floor(x * 256 + 0.5), everything >= 1 to one value; normal and emissive to an octahedral pair of halves and RGBE8.  So the contents are k / 128,
# k < 127, in the G-buffer layers — exact in a half, and both squeezes keep any two of them apart (2 k - 2 k / 256 + 0.0255 floors to 2 k up to
# 6 and to 2 k - 1 from 8 on; 2 k + 0.5256 to 2 k) — and integers in direct.  The HALF part starts with direct.R, direct.G and diffuse and ends
# with roughness, metalness, direct.B and direct.A: every word position a run is planted at shows in the slots, whatever word lands there.
# normal and emissive words in the middle are seen only as far as their encodings go.
SQUEEZED = ("diffuse", "normal", "roughness", "metalness", "emissive")
_ORDER = ["direct.R", "direct.G"] + [n for n in NAMES if n.split(".")[0] in ("diffuse", "normal", "emissive")] + ["roughness.Y", "metalness.Y", "direct.B", "direct.A"]
HALF_PART = [(n, HALF) for n in _ORDER]   # 16 words per texel
FLOAT_PART = [(n, FLOAT) for n in NAMES if n.split(".")[0] in FLOAT_LAYERS]     # 6 words per texel
MIXED_PART = [(n, FLOAT if n.split(".")[0] in FLOAT_LAYERS else HALF) for n in NAMES]
BUSY = ("direct.R", "roughness.Y", "depth.Z")
assert sorted(n for n, _ in HALF_PART + FLOAT_PART) == sorted(NAMES)


def half_values(name, idx):
    """indices -> the channel's values: integers where the pack kernel keeps the bits, idx / 128 (idx < 127) in a squeezed layer"""
    idx = np.asarray(idx)
    if name.split(".")[0] in SQUEEZED:
        assert idx.max() < 127
        return (idx / 128.0).astype(np.float32)
    return idx.astype(np.float32)



class Frame:
    """W x H texels; parts: [[(channel, pixel type)]]; rects: [(part, x, y, cols, rows)], scanline 0 the top one; channels: {name: (H, W) float32};
    opts(k, rect) -> piz_block's keywords for block k, or the block's bytes.  blocks: the bytes of each, in the order of rects."""

    def __init__(self, W, H, parts, rects, channels, opts=None):
        self.W, self.H, self.parts, self.rects, self.channels = W, H, parts, rects, channels
        self.blocks = []
        for k, (part, x, y, cols, rows) in enumerate(rects):
            o = opts(k, rects[k]) if opts else {}
            self.blocks.append(o if isinstance(o, bytes) else piz_block(self.block_planes(k), parts[part], **o))

    def block_planes(self, k):
        part, x, y, cols, rows = self.rects[k]
        return {n: self.channels[n][y:y + rows, x:x + cols] for n, _ in self.parts[part]}

    def raw_bytes(self, k):
        part, _, _, cols, rows = self.rects[k]
        return rows * cols * sum(2 if pt == HALF else 4 for _, pt in self.parts[part])

    def raw_block(self, k):
        """block k as the decoders return it: per scanline every channel's samples"""
        part, _, _, _, rows = self.rects[k]
        p = self.block_planes(k)
        return b"".join(p[n][r].astype("<f2" if pt == HALF else "<f4").tobytes() for r in range(rows) for n, pt in self.parts[part])

    def descriptor(self):
        """-> (the blocks' bytes one behind the other as a uint8 array, the imageio.ExrAovLayout that describes them)"""
        from rfx_amd import abi
        feeds = {cn: (pi, j) for pi, key in enumerate(imageio.AOV_LAYOUT) for j, cn in enumerate(imageio.AOV_LAYOUT[key])}
        parts = [(imageio._COMP_PIZ, [(pt,) + feeds[n] for n, pt in chans]) for chans in self.parts]
        rec = np.zeros(len(self.rects), abi.EXR_BLOCK_DTYPE)
        at = 0
        for k, (rect, b) in enumerate(zip(self.rects, self.blocks)):
            rec[k] = rect + (0, at, len(b))
            at += len(b)
        types_ = {n: pt for chans in self.parts for n, pt in chans}
        planes = {key: (len(cn), "half" if all(types_[c] == HALF for c in cn) else "float") for key, cn in imageio.AOV_LAYOUT.items() if cn[0] in types_}
        return np.frombuffer(b"".join(self.blocks), np.uint8), imageio.ExrAovLayout(self.W, self.H, at, parts, None, planes, rec)

    def aov_planes(self, channels=None):
        """Context.stage_aov's planes: frame row 0 is the bottom scanline; a layer of HALF channels is float16"""
        ch = channels or self.channels
        types_ = {n: pt for chans in self.parts for n, pt in chans}
        out = {}
        for key, cn in imageio.AOV_LAYOUT.items():
            if cn[0] not in types_:
                continue
            a = np.stack([ch[c][::-1] for c in cn], -1) if len(cn) > 1 else ch[cn[0]][::-1]
            out[key] = np.ascontiguousarray(a.astype(np.float16 if all(types_[c] == HALF for c in cn) else np.float32))
        return out


def content(W, H, seed, values=1500, palette=2000):
    """seeded channels: a HALF channel draws indices from 0 .. values - 1 (0 .. 126 in a squeezed layer) for half_values — integers, which a half
    holds up to 2048, or 128ths —, a FLOAT channel from `palette` seeded integers below 2^22 (never 1), so its low words vary.  The BUSY channels
    are noise, the others constant over squares of 8 x 8 texels."""
    rng = np.random.default_rng(seed)
    pal = rng.integers(2, 1 << 22, palette)
    y, x = np.mgrid[0:H, 0:W]
    out = {}
    for c, n in enumerate(NAMES):
        isf = n.split(".")[0] in FLOAT_LAYERS
        top = palette if isf else min(values, 127) if n.split(".")[0] in SQUEEZED else values
        v = rng.integers(0, top, (H, W)) if n in BUSY else ((x // 8) * 5 + (y // 8) * 3 + c) % min(7, values) * (1 if isf or top < 127 else 18)
        out[n] = pal[v].astype(np.float32) if isf else half_values(n, v)
    return out


def scanline_rects(parts, W, H):
    return [(p, 0, y, W, min(32, H - y)) for p in range(len(parts)) for y in range(0, H, 32)]


def tile_rects(parts, W, H, tw, th):
    return [(p, x, y, min(tw, W - x), min(th, H - y)) for p in range(len(parts)) for y in range(0, H, th) for x in range(0, W, tw)]


# ---- the stream forms: 70 x 33, per part a scanline block of 32 rows and one of 1 row (no wavelet level)
SW, SH = 70, 33
SPLIT = [HALF_PART, FLOAT_PART]
PLANTED_BLOCK = 1  # the HALF part's block of one row: its 1120 words are the bottom scanline's values themselves, channel after channel


def _few(seed):
    """few symbols, and still 59 or more in every block: squares of 7 values, and in scanlines 5, 6 and the bottom one noise of 64 values"""
    rng = np.random.default_rng(seed)
    pal = rng.integers(2, 1 << 22, 64)
    out = content(SW, SH, seed, values=7, palette=7)
    for n in NAMES:
        v = rng.integers(0, 64, (3, SW))
        out[n][[5, 6, SH - 1]] = pal[v].astype(np.float32) if n.split(".")[0] in FLOAT_LAYERS else half_values(n, v)
    return out


def _bottom_row(ch, values):
    """the bottom scanline of the HALF part's channels <- `values` / 128 (all below 127; a run may cross from one channel into the next, so the
    direct channels take 128ths too), 70 per channel in the part's order: the words of PLANTED_BLOCK up to the lookup, which keeps equal
    values equal and different ones different"""
    ch = {n: v.copy() for n, v in ch.items()}
    for c, (n, _) in enumerate(HALF_PART):
        ch[n][SH - 1] = values[SW * c:SW * (c + 1)] / 128.0
    return ch


def _planted(runs, seed):
    """noise, and in the bottom scanline 1120 values of which no two neighbours are equal but inside the planted runs"""
    rng = np.random.default_rng(seed)
    n = SW * len(HALF_PART)
    v = np.cumsum(rng.integers(1, 39, n)) % 39 + 1  # (steps of 1 .. 38 modulo 39: no accidental repeat)
    for pos, count in runs:
        v[pos:pos + count] = v[pos - 1]
        if pos + count < n and v[pos + count] == v[pos - 1]:
            v[pos + count] += 80
    return _bottom_row(content(SW, SH, seed), v)


def stream_case(name):
    """-> (Frame, claims): claims = {block index: {fact: value}} for tests/test_piz_cases_cpu.py to read off the block's bytes"""
    parts, rects = SPLIT, scanline_rects(SPLIT, SW, SH)
    everywhere = lambda d: {k: d for k in range(len(rects))}  # noqa: E731
    nw = SW * len(HALF_PART)
    planted = {
        "run_of_255_from_64": [(64, 255)],
        "run_from_64": [(64, 5)],
        "run_from_63": [(63, 3)],
        "runs_of_0": [(128, 0), (100, 0)],
        "word_run_alternation": [(p, 1) for p in range(201, 331, 2)],
        "run_of_255_to_nwords": [(nw - 255, 255)],
        "last_word_alone": [(nw - 41, 40)],
    }
    if name in planted:
        runs = sorted(planted[name])
        ch = _planted(runs, 40 + sorted(planted).index(name))
        f = Frame(SW, SH, parts, rects, ch, lambda k, r: dict(runs="planted", planted=runs) if k == PLANTED_BLOCK else {})
        return f, {PLANTED_BLOCK: {"runs": runs, "nwords": nw}}
    if name == "chain":
        return Frame(SW, SH, parts, rects, _few(21), lambda k, r: dict(lengths="chain")), everywhere({"longest": 58})
    if name == "flat":
        return Frame(SW, SH, parts, rects, _few(22), lambda k, r: dict(lengths="flat", runs="none")), everywhere({"shortest_above": FAST_BITS})
    if name == "single":  # every block one value: zero, but 0.5 in the bottom scanline of the HALF part
        ch = {n: np.zeros((SH, SW), np.float32) for n in NAMES}
        for n, _ in HALF_PART:
            ch[n][SH - 1] = 0.5
        return Frame(SW, SH, parts, rects, ch, lambda k, r: dict(lengths="single", runs="none")), everywhere({"codes": 1})
    if name == "superset_bitmap":
        return Frame(SW, SH, parts, rects, content(SW, SH, 23), lambda k, r: dict(bitmap="superset", seed=k)), everywhere({"bitmap": "superset"})
    if name == "full_bitmap_mixed_part":
        mixed = [MIXED_PART]
        return Frame(SW, SH, mixed, scanline_rects(mixed, SW, SH), content(SW, SH, 24), lambda k, r: dict(bitmap="full")), {0: {"mx": 65535}, 1: {"mx": 65535}}
    if name in ("bit0_set", "bit0_clear"):
        return (Frame(SW, SH, parts, rects, content(SW, SH, 25), lambda k, r: dict(bit0=name == "bit0_set")), everywhere({"bit0": name == "bit0_set"}))
    if name == "padded_bitmap_range":
        # (a half's bits are 0 or 0x2000 and more for 1 / 128 and more: zero bytes in front of the first one of the HALF part's blocks)
        return Frame(SW, SH, parts, rects, content(SW, SH, 26), lambda k, r: dict(bitmap_pad=3)), everywhere({"bitmap_pad": 3})
    if name in ("empty_bitmap_8191_0", "empty_bitmap_1_0"):  # the blocks of 32 rows all zero; the bottom scanline noise
        ch = {n: v * (np.arange(SH) == SH - 1)[:, None] for n, v in content(SW, SH, 27).items()}
        e = (8191, 0) if name.endswith("8191_0") else (1, 0)
        return Frame(SW, SH, parts, rects, ch, lambda k, r: dict(empty=e)), {0: {"empty": e, "mx": 0}, 2: {"empty": e, "mx": 0}}
    if name == "padded_table_length":
        return Frame(SW, SH, parts, rects, content(SW, SH, 28), lambda k, r: dict(table_pad=1 + 2 * k)), {k: {"table_pad": 1 + 2 * k} for k in range(4)}
    if name == "padded_hlen":
        return Frame(SW, SH, parts, rects, content(SW, SH, 29), lambda k, r: dict(hlen_pad=1 + 3 * k)), {k: {"hlen_pad": 1 + 3 * k} for k in range(4)}
    assert name == "nbits_not_whole_bytes", name
    return Frame(SW, SH, parts, rects, content(SW, SH, 30), lambda k, r: dict(odd_nbits=True)), everywhere({"odd_nbits": True})


def last_word_alone_in_its_group():
    """65 x 1: depth alone in a HALF part — 65 words, none repeated, no run: the 65th is the only word of the last group, stored by the final
    flush from lane 0 — and every other channel in a second part"""
    W, H = 65, 1
    parts = [[("depth.Z", HALF)], [c for c in MIXED_PART if c[0] != "depth.Z"]]
    ch = content(W, H, 33)
    ch["depth.Z"] = (np.random.default_rng(34).permutation(W)[None, :] + 2).astype(np.float32)  # (never 1: the texel stays covered)
    return Frame(W, H, parts, [(0, 0, 0, W, H), (1, 0, 0, W, H)], ch, lambda k, r: dict(runs="none") if k == 0 else {})


STREAM_CASES = ["chain", "flat", "single", "superset_bitmap", "full_bitmap_mixed_part", "bit0_set", "bit0_clear", "padded_bitmap_range", "empty_bitmap_8191_0",
                "empty_bitmap_1_0", "padded_table_length", "padded_hlen", "nbits_not_whole_bytes", "run_of_255_from_64", "run_from_64", "run_from_63",
                "runs_of_0", "word_run_alternation", "run_of_255_to_nwords", "last_word_alone"]

# ---- the block shapes: one block per part, cols x rows, each in 14-bit arithmetic (the exact bitmap) and modulo 2^16 (the full one)
SHAPES = [(1, 1), (1, 40), (40, 1), (2, 2), (3, 3), (63, 65), (65, 127), (127, 129), (129, 127), (257, 32)]
_frames = {}


def cached(key, make):
    """the frames are built once per process, and never changed"""
    if key not in _frames:
        _frames[key] = make()
    return _frames[key]


def shape_case(cols, rows, w14):
    rects = [(p, 0, 0, cols, rows) for p in range(2)]
    return cached(("shape", cols, rows, w14), lambda: Frame(cols, rows, SPLIT, rects, content(cols, rows, 100 + cols + rows), lambda k, r: {} if w14 else dict(bitmap="full")))


TW, TH, TILE = 200, 140, (127, 129)


def tiled_case():
    return cached("tiled", lambda: Frame(TW, TH, SPLIT, tile_rects(SPLIT, TW, TH, *TILE), content(TW, TH, 7)))
