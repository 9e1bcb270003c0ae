"""Shared by tests/test_png_edges_cpu.py and tests/test_gpu_png_edges.py: inputs that take K8 (csrc/k8_png.h over csrc/k8_coder.h) to the edges of its bit window, its
frame shapes, its stored blocks, the choice between the two payload forms, the block header's tokens, the filter ties and the Adler sums, and
a model of the kernel's bit window that says how close a scanline comes.  Pure NumPy on top of tests/png_device_ref.py; every generator is
seeded and returns (img, filter) with img an (H, W, channels) uint8 array (row 0 = bottom) and filter rfx_stage_png's 0..4.  The CPU tests
assert each generator's premise, so a case that no longer reaches its edge fails there and not silently on the device."""
import functools
from collections import namedtuple

import numpy as np

import png_device_ref as R

STEP_BYTES, LANES, LANE_BYTES = 256, 64, 4  # k8_png_rows<false>'s sweep: 64 lanes by 4 bytes per step
WINDOW_BITS = 31 + STEP_BYTES * R.MAXBITS  # what the LDS window is laid out for: 3871

Header = namedtuple("Header", "lens cllens hclen tokens bits cl_depth")
Window = namedtuple("Window", "header_bits first_flush steps max_nb spills tokens")


def block_header(line):
    """the dynamic block's header for a filtered scanline, as compressed_payload states it: the literal lengths, the code-length code, HCLEN,
    the tokens (symbol, extra bits, extra value), the header's bit count and the depth of the code-length code before the limit of 7"""
    freq = np.bincount(line, minlength=257).astype(np.int64)
    freq[256] = 1
    lens = R.code_lengths(freq, R.MAXBITS)
    tokens = R.length_tokens(lens + [0])
    clfreq = [0] * 19
    for t in tokens:
        clfreq[t[0]] += 1
    cllens = R.code_lengths(clfreq, R.CL_MAXBITS)
    hclen = max(4, max(i + 1 for i, s in enumerate(R.CL_ORDER) if cllens[s]))
    bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(cllens[s] + eb for s, eb, _ in tokens)
    return Header(lens, cllens, hclen, tokens, bits, max(R.code_lengths(clfreq, 99)))


def window_model(line):
    """The step arithmetic of k8_png_rows<false> (the literals' sweep of csrc/k8_coder.h, which starts behind the type byte) for a filtered
    scanline (type byte first) in the compressed form: the header and the type byte's code go into the window and whole dwords leave (first_flush = the bits in the window then); every step of 256 bytes adds its lanes' codes behind
    the pos & 31 bits carried over.  -> Window(header_bits, first_flush, steps = the bits in the window per step with the carry counted,
    max_nb = the most bits one lane packs, spills = lanes whose (o & 31) + nb > 64 reach a third dword, tokens = the header's)"""
    line = np.asarray(line, np.uint8)
    h = block_header(line)
    lens = np.asarray(h.lens, np.int64)
    pos = h.bits + int(lens[line[0]])
    first = pos
    pos &= 31
    steps, max_nb, spills = [], 0, 0
    body = line[1:]
    for base in range(0, body.size, STEP_BYTES):
        part = lens[body[base:base + STEP_BYTES]]
        nb = np.zeros(LANES, np.int64)
        np.add.at(nb, np.arange(part.size) // LANE_BYTES, part)
        o = pos + np.concatenate([[0], np.cumsum(nb)[:-1]])
        spills += int(((nb > 0) & ((o & 31) + nb > 64)).sum())
        max_nb = max(max_nb, int(nb.max()))
        pos += int(nb.sum())
        steps.append(pos)
        pos &= 31
    return Window(h.bits, first, steps, max_nb, spills, h.tokens)


def top_line(img, filt):
    """the first scanline of the stream: the tile's top row, filtered"""
    return R.filtered_rows(np.asarray(img, np.uint8), filt)[0]


def _frozen(img):
    img = np.ascontiguousarray(img, np.uint8)
    img.setflags(write=False)
    return img


def _row_of(counts, seed):
    """counts: {byte value: occurrences} -> the shuffled row"""
    vals = np.repeat(np.array(list(counts), np.uint8), list(counts.values()))
    return np.random.default_rng(seed).permutation(vals)


def _two_rows(row, ch=3):
    """the row on top and its reverse below it: both scanlines have the row's histogram"""
    assert row.size % ch == 0
    return _frozen(np.stack([row[::-1], row]).reshape(2, row.size // ch, ch))


# ---------------------------------------------------------------- the bit window at its fullest
DEEP_LEADS = (0, 256, 3)
DEEP_FREQUENT = tuple(range(1, 8))   # seven byte values with counts 257, 514, ..., 257 * 64
DEEP_RARE = tuple(range(16, 256))    # 240 values, 256 draws: each once, sixteen of them twice


@functools.lru_cache(maxsize=None)
def deep_row(lead):
    """10965 x 2 x 3, filter None: seven frequent values in powers of two over 240 rare ones make the unconstrained code 16 deep, so the
    limited one hands out 15-bit codes; the 256 rare bytes stand together at byte `lead` of the row, where one step of the sweep (lead 0, 256)
    or two (lead 3) take them: lanes that pack four 15-bit codes, a window near its 3871 bits"""
    rng = np.random.default_rng(1000 + lead)
    frequent = np.repeat(np.array(DEEP_FREQUENT, np.uint8), [257 << k for k in range(7)])
    rare = np.concatenate([np.array(DEEP_RARE, np.uint8), rng.choice(np.array(DEEP_RARE, np.uint8), 16, replace=False)])
    frequent, rare = rng.permutation(frequent), rng.permutation(rare)
    row = np.concatenate([frequent[:lead], rare, frequent[lead:]])
    assert row.size == 32895
    return _two_rows(row), 1


# ---------------------------------------------------------------- comp_bytes <= stored_bytes at equality and one byte to either side
TIE_K = (78, 79, 80)  # found by search: the first k bytes of the row overwritten with one value
TIE_DIFF = (1, 0, -1)  # len(compressed) - len(stored) of the scanlines: stored, compressed (the tie), compressed


@functools.lru_cache(maxsize=None)
def tie(k):
    """97 x 2 x 3, filter None: a random row whose first k bytes are one value"""
    row = np.random.default_rng(7).integers(0, 256, 291, dtype=np.uint8)
    row[:k] = 7
    return _frozen(np.stack([row, row]).reshape(2, 97, 3)), 1


# ---------------------------------------------------------------- stored blocks
STORED_EDGES = ((21845, 3, 2), (32768, 4, 3))  # (W, channels, blocks): n = 65536 -> a second block of one byte; n = 131073 -> a third of three


@functools.lru_cache(maxsize=None)
def stored_block_edges(W, ch):
    return _frozen(np.random.default_rng(W + ch).integers(0, 256, (2, W, ch), dtype=np.uint8)), 0


# ---------------------------------------------------------------- Adler partial sums, chunk counts
@functools.lru_cache(maxsize=None)
def largest_adler():
    """32768 x 3 x 4 of 255s, filter None: the largest s1 and s2 a scanline can have"""
    return _frozen(np.full((3, 32768, 4), 255, np.uint8)), 1


@functools.lru_cache(maxsize=None)
def many_rows():
    """1 x 32768 x 3 random, adaptive: 32768 chunks (512 rounds of k8_png_scan's loop), every `up` one pixel"""
    return _frozen(np.random.default_rng(32768).integers(0, 256, (32768, 1, 3), dtype=np.uint8)), 0


# ---------------------------------------------------------------- tiny frames and rows that straddle one step
TINY_SIZES = ((1, 1), (1, 5), (5, 1), (64, 1), (2, 64), (3, 65), (85, 2), (86, 2), (64, 2))  # (W, H)
TINY = tuple((W, H, ch, filt) for (W, H) in TINY_SIZES for ch in (3, 4) for filt in (0, 4))


@functools.lru_cache(maxsize=None)
def tiny(W, H, ch, filt):
    if W * H < 70:
        img = np.random.default_rng(W * 1000 + H * 10 + ch).integers(0, 256, (H, W, ch), dtype=np.uint8)
    else:
        img = R.noisy_frame(W, H, ch, seed=W * 1000 + H * 10 + ch)
    return _frozen(img), filt


# ---------------------------------------------------------------- header tokens
def _dyadic_row(counts, nbytes, seed):
    """counts: {value: occurrences} for values above 0; byte 0 takes what is left of `nbytes`"""
    counts = dict(counts)
    rest = nbytes - sum(counts.values())
    assert rest >= 0 and 0 not in counts
    if rest:
        counts[0] = rest
    return _row_of(counts, seed)


def _runs(spec):
    """spec: (gap, run, count) triples laid out from byte value 1 upwards: `gap` unused values, then `run` consecutive values `count` times each
    -> ({value: count}, the next free value)"""
    counts, v = {}, 1
    for gap, run, count in spec:
        v += gap
        for _ in range(run):
            counts[v] = count
            v += 1
    assert v <= 256
    return counts, v


TOKEN_FRAMES = ("runs", "gap138", "gap139", "gap140", "gap149", "two_symbols", "fibonacci", "deep_cl", "deep_row")


@functools.lru_cache(maxsize=None)
def token_corners(name):
    """frames with filter None whose first scanline's alphabet is planted: gaps in it are the zero runs, consecutive values with equal counts
    the non-zero runs of the header's code-length sequence"""
    if name == "runs":
        # with the type byte and the end-of-block symbol the scanline's counts sum to 512 = 2^9 and each is a power of two, so the lengths
        # are 9 - log2(count): runs of 7 (length 5), 8, 9, 10 and 4 (length 6) behind zero runs of 1, 2, 3, 10 and 11, then 4, 3, 5
        counts, _ = _runs(((1, 7, 16), (2, 8, 8), (3, 9, 8), (10, 10, 8), (11, 4, 8), (4, 1, 16), (3, 1, 4), (5, 1, 2), (1, 1, 1)))
        return _two_rows(_dyadic_row(counts, 510, 1)), 1
    if name in ("gap138", "gap139", "gap140", "gap149"):
        v = int(name[3:]) + 1  # values 1 .. v - 1 unused
        return _two_rows(_dyadic_row({v: 150}, 300, 2)), 1
    if name == "two_symbols":  # byte 0 and the end of block: one bit each
        return _frozen(np.zeros((2, 100, 3), np.uint8)), 1
    if name == "fibonacci":
        # the type byte and the end of block once each, the row's fifteen values 2, 3, 5, ..., 1597 times (the last one padded to whole
        # pixels): the unconstrained code is 16 deep, the limited one has the lengths up to 15
        fib = [2, 3]
        while len(fib) < 15:
            fib.append(fib[-1] + fib[-2])
        fib[-1] += -sum(fib) % 3
        return _two_rows(_row_of({3 * i + 2: c for i, c in enumerate(fib[::-1])}, 3)), 1
    if name == "deep_cl":
        # byte values 1..127 take their length from the ruler sequence (the trailing zeros of the value: 64 values 4 times each, 32 values
        # 8 times, ..., one value 256 times), so no two neighbours share a length, nothing becomes a run, and the lengths' own frequencies
        # 64, 32, ..., 1 make the code-length code itself deeper than its limit of 7
        counts = {v: 4 << ((v & -v).bit_length() - 1) for v in range(1, 128)}
        return _two_rows(_dyadic_row(counts, sum(counts.values()) + 128, 4)), 1
    if name == "deep_row":  # lengths 14 and 15 side by side
        return deep_row(0)
    raise ValueError(name)


# what the family's headers must contain, as (what, predicate over one header's token list)
def _zero_runs(tokens):
    """the lengths of the zero runs a token list spells"""
    out, r = [], 0
    for s, _, ev in tokens:
        if s == 18:
            r += ev + 11
        elif s == 17:
            r += ev + 3
        elif s == 0:
            r += 1
        else:
            if r:
                out.append(r)
            r = 0
    if r:
        out.append(r)
    return out


def _nonzero_runs(tokens):
    """(run length, its tokens) for every non-zero run"""
    out, i = [], 0
    while i < len(tokens):
        s = tokens[i][0]
        if 1 <= s <= 15:
            j, n = i + 1, 1
            while j < len(tokens) and (tokens[j][0] == 16 or tokens[j][0] == s):
                n += tokens[j][2] + 3 if tokens[j][0] == 16 else 1
                j += 1
            out.append((n, [t[::2] for t in tokens[i:j]]))
            i = j
        else:
            i += 1
    return out


def token_coverage(token_lists):
    """-> the sorted names of the corners the token lists reach, out of TOKEN_CORNERS"""
    got = set()
    for tokens in token_lists:
        pairs = [(s, ev) for s, _, ev in tokens]
        for s, ev in pairs:
            got.add("symbol %d" % s)
            if (s, ev) in ((18, 0), (18, 127), (17, 0), (17, 7), (16, 0), (16, 3)):
                got.add("(%d, %d)" % (s, ev))
        for k in range(len(pairs)):
            if pairs[k] == (18, 127) and pairs[k + 1:k + 2] == [(18, 0)]:
                got.add("zero run 149 as (18, 127) (18, 0)")
            if pairs[k] == (18, 127) and pairs[k + 1:k + 2] == [(0, 0)] and pairs[k + 2:k + 3] != [(0, 0)]:
                got.add("zero run 139 as (18, 127) 0")
            if pairs[k] == (18, 127) and pairs[k + 1:k + 3] == [(0, 0), (0, 0)] and pairs[k + 3:k + 4] != [(0, 0)]:
                got.add("zero run 140 as (18, 127) 0 0")
        for r in _zero_runs(tokens):
            if r in (1, 2, 10, 11, 138, 139, 140, 149):
                got.add("zero run %d" % r)
        for n, toks in _nonzero_runs(tokens):
            v = toks[0]
            want = {7: [v, (16, 3)], 8: [v, (16, 3), v], 9: [v, (16, 3), v, v], 10: [v, (16, 3), (16, 0)]}
            if n in want and toks == want[n]:
                got.add("non-zero run %d" % n)
    return sorted(got)


TOKEN_CORNERS = sorted(
    ["symbol %d" % s for s in range(19)] + ["(18, 0)", "(18, 127)", "(17, 0)", "(17, 7)", "(16, 0)", "(16, 3)"]
    + ["zero run %d" % r for r in (1, 2, 10, 11, 138, 139, 140, 149)]
    + ["zero run 139 as (18, 127) 0", "zero run 140 as (18, 127) 0 0", "zero run 149 as (18, 127) (18, 0)"]
    + ["non-zero run %d" % n for n in (7, 8, 9, 10)])


# ---------------------------------------------------------------- adaptive filter ties
FILTER_TIES = (("up_paeth", 2), ("sub_paeth", 1))  # (name, the type every scanline below the first must get)


@functools.lru_cache(maxsize=None)
def filter_ties(name):
    """97 x 4 x 3, adaptive.  up_paeth: every row a copy of a noisy row, so Up and Paeth both cost 0 and the lower type number, Up, wins.
    sub_paeth: every row constant along x and twice the row below it (mod 256): Sub leaves the first pixel x, Paeth predicts it from above and
    leaves x - 2 x = -x at the same cost, both far below None and Up"""
    if name == "up_paeth":
        row = R.noisy_frame(97, 1, 3, seed=21)[0]
        return _frozen(np.stack([row] * 4)), 0
    if name == "sub_paeth":
        colours = (np.array([5, 11, 23]) * np.array([[1], [2], [4], [8]])).astype(np.uint8)  # bottom row first: each row is twice the one below
        return _frozen(np.repeat(colours[:, None, :], 97, axis=1)), 0
    raise ValueError(name)


# ---------------------------------------------------------------- every case, by name
def all_cases():
    """(id, generator call) for every case of this module; the frames are built (and cached) when the call is made"""
    cases = [("deep_row-lead%d" % lead, functools.partial(deep_row, lead)) for lead in DEEP_LEADS]
    cases += [("tie-k%d" % k, functools.partial(tie, k)) for k in TIE_K]
    cases += [("stored-%dx2x%d" % (W, ch), functools.partial(stored_block_edges, W, ch)) for (W, ch, _) in STORED_EDGES]
    cases += [("largest_adler", largest_adler), ("many_rows", many_rows)]
    cases += [("tiny-%dx%dx%d-f%d" % c, functools.partial(tiny, *c)) for c in TINY]
    cases += [("tokens-" + n, functools.partial(token_corners, n)) for n in TOKEN_FRAMES if n != "deep_row"]
    cases += [("filter_tie-" + n, functools.partial(filter_ties, n)) for n, _ in FILTER_TIES]
    return cases


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """-> (img, filter, the restatement's result prefix), computed once per process"""
    img, filt = dict(all_cases())[case_id]()
    return img, filt, R.result_prefix(img, filt)
