"""Shared by the match-form tests (tests/test_png_matches_cpu.py, test_exr_matches_cpu.py, test_gpu_png_matches.py, test_gpu_exr_matches.py and the
Node twins): inputs that take K8's scanline kernels with MATCHES (csrc/k8_coder.h, include/rfx.h "Match form") to the edges of the token rule, of the sweep's
256-position steps, of the lane's bit accumulator, of the bit window and of the form choice, and a model of the sweep that says how close an
input comes.  Pure NumPy on top of tests/match_device_ref.py.  A case is built from a planted byte sequence d:

    PNG   one scanline, filter None (rfx_stage_png's filter 1): the type byte 0, then the row's bytes — d[0] = 0, d[1:] = the row
    EXR   one scanline of 4 channels: the low bytes of its halfs carry d (t = the running sum of d - 128), the high bytes are 3c throughout —
          a run of 128s behind the planted part, to the last byte — or alternate 3c / 3d where the case wants no repeat of its own

PNG_CASES / EXR_CASES: name -> a function returning (img uint8 (H, W, ch), filter) / halfs float16 (H, W, ch), row 0 = bottom, read-only.  The CPU
tests assert each case's premise, so a case that no longer reaches its edge fails there and not silently on the device."""
import functools
from collections import namedtuple

import numpy as np

import exr_device_ref as X
import match_device_ref as M
import png_device_ref as R

RUN_LENGTHS = (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 519)  # repeating positions: a run of m is m + 1 equal bytes
SIZES = ((5, 3), (97, 55), (128, 72))
STEP, LANES, LANE_POSITIONS = 256, 64, 4  # the kernels' sweep: 64 lanes by 4 positions per step
WINDOW_BITS = 31 + 21 + 255 * R.MAXBITS   # what a step can hold at most: the carry, one match end on the step's first position, 255 literals = 3877
LANE_BITS = 21 + 3 * R.MAXBITS            # ... and a lane: 66

Sweep = namedtuple("Sweep", "steps max_nb over64 matches")


def sweep_model(d):
    """The step arithmetic of the coder's emission (k8_emit) for the sequence d in form (c): every step of 256 positions adds the bits of the
    tokens that END in it behind the pos & 31 bits carried over (the header's bits count as a carry of 31: an upper bound).  -> Sweep(steps =
    the bits in the window per step with the carry counted, max_nb = the most bits one lane packs, over64 = lanes with more than 64, matches)"""
    pos, tok, sym, eb, _, lens = M.coded(d)
    bits = np.asarray(lens, np.int64)[sym] + eb + (tok >= 256)
    n = len(d)
    per_pos = np.zeros((n + STEP - 1) // STEP * STEP, np.int64)
    per_pos[pos] = bits
    lanes = per_pos.reshape(-1, LANES, LANE_POSITIONS).sum(2)
    steps, carry = [], 31
    for s in lanes.sum(1):
        steps.append(carry + int(s))
        carry = steps[-1] & 31
    return Sweep(steps, int(lanes.max()), int((lanes > 64).sum()), int((tok >= 256).sum()))


# ---------------------------------------------------------------- byte sequences
def nonrep(n, seed, first_not=None, last_not=None):
    """n random bytes in 16..79 (six bits of entropy each: the literal form compresses them), no two neighbours equal, the first / last not
    the given value"""
    rng = np.random.default_rng(seed)
    out = rng.integers(16, 80, n).astype(np.int64)
    for i in range(n):
        while (i and out[i] == out[i - 1]) or (i == 0 and out[i] == first_not) or (i == n - 1 and out[i] == last_not):
            out[i] = rng.integers(16, 80)
    return out.astype(np.uint8)


def planted(total, runs, seed=1):
    """a sequence of `total` bytes with d[0] = 0: non-repeating filler with, for every (start, m, value) in runs, `value` (below 16: no filler
    byte) at [start - 1, start + m) — positions start .. start + m - 1 are repeating and nothing else is"""
    d = np.concatenate([[0], nonrep(total - 1, seed)]).astype(np.uint8)
    for start, m, value in runs:
        assert 1 <= start and start + m <= total and value < 16
        d[start - 1:start + m] = value
    return d


def repeating(d):
    d = np.asarray(d)
    return np.flatnonzero(np.concatenate([[False], d[1:] == d[:-1]]))


@functools.lru_cache(maxsize=None)
def deep(end):
    """33097 positions in which form (c)'s code reaches 15 bits — seven frequent values in powers of two, laid out so that no three neighbours
    are equal, over 240 rare ones — with ONE match of 200 that ends on position `end`, a multiple of 256: the first position of a step, and of
    a lane whose other three positions are rare literals (21 + 45 = 66 bits), in a step whose other 255 positions are rare literals too"""
    rng = np.random.default_rng(2000 + end)
    others = rng.permutation(np.repeat(np.arange(2, 8, dtype=np.uint8), [257 << k for k in range(5, -1, -1)]))  # 16191, never neighbours below
    ones = np.ones(others.size + 1, np.int64)
    ones[rng.choice(ones.size, 257 * 64 - ones.size, replace=False)] = 2  # 16448 bytes of value 1 in the gaps, one or two a gap
    frequent = np.concatenate([np.concatenate([[1] * int(k), [o]]) for k, o in zip(ones, np.append(others, 1))])[:-1].astype(np.uint8)
    rare = np.concatenate([np.arange(16, 256), rng.choice(np.arange(16, 256), 16, replace=False)]).astype(np.uint8)
    while True:
        rare = rng.permutation(rare)
        if (rare[1:] != rare[:-1]).all():
            break
    m = 200
    lead = end - m - 1  # frequent bytes behind the type byte
    d = np.concatenate([[0], frequent[:lead], np.full(m + 1, 8), rare, frequent[lead:]]).astype(np.uint8)
    assert d.size == 33097 and (d[end - m:end + 1] == 8).all() and d[end + 1] != 8
    return d


# ---------------------------------------------------------------- PNG: (img, filter)
def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def png_of(d, ch=3):
    """the one-row frame whose filtered scanline under filter None is d (d[0] = 0, the type byte)"""
    d = np.asarray(d, np.uint8)
    assert d[0] == 0 and (d.size - 1) % ch == 0
    return _frozen(d[1:].reshape(1, -1, ch)), 1


def half_flat_bytes(W, H, ch=3, seed=1):
    """png_device_ref.noisy_frame with its right half one colour"""
    img = R.noisy_frame(W, H, ch, seed)
    img[:, W // 2:] = (40, 90, 200, 255)[:ch]
    return _frozen(img)


def ramp_bytes(W, H, ch=3, seed=1):
    """... with its lower half a clean horizontal ramp (Sub leaves runs of 0 and 1)"""
    img = R.noisy_frame(W, H, ch, seed)
    img[:H // 2] = (np.arange(W) * 255 // max(W - 1, 1)).astype(np.uint8)[None, :, None]
    return _frozen(img)


@functools.lru_cache(maxsize=None)
def only_match_loses(kind):
    """a row of 600 bytes without a repeat but for one run of 3: form (c) saves two literals and pays a length symbol and a longer header, so
    it is not smaller and form (a) stays.  Found by search over the seed; the CPU tests assert it."""
    for seed in range(200):
        d = planted(601, [(300, 3, 5)], seed) if kind == "png" else exr_d(planted(600, [(300, 3, 5)], seed), "alternating")
        c, a = (M.png_payload_c(d), R.compressed_payload(d)) if kind == "png" else (M.exr_data_c(d), X.zlib_stream(d))
        if len(c) >= len(a):
            return d
    raise AssertionError("no seed gives the premise")


def run_starts(m):
    """where the run cases plant their runs of m: one long run, or ten short ones at every residue of a lane's four positions"""
    return [7] if m > 4 else [7 + 101 * k for k in range(10)]


PNG_CASES = {"run_%d" % m: functools.partial(lambda m: png_of(planted(1201, [(s, m, 3) for s in run_starts(m)], m)), m) for m in RUN_LENGTHS}
PNG_CASES.update({
    "run_from_d1": lambda: png_of(planted(601, [(1, 20, 0)])),  # the type byte None = 0 = the first residuals
    "run_to_last_byte": lambda: png_of(planted(601, [(560, 41, 2)])),
    "run_across_one_step": lambda: png_of(planted(1201, [(250, 13, 4)])),
    "run_across_two_steps": lambda: png_of(planted(1201, [(250, 271, 4)])),
    "constant_row": lambda: (_frozen(np.zeros((1, 200, 3), np.uint8)), 1),
    "no_repeat": lambda: png_of(planted(601, [])),
    "only_match_loses": lambda: png_of(only_match_loses("png")),
    "stored_row": lambda: (_frozen(np.zeros((1, 1, 3), np.uint8)), 1),  # n = 4 with a match of 3: the stored form stays
    "lane_over_64_bits": lambda: png_of(deep(512)),
    "window_edge": lambda: png_of(deep(256)),
    "long_scanline": lambda: (half_flat_bytes(16386, 1, 4, seed=3), 0),  # 65 544 bytes a row
})
for _W, _H in SIZES:
    PNG_CASES["half_flat_%dx%d" % (_W, _H)] = functools.partial(lambda W, H: (half_flat_bytes(W, H, 3, seed=W), 0), _W, _H)
    PNG_CASES["half_flat_rgba_paeth_%dx%d" % (_W, _H)] = functools.partial(lambda W, H: (half_flat_bytes(W, H, 4, seed=W + 1), 4), _W, _H)
    PNG_CASES["constant_%dx%d" % (_W, _H)] = functools.partial(lambda W, H: (_frozen(np.full((H, W, 3), 77, np.uint8)), 0), _W, _H)
PNG_CASES["ramp_97x55"] = lambda: (ramp_bytes(97, 55), 0)


@functools.lru_cache(maxsize=None)
def png_case(name):
    return PNG_CASES[name]()


# ---------------------------------------------------------------- EXR: halfs
def exr_d(d_low, high="constant"):
    """the predicted bytes of the scanline halfs_of(d_low, high) makes: d_low (padded to whole pixels of 4 channels with non-repeating bytes),
    then the high bytes' part"""
    return X.predict(X.raw_blocks(halfs_of(d_low, high))[0])


def halfs_of(d_low, high="constant"):
    """one scanline of 4 channels whose predicted bytes begin with d_low: (1, W, 4) float16 in [1, 1.5)"""
    d = np.asarray(d_low, np.uint8)
    pad = -d.size % 4
    if pad:
        d = np.concatenate([d, nonrep(pad, 99, first_not=int(d[-1]))])
    W = d.size // 4
    t = (np.cumsum(d.astype(np.int64) - 128) + 128) & 255  # t[0] = d[0], t[i] = t[i - 1] + d[i] - 128
    hi = np.full(4 * W, 0x3c, np.int64)
    if high == "alternating":
        hi[1::2] = 0x3d  # differences +1, -1, ...: 129, 127, ... never a repeat
    bits = (t | (hi << 8)).astype(np.uint16).reshape(4, W)  # the channels in alphabetical order: A, B, G, R
    return _frozen(bits[::-1].T.reshape(1, W, 4).view(np.float16))


def half_flat_halfs(W, H, ch=4, seed=1):
    """exr_device_ref.smooth_noisy_halfs with its right half one colour"""
    a = X.smooth_noisy_halfs(W, H, ch, seed)
    a[:, W // 2:] = np.array((0.25, 0.5, 0.75, 1.0)[:ch], np.float16)
    return _frozen(a)


EXR_CASES = {"run_%d" % m: functools.partial(lambda m: halfs_of(planted(1200, [(s, m, 3) for s in run_starts(m)], m)), m) for m in RUN_LENGTHS}
EXR_CASES.update({
    "run_from_d1": lambda: halfs_of(planted(600, [(1, 20, 0)])),
    "run_to_last_byte": lambda: halfs_of(planted(600, [])),  # the high bytes' 128s
    "run_across_one_step": lambda: halfs_of(planted(1200, [(250, 13, 4)])),
    "run_across_two_steps": lambda: halfs_of(planted(1200, [(250, 271, 4)])),
    "constant_row": lambda: _frozen(np.full((1, 150, 4), 0.5, np.float16)),
    "no_repeat": lambda: halfs_of(planted(600, []), "alternating"),
    "only_match_loses": lambda: halfs_of(only_match_loses("exr")[:600], "alternating"),
    "raw_row": lambda: _frozen(np.array([[[0x3838, 0x3800, 0x3800, 0x3800]]], np.uint16).view(np.float16)),  # n = 8, d = 0 128 128 184 128 128 128 128: a match of 3, and the raw block stays
    "lane_over_64_bits": lambda: halfs_of(deep(512), "alternating"),
    "window_edge": lambda: halfs_of(deep(256), "alternating"),
    "long_scanline": lambda: half_flat_halfs(8193, 1, 4, seed=3),  # 65 544 bytes a row
})
for _W, _H in SIZES:
    EXR_CASES["half_flat_%dx%d" % (_W, _H)] = functools.partial(lambda W, H: half_flat_halfs(W, H, 4, seed=W), _W, _H)
    EXR_CASES["half_flat_rgb_%dx%d" % (_W, _H)] = functools.partial(lambda W, H: half_flat_halfs(W, H, 3, seed=W + 1), _W, _H)
    EXR_CASES["smooth_%dx%d" % (_W, _H)] = functools.partial(lambda W, H: _frozen(X.smooth_noisy_halfs(W, H, 4, seed=W)), _W, _H)


@functools.lru_cache(maxsize=None)
def exr_case(name):
    return EXR_CASES[name]()


def exr_line(name):
    """the predicted bytes of the case's top scanline"""
    return X.predict(X.raw_blocks(exr_case(name))[0])


def png_line(name):
    """the filtered bytes of the case's top scanline"""
    img, filt = png_case(name)
    return R.filtered_rows(img, filt)[0]
