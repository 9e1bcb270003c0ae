"""CPU (-m "not gpu"): K9's PIZ cores (csrc/k9_piz.h) off the device.  The header and tests/piz_core_driver.cpp are compiled into a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer (their runtimes linked statically; no Python in that process) and run over a corpus
written here; every buffer the program hands the cores has exactly the size the format states, so an access outside one is a sanitizer report,
and the program aborts when a decode costs more loop iterations than input bits + output words.  imageio's _piz_uncompress_block, _huf_uncompress
and _wav2 — the host decode — are the judges."""
import os
import struct
import subprocess

import numpy as np
import pytest

from rfx_amd import imageio

from piz_cases import GAPS, SKEW, Bits, huffman_block, table_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realism-effects_amd", "csrc")
K9_OK = 0
(K9_E_PIZ_BITMAP, K9_E_PIZ_HEADER, K9_E_PIZ_RANGE, K9_E_PIZ_TABLE, K9_E_PIZ_LENGTHS, K9_E_PIZ_CODE, K9_E_PIZ_RUN, K9_E_PIZ_WORDS,
 K9_E_PIZ_TRUNCATED) = range(15, 24)
FAST_BITS = 12  # k9_piz.h K9_PIZ_FAST_BITS
HALF, FLOAT = imageio._PT_HALF, imageio._PT_FLOAT
# (rows, cols) of a word plane; every one also runs transposed
SHAPES = [(1, 1), (1, 40), (3, 1), (5, 3), (6, 33), (17, 33), (32, 31), (32, 97), (64, 70)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k9piz") / "piz_core_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "piz_core_driver.cpp"), "-o", exe])
    return exe


def call(driver, tmp_path, corpus_bytes):
    corpus, results = str(tmp_path / "corpus.bin"), str(tmp_path / "results.bin")
    with open(corpus, "wb") as f:
        f.write(corpus_bytes)
    p = subprocess.run([driver, corpus, results], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert p.returncode == 0, "the driver ended with %d:\n%s" % (p.returncode, p.stderr[-4000:])
    return open(results, "rb").read()


def run_huffman(driver, tmp_path, records):
    """records: [(Huffman block, nwords)] -> [(code, words or None)]"""
    d = call(driver, tmp_path, b"".join(struct.pack("<III", 0, n, len(s)) + s for s, n in records))
    at, out = 0, []
    for s, n in records:
        code, iters = struct.unpack_from("<iQ", d, at)
        at += 12
        assert iters <= 8 * len(s) + n
        out.append((code, np.frombuffer(d, "<u2", n, at) if code == K9_OK else None))
        at += 2 * n if code == K9_OK else 0
    assert at == len(d)
    return out


def run_blocks(driver, tmp_path, records):
    """records: [(PIZ block, chans, cols, rows)] -> [(code, mx, raw bytes or None)]"""
    corpus = b"".join(struct.pack("<IIII", 2, cols, rows, len(chans)) + bytes(1 if pt == HALF else 0 for _, pt in chans) + struct.pack("<I", len(s)) + s
                      for s, chans, cols, rows in records)
    d = call(driver, tmp_path, corpus)
    at, out = 0, []
    for s, chans, cols, rows in records:
        n = 2 * rows * cols * sum(1 if pt == HALF else 2 for _, pt in chans)
        code, iters, mx = struct.unpack_from("<iQi", d, at)
        at += 16
        assert iters <= 8 * len(s) + n // 2
        out.append((code, mx, d[at:at + n] if code == K9_OK else None))
        at += n if code == K9_OK else 0
    assert at == len(d)
    return out


def raw_block(planes, chans):
    """{name: (rows, cols) array of the channel's dtype} -> the scanline-interleaved bytes"""
    rows = next(iter(planes.values())).shape[0]
    return b"".join(planes[name][r].astype("<f2" if pt == HALF else "<f4").tobytes() if planes[name].dtype.kind == "f"
                    else planes[name][r].astype("<u2" if pt == HALF else "<u4").tobytes() for r in range(rows) for name, pt in chans)


def smooth(rows, cols, k=0):
    y, x = np.mgrid[0:rows, 0:cols]
    return (0.5 + 0.4 * np.sin(0.11 * x + 0.3 * k) * np.cos(0.07 * y + k) + 0.001 * ((x * 7 + y * 3) % 5)).astype(np.float32)


def block_corpus():
    """name -> (chans, cols, rows, raw bytes): the contents the writer's PIZ blocks are made of"""
    rng = np.random.default_rng(11)
    out = {}
    for rows, cols in SHAPES:
        chans = [("A", HALF), ("B", HALF)]
        out["smooth_halves_%dx%d" % (rows, cols)] = (chans, cols, rows, raw_block({"A": smooth(rows, cols), "B": smooth(rows, cols, 1)}, chans))
    chans = [("Z", FLOAT)]
    out["float_channel"] = (chans, 33, 17, raw_block({"Z": smooth(17, 33, 2) * 100.0}, chans))
    chans = [("A", HALF), ("Z", FLOAT), ("B", HALF)]
    out["mixed"] = (chans, 97, 32, raw_block({"A": smooth(32, 97), "Z": smooth(32, 97, 3) * 9.0, "B": smooth(32, 97, 4)}, chans))
    chans = [("A", HALF), ("B", HALF)]
    out["constant_planes"] = (chans, 70, 32, raw_block({"A": np.full((32, 70), 0.25, np.float32), "B": np.full((32, 70), 3.5, np.float32)}, chans))
    out["single_value"] = ([("A", HALF)], 40, 8, raw_block({"A": np.full((8, 40), 0x3c00, np.uint16)}, [("A", HALF)]))
    out["zero_only"] = ([("A", HALF)], 40, 8, raw_block({"A": np.zeros((8, 40), np.uint16)}, [("A", HALF)]))
    out["noise"] = ([("A", HALF)], 31, 32, raw_block({"A": rng.integers(0, 3000, (32, 31)).astype(np.uint16)}, [("A", HALF)]))
    ramp = ((7 * np.arange(32 * 640)) % 65536).astype(np.uint16).reshape(32, 640)  # 20480 distinct words: modulo-16-bit arithmetic
    out["ramp_of_20480_values"] = ([("A", HALF)], 640, 32, raw_block({"A": ramp}, [("A", HALF)]))
    return out


def huffman_part(block):
    mn, mxb = struct.unpack_from("<HH", block, 0)
    pos = 4 + (mxb - mn + 1 if mn <= mxb else 0)
    (hlen,) = struct.unpack_from("<i", block, pos)
    return block[pos + 4:pos + 4 + hlen]


def test_blocks_of_the_writer_equal_the_host_decode(driver, tmp_path):
    corpus = block_corpus()
    names = list(corpus)
    records = []
    for name in names:
        chans, cols, rows, raw = corpus[name]
        packed = imageio._piz_compress_block(raw, chans, cols, rows)
        assert imageio._piz_uncompress_block(packed, chans, cols, rows) == raw, name
        records.append((packed, chans, cols, rows))
    mxs = {}
    for name, (packed, chans, cols, rows), (code, mx, got) in zip(names, records, run_blocks(driver, tmp_path, records)):
        words = np.frombuffer(corpus[name][3], "<u2")
        assert mx == np.union1d(words, [0]).size - 1, name
        assert code == K9_OK and got == corpus[name][3], "%s: code %d" % (name, code)
        mxs[name] = mx
    assert mxs["ramp_of_20480_values"] >= 16384 and mxs["mixed"] < 16384 and mxs["zero_only"] == 0 and mxs["single_value"] == 1
    # the Huffman blocks alone: the words before the wavelet, against _huf_uncompress
    hrecords = [(huffman_part(p), rows * cols * sum(1 if pt == HALF else 2 for _, pt in chans)) for p, chans, cols, rows in records]
    for name, (s, n), (code, got) in zip(names, hrecords, run_huffman(driver, tmp_path, hrecords)):
        assert code == K9_OK and (got == imageio._huf_uncompress(s, n)).all(), name


# ---------------------------------------------------------------- hand-made Huffman blocks (the bit writer and the blocks: tests/piz_cases.py)
def test_handmade_huffman_blocks(driver, tmp_path):
    tb = table_bits(GAPS, 0, 300).bits
    assert len(tb) == 6 * 4 + 6 + 2 * 14  # (one short escape, two long ones)
    cases = {
        "codes_up_to_58_bits": (huffman_block(SKEW, 0, 58, list(range(58)) + [("run", 3), 13, 57, ("run", 0), 0]), 58 + 3 + 3),
        "single_symbol_of_length_1": (huffman_block({7: 1}, 7, 8, [7] * 21), 21),
        "both_zero_run_escapes": (huffman_block(GAPS, 0, 300, [0, 4, 105, 4, 0, ("run", 2)]), 7),
        "run_of_255_ends_at_nwords": (huffman_block(GAPS, 0, 300, [105, ("run", 255)]), 256),
        "run_crosses_the_groups_of_64": (huffman_block(GAPS, 0, 300, [0] * 63 + [4, ("run", 200), 105] + [0] * 70 + [("run", 1)]), 63 + 201 + 71 + 1),
    }
    assert max(SKEW.values()) == 58 and min(ln for ln in SKEW.values() if ln > FAST_BITS) == FAST_BITS + 1
    names = sorted(cases)
    for name, (code, got) in zip(names, run_huffman(driver, tmp_path, [cases[n] for n in names])):
        s, n = cases[name]
        assert code == K9_OK and (got == imageio._huf_uncompress(s, n)).all(), "%s: code %d" % (name, code)


def test_every_listed_failure_is_a_code(driver, tmp_path):
    good = huffman_block(GAPS, 0, 300, [0, 4, 105, ("run", 5), 4])
    one = {7: 1}
    cases = {
        "table_length_outside_the_block": (huffman_block(GAPS, 0, 300, [0], tlen=4000), 1, K9_E_PIZ_HEADER),
        "shorter_than_its_header": (good[:19], 9, K9_E_PIZ_HEADER),
        "im_of_65537": (struct.pack("<I", 65537) + good[4:], 9, K9_E_PIZ_RANGE),
        "iM_of_65537": (good[:4] + struct.pack("<I", 65537) + good[8:], 9, K9_E_PIZ_RANGE),
        "table_ends_inside_an_entry": (huffman_block(GAPS, 0, 300, [0], table=Bits().put(6, 2).put(6, 60).put(6, 2).put(6, 63)), 1, K9_E_PIZ_TABLE),
        "zero_run_past_iM": (huffman_block({0: 1, 1: 1}, 0, 3, [0], table=Bits().put(6, 1).put(6, 1).put(6, 61)), 1, K9_E_PIZ_TABLE),
        "over_subscribed": (huffman_block({0: 1, 1: 1, 2: 1}, 0, 2, [0]), 1, K9_E_PIZ_LENGTHS),
        "incomplete_with_two_symbols": (huffman_block({0: 2, 1: 2}, 0, 1, [0]), 1, K9_E_PIZ_LENGTHS),
        "a_bit_pattern_that_is_no_code": (huffman_block(one, 7, 8, [7] * 40)[:22] + b"\x04" + b"\0" * 4, 40, K9_E_PIZ_CODE),
        "run_with_nothing_to_repeat": (huffman_block(GAPS, 0, 300, [("run", 2), 0]), 3, K9_E_PIZ_RUN),
        "run_past_nwords": (huffman_block(GAPS, 0, 300, [0, ("run", 9)]), 9, K9_E_PIZ_RUN),
        "fewer_words": (huffman_block(GAPS, 0, 300, [0, 4, 105]), 4, K9_E_PIZ_WORDS),
        "more_words": (huffman_block(GAPS, 0, 300, [0, 4, 105]), 2, K9_E_PIZ_WORDS),
        "input_ends_inside_a_code": (huffman_block(SKEW, 0, 58, [57, 57, 57])[:-9], 3, K9_E_PIZ_TRUNCATED),
        "input_ends_inside_a_run_count": (huffman_block(GAPS, 0, 300, [0, ("run", 3)], nbits=7), 4, K9_E_PIZ_TRUNCATED),
    }
    assert huffman_block(one, 7, 8, [7] * 40)[22:] == b"\0" * 5
    names = sorted(cases)
    for name, (code, _) in zip(names, run_huffman(driver, tmp_path, [cases[n][:2] for n in names])):
        assert code == cases[name][2], "%s: code %d" % (name, code)
    # the block header: the bitmap's range, the bitmap and hlen against the block's size
    chans = [("A", HALF)]
    blk = imageio._piz_compress_block(raw_block({"A": smooth(4, 9)}, chans), chans, 9, 4)
    mn, mxb = struct.unpack_from("<HH", blk, 0)
    pos = 4 + mxb - mn + 1
    bad = {
        "bitmap_max_of_8192": (struct.pack("<HH", mn, 8192) + blk[4:], K9_E_PIZ_BITMAP),
        "empty_bitmap_from_8192": (struct.pack("<HH", 8192, 0) + blk[4:], K9_E_PIZ_BITMAP),
        "bitmap_outside_the_block": (struct.pack("<HH", 0, 8191) + blk[4:], K9_E_PIZ_HEADER),
        "hlen_outside_the_block": (blk[:pos] + struct.pack("<i", len(blk) - pos - 3) + blk[pos + 4:], K9_E_PIZ_HEADER),
        "negative_hlen": (blk[:pos] + struct.pack("<i", -5) + blk[pos + 4:], K9_E_PIZ_HEADER),
        "hlen_lowered": (blk[:pos] + struct.pack("<i", len(blk) - pos - 4 - 2) + blk[pos + 4:], K9_E_PIZ_TRUNCATED),
        "three_bytes": (blk[:3], K9_E_PIZ_HEADER),
    }
    names = sorted(bad)
    for name, (code, _, _) in zip(names, run_blocks(driver, tmp_path, [(bad[n][0], chans, 9, 4) for n in names])):
        assert code == bad[name][1], "%s: code %d" % (name, code)


@pytest.mark.parametrize("w14", [True, False])
def test_cellwise_wavelet_equals_the_whole_plane(driver, tmp_path, w14):
    rng = np.random.default_rng(5 + w14)
    mx = 16383 if w14 else 65535
    planes = [rng.integers(0, mx + 1, shape).astype(np.uint16) for rows, cols in SHAPES for shape in ((rows, cols), (cols, rows))]
    planes += [rng.integers(0, mx + 1, shape).astype(np.uint16) for shape in ((64, 64), (65, 130), (127, 200), (40, 1), (2, 2))]
    got = call(driver, tmp_path, b"".join(struct.pack("<IIII", 1, p.shape[1], p.shape[0], int(w14)) + p.astype("<u2").tobytes() for p in planes))
    at = 0
    for p in planes:
        want = p.copy()
        imageio._wav2(want, mx, True)
        assert (np.frombuffer(got, "<u2", p.size, at).reshape(p.shape) == want).all(), p.shape
        at += 2 * p.size
    assert at == len(got)


def test_single_byte_mutations_stay_inside_the_buffers(driver, tmp_path):
    """1 200 seeded mutations of the writer's blocks (header, bitmap, length table and code bits alike): the sanitizers and the iteration cap judge
    every one; each is refused with a PIZ code, or decodes — and then to what the host decode returns wherever the host decodes it too"""
    rng = np.random.default_rng(17)
    corpus = block_corpus()
    bases = []
    for name in ("smooth_halves_6x33", "float_channel", "constant_planes", "noise", "smooth_halves_32x31"):
        chans, cols, rows, raw = corpus[name]
        bases.append((imageio._piz_compress_block(raw, chans, cols, rows), chans, cols, rows))
    records = []
    for k in range(1200):
        s, chans, cols, rows = bases[k % len(bases)]
        i = int(rng.integers(0, len(s) if k % 3 else min(len(s), 64)))  # (every third one in the headers and the start of the bitmap)
        records.append((s[:i] + bytes([s[i] ^ int(rng.integers(1, 256))]) + s[i + 1:], chans, cols, rows))
    decoded = 0
    for (s, chans, cols, rows), (code, _, got) in zip(records, run_blocks(driver, tmp_path, records)):
        assert code == K9_OK or 15 <= code <= 23
        if code == K9_OK:
            decoded += 1
            try:
                want = imageio._piz_uncompress_block(s, chans, cols, rows)
            except Exception:  # noqa: BLE001 (the host decode refuses in many ways; what it refuses may still be a stream this rule set takes)
                continue
            assert got == want
    assert 0 < decoded < 1200  # (a changed bitmap byte or low code bit may still decode; a changed header field does not)
