"""CPU (-m "not gpu"): the blocks tests/piz_cases.py writes for tests/test_gpu_exr_piz_edges.py, before a device sees them.  The claims: what
every case is meant to hold is read off the bytes of its blocks — the bitmap and mx, the code lengths, the framing fields, and for the planted
runs the escapes found by walking the code bits.  The reference: every block goes through imageio's host decode and through the stand-alone
sanitized driver of tests/test_piz_core_cpu.py (csrc/k9_piz.h with K9PizHostIO), and both must return the planes the block was made from — the
expectation the device test holds the decode to is right by construction, and two decoders that share no code with the writer agree with it."""
import struct

import numpy as np
import pytest

import piz_cases as PC
import test_gpu_exr_piz as P
from rfx_amd import imageio
from test_piz_core_cpu import K9_OK, driver, run_blocks  # noqa: F401 (the fixture that builds the driver is shared)


def facts(blk, walk=False):
    """one PIZ block's bytes -> what they state"""
    f = {}
    mn, mxb = struct.unpack_from("<HH", blk, 0)
    n = mxb - mn + 1 if mn <= mxb else 0
    f["range"], f["bitmap"] = (mn, mxb), np.frombuffer(blk, np.uint8, n, 4)
    whole = np.zeros(8192, np.uint8)
    whole[mn:mn + n] = f["bitmap"]
    f["bit0"] = bool(whole[0] & 1)
    f["values"] = int(np.unpackbits(whole).sum()) - int(f["bit0"])  # the nonzero values with a bit
    f["mx"] = f["values"]
    pos = 4 + n
    (hlen,) = struct.unpack_from("<i", blk, pos)
    assert pos + 4 + hlen == len(blk)
    im, iM, tlen, nbits, zero = struct.unpack_from("<IIIII", blk, pos + 4)
    f.update(hlen=hlen, im=im, iM=iM, tlen=tlen, nbits=nbits)
    tb = np.unpackbits(np.frombuffer(blk, np.uint8, tlen, pos + 24))
    six = lambda at: int(np.packbits(tb[at:at + 6])[0]) >> 2  # noqa: E731
    at, i, lengths = 0, im, {}
    while i <= iM:
        ln = six(at)
        at += 6
        if ln == 63:
            i += int(np.packbits(tb[at:at + 8])[0]) + 6
            at += 8
        elif ln >= 59:
            i += ln - 57
        else:
            if ln:
                lengths[i] = ln
            i += 1
    assert i == iM + 1
    f["lengths"], f["table_used"] = lengths, (at + 7) // 8
    f["table_tail"] = bytes(blk[pos + 24 + f["table_used"]:pos + 24 + tlen])
    f["code_bytes"] = hlen - 20 - tlen
    if walk:
        inv = {(ln, c): s for s, c in PC.canonical(lengths).items() for ln in [lengths[s]]}
        lens = sorted(set(lengths.values()))
        data = blk[pos + 24 + tlen:pos + 24 + tlen + (nbits + 7) // 8]
        db, total = int.from_bytes(data, "big"), 8 * len(data)
        bp, nw, runs = 0, 0, []
        while bp < nbits:
            for ln in lens:
                s = inv.get((ln, (db >> (total - bp - ln)) & ((1 << ln) - 1)))
                if s is not None:
                    break
            assert s is not None
            bp += ln
            if s == iM:
                cs = (db >> (total - bp - 8)) & 255
                bp += 8
                runs.append((nw, cs))
                nw += cs
            else:
                nw += 1
        assert bp == nbits
        f["runs"], f["nwords"] = runs, nw
    return f


def check_reference(driver, tmp_path, frame, what):
    """every block of the frame through both decoders: the planes it was made from, and the mx its bitmap states"""
    records = []
    for k, ((part, _, _, cols, rows), blk) in enumerate(zip(frame.rects, frame.blocks)):
        assert len(blk) != frame.raw_bytes(k), "%s: block %d has the raw size" % (what, k)
        chans = frame.parts[part]
        assert imageio._piz_uncompress_block(blk, chans, cols, rows) == frame.raw_block(k), "%s: the host decode of block %d" % (what, k)
        records.append((blk, chans, cols, rows))
    for k, (code, mx, got) in enumerate(run_blocks(driver, tmp_path, records)):
        assert code == K9_OK and got == frame.raw_block(k), "%s: the driver on block %d, code %d" % (what, k, code)
        assert mx == facts(frame.blocks[k])["mx"]


@pytest.mark.parametrize("name", PC.STREAM_CASES)
def test_stream_case_holds_what_it_claims_and_decodes_to_its_planes(driver, tmp_path, name):
    frame, claims = PC.stream_case(name)
    assert (frame.W, frame.H) == (70, 33) and sorted({r[4] for r in frame.rects}) == [1, 32] and all(r[3] == 70 for r in frame.rects)
    data, lay = frame.descriptor()
    fast = P.block_facts(data, lay)  # (test_gpu_exr_piz's reader of the same bytes)
    assert len(fast) == len(frame.blocks)
    assert claims
    for k, blk in enumerate(frame.blocks):
        c = claims.get(k, {})
        f = facts(blk, walk="runs" in c)
        L = f["lengths"]
        assert fast[k][0] == f["mx"] and fast[k][1] == max(L.values())
        words = np.frombuffer(frame.raw_block(k), "<u2")
        distinct = np.setdiff1d(words, [0]).size
        if c.get("bitmap") == "superset":
            assert f["values"] == distinct + 256 and f["mx"] < 16384
        elif "mx" not in c:
            assert f["values"] == distinct and f["mx"] < 16384  # exact
        if "mx" in c:
            assert f["mx"] == c["mx"]
            if c["mx"] == 65535:
                assert f["range"] == (0, 8191) and (f["bitmap"] == 255).all() and distinct < 16384
        if "longest" in c:
            assert max(L.values()) == c["longest"] == 58 == L[f["iM"]] and min(L.values()) == 1 and len(L) >= 59
        if "shortest_above" in c:
            assert min(L.values()) > c["shortest_above"] == 12 and len(set(L.values())) == 1 and len(L) == 1 << max(L.values())
        if "codes" in c:
            assert len(L) == c["codes"] == 1 and list(L.values()) == [1] and f["iM"] not in L and f["nbits"] == words.size
        if "bit0" in c:
            assert f["bit0"] == c["bit0"] and (k >= 2 or (words == 0).any())  # (the HALF blocks hold the value 0)
            assert f["range"][0] == 0 if c["bit0"] else f["range"][0] > 0
        if "bitmap_pad" in c and k < 2:  # the HALF part's blocks: their values leave room on both sides
            p = c["bitmap_pad"]
            assert not f["bitmap"][:p].any() and not f["bitmap"][-p:].any() and f["bitmap"][p] and f["bitmap"][-p - 1]
        if "empty" in c:
            assert f["range"] == c["empty"] and f["bitmap"].size == 0 and not words.any()
        if "table_pad" in c:
            assert f["tlen"] - f["table_used"] == c["table_pad"] > 0 and f["table_tail"] == b"\0" * c["table_pad"]
        else:
            assert f["tlen"] == f["table_used"]
        if "hlen_pad" in c:
            assert f["code_bytes"] - (f["nbits"] + 7) // 8 in (c["hlen_pad"], c["hlen_pad"] + 1) and c["hlen_pad"] > 0
        else:
            assert f["code_bytes"] - (f["nbits"] + 7) // 8 in (0, 1)  # (1: the byte that keeps the block off the raw size)
        if "odd_nbits" in c:
            assert f["nbits"] % 8 != 0
        if "runs" in c:
            assert f["runs"] == c["runs"] and f["nwords"] == c["nwords"] == words.size == 1120 and f["nwords"] & 63, f["runs"]
    check_reference(driver, tmp_path, frame, name)


def test_the_planted_runs_stand_where_the_wave_io_has_its_edges():
    runs = {}
    for name in PC.STREAM_CASES:
        if name.startswith(("run", "word_run", "last_word")):
            frame, claims = PC.stream_case(name)
            runs[name] = facts(frame.blocks[PC.PLANTED_BLOCK], walk=True)["runs"]
    n = 1120
    assert runs["run_of_255_from_64"] == [(64, 255)] and runs["run_from_64"][0][0] & 63 == 0  # right after the flush at position 63
    assert runs["run_from_63"][0][0] & 63 == 63
    assert sorted(runs["runs_of_0"]) == [(100, 0), (128, 0)]  # mid-group, and at a group's start
    assert runs["word_run_alternation"] == [(p, 1) for p in range(201, 331, 2)]  # word, run, word, run over 130 words, across two groups' ends
    assert runs["run_of_255_to_nwords"] == [(n - 255, 255)] and n & 63 == 32  # ends at nwords, in a last group that is partial
    (p, c), = runs["last_word_alone"]
    assert p + c == n - 1 and (n - 1) & 63  # the run ends one word before the block does: the last word waits alone, not at a group's start


def test_last_word_alone_in_its_group(driver, tmp_path):
    frame = PC.last_word_alone_in_its_group()
    f = facts(frame.blocks[0], walk=True)
    assert f["nwords"] == 65 and f["nwords"] & 63 == 1 and f["runs"] == [] and len(f["lengths"]) == 66  # 65 different words and the escape
    check_reference(driver, tmp_path, frame, "65 words")


def test_the_pack_kernel_keeps_the_planted_values_apart():
    """k0_import.hip's two squeezes restated in float32 — diffuse: floor(min(x + 1e-4, 0.999999) * 255), roughness and metalness:
    floor(min(x + 1e-4, 0.999999) * 256 + 0.5) — are one-to-one on k / 128, k < 127, and send no such value where an integer >= 1 goes"""
    x = (np.arange(127) / 128.0).astype(np.float16).astype(np.float32)
    assert (x == np.arange(127, dtype=np.float32) / np.float32(128)).all()  # exact in a half
    f = np.float32
    lim = lambda v: np.minimum(v + f(0.0001), f(0.999999))  # noqa: E731
    for squeeze in (lambda v: np.floor(lim(v) * f(255)), lambda v: np.floor(lim(v) * f(256) + f(0.5))):
        out = squeeze(x)
        assert np.unique(out).size == 127 and squeeze(np.array([1, 5, 119], f))[0] not in out
    # the planted row holds nothing else, and its runs stand in direct, diffuse, roughness and metalness alone
    order = [n for n, _ in PC.HALF_PART]
    assert order[:6] == ["direct.R", "direct.G", "diffuse.R", "diffuse.G", "diffuse.B", "diffuse.A"] and order[-4:] == ["roughness.Y", "metalness.Y", "direct.B", "direct.A"]
    for name in PC.STREAM_CASES:
        if name.startswith(("run", "word_run", "last_word")):
            frame, claims = PC.stream_case(name)
            row = np.concatenate([frame.channels[n][PC.SH - 1] for n in order])
            assert ((row * 128 == np.round(row * 128)) & (row * 128 < 127) & (row > 0)).all()
            for pos, count in claims[PC.PLANTED_BLOCK]["runs"]:
                assert pos + count <= 6 * PC.SW or pos - 1 >= 12 * PC.SW, name


def test_length_table_and_bit_packer_equal_the_bit_by_bit_writer():
    """the vectorised packer and length table of piz_cases against its Bits / table_bits, which test_piz_core_cpu.py's blocks are made with"""
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 59, 500)
    codes = [int(rng.integers(0, 1 << 62)) & ((1 << int(ln)) - 1) for ln in lens]
    b = PC.Bits()
    for ln, c in zip(lens, codes):
        b.put(int(ln), c)
    assert PC.pack_tokens(codes, lens) == (b.bytes(), len(b.bits))
    for lengths, im, iM in ((PC.GAPS, 0, 300), (PC.SKEW, 0, 58), ({7: 1}, 7, 8), ({5: 3, 2000: 9, 2001: 9, 65536: 2}, 5, 65536), ({0: 1, 1: 1}, 0, 700)):
        t = PC.table_bits(lengths, im, iM)
        assert PC.length_table(lengths, im, iM) == (t.bytes(), len(t.bits))


@pytest.mark.parametrize("cols,rows", PC.SHAPES, ids=lambda v: str(v))
def test_shape_case_decodes_to_its_planes(driver, tmp_path, cols, rows):
    for w14 in (True, False):
        frame = PC.shape_case(cols, rows, w14)
        for k, blk in enumerate(frame.blocks):
            f = facts(blk)
            assert f["mx"] < 16384 if w14 else f["mx"] == 65535
            assert frame.rects[k][3:] == (cols, rows)
        if (cols, rows) == (1, 1):
            assert all(len(b) > frame.raw_bytes(k) for k, b in enumerate(frame.blocks))  # packed > raw: a stream all the same
        check_reference(driver, tmp_path, frame, "%d x %d, %s" % (cols, rows, "14-bit" if w14 else "16-bit"))


def test_tiled_case_decodes_to_its_planes(driver, tmp_path):
    frame = PC.tiled_case()
    assert sorted(r[3:] for r in frame.rects if r[0] == 0) == [(73, 11), (73, 129), (127, 11), (127, 129)]
    check_reference(driver, tmp_path, frame, "tiled")
