"""CPU (-m "not gpu"): the premises of tests/png_edge_cases.py, one assertion each — every case reaches the edge of K8 it is named after — and the
restatement's own result for every case as a valid PNG (zlib over the IDAT payloads, imageio.read_png) before the device is asked for it in
tests/test_gpu_png_edges.py.  Also the two places where tests/png_device_ref.py is evaluated faster than it is stated: the filter choice for
all scanlines at once against choose_filter per scanline, and the lower bound that spares payload() the compressed form of a tiny line."""
import struct
import zlib

import numpy as np
import pytest

import png_device_ref as R
import png_edge_cases as E
from rfx_amd import imageio

CASES = E.all_cases()


def chunks(data):
    """the chunks of a file body -> [(tag, payload)], every CRC checked"""
    out, pos = [], 0
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        out.append((tag, body))
        pos += 12 + n
    assert pos == len(data)
    return out


def _forms(img, filt):
    """per scanline: (len(compressed) - len(stored), the payload's form 'a' / 'b')"""
    out = []
    for l in R.filtered_rows(img, filt):
        a, b = R.compressed_payload(l), R.stored_payload(l)
        out.append((len(a) - len(b), "a" if R.payload(l) == a else "b"))
    return out


# ---------------------------------------------------------------- the window model
def test_window_model_counts_the_bits_the_restatement_packs():
    lines = [E.top_line(*E.deep_row(3)), E.top_line(*E.token_corners("runs")), E.top_line(R.noisy_frame(97, 5, 4), 4), E.top_line(*E.tiny(1, 1, 3, 0))]
    for line in lines:
        w, h = E.window_model(line), E.block_header(line)
        lens = np.asarray(h.lens)
        bits = w.header_bits + int(lens[line].sum()) + h.lens[256] + 3  # header, the literals (type byte included), end of block, the stored block's 3
        assert (bits + 7) // 8 + 4 == len(R.compressed_payload(line))
        assert len(w.steps) == (line.size - 1 + 255) // 256 and w.tokens == h.tokens
        # the window's bits, carries taken out, are the header's, the type byte's and the literals'
        total = w.first_flush + sum(s - (p & 31) for s, p in zip(w.steps, [w.first_flush] + w.steps[:-1]))
        assert total == w.header_bits + int(lens[line].sum())
        assert max([w.first_flush] + w.steps) <= E.WINDOW_BITS and w.max_nb <= 4 * R.MAXBITS


@pytest.mark.parametrize("lead", E.DEEP_LEADS)
def test_deep_row_fills_the_window(lead):
    img, filt = E.deep_row(lead)
    assert img.shape == (2, 10965, 3) and filt == 1
    for line in R.filtered_rows(img, filt):
        assert line.size == 32896 and line[0] == 0
        freq = np.bincount(line, minlength=257)
        freq[256] = 1
        assert sorted(freq[list(E.DEEP_FREQUENT)]) == [257 << k for k in range(7)]
        assert (freq[list(E.DEEP_RARE)] > 0).all() and freq[list(E.DEEP_RARE)].sum() == 256
        assert max(R.code_lengths(freq, 99)) == 16
        assert max(R.code_lengths(freq, R.MAXBITS)) == 15
        assert len(R.compressed_payload(line)) < len(R.stored_payload(line))  # form (a): the window is used at all
    w = E.window_model(R.filtered_rows(img, filt)[0])  # the top scanline: the rare run at byte `lead`
    print("deep_row lead %d: header %d bits, fullest step %d of %d bits, max nb %d, %d lanes spill into a third dword"
          % (lead, w.header_bits, max(w.steps), E.WINDOW_BITS, w.max_nb, w.spills))
    assert max(w.steps) >= 3700
    assert w.max_nb == 60
    assert w.spills > 40
    fullest = int(np.argmax(w.steps))
    assert fullest == (1 if lead == 256 else 0)  # the step that takes the run (lead 3: most of it)


def test_tie_is_one_byte_to_either_side_of_equal():
    got = []
    for k, want in zip(E.TIE_K, E.TIE_DIFF):
        img, filt = E.tie(k)
        assert img.shape == (2, 97, 3) and filt == 1
        forms = _forms(img, filt)
        assert [d for d, _ in forms] == [want, want]
        got.append(forms[0][1])
    assert E.TIE_DIFF == (1, 0, -1)
    assert got == ["b", "a", "a"]  # stored; compressed at the tie; compressed


@pytest.mark.parametrize("edge", E.STORED_EDGES, ids=lambda e: "%dx%d-%dblocks" % e)
def test_stored_block_edges_take_form_b(edge):
    W, ch, blocks = edge
    img, filt = E.stored_block_edges(W, ch)
    n = 1 + W * ch
    assert img.shape == (2, W, ch) and blocks == (n + 65534) // 65535
    assert n - (blocks - 1) * 65535 == {2: 1, 3: 3}[blocks]  # the last block: one byte, three bytes
    frag, _, _, raw, payloads = R.fragment(img, filt)
    for p in payloads:
        assert len(p) == n + 5 * blocks
        last = (blocks - 1) * 65540
        tail = n - (blocks - 1) * 65535
        assert p[last] == 0 and struct.unpack("<HH", p[last + 1:last + 5]) == (tail, tail ^ 0xFFFF)
    assert len(frag) == 2 * (12 + 5 * blocks + n) and 32 + len(frag) == R.bound(W, 2, ch)


def test_largest_adler_sums():
    img, filt = E.largest_adler()
    assert img.shape == (3, 32768, 4) and filt == 1 and (img == 255).all()
    lines = R.filtered_rows(img, filt)
    n = lines[0].size
    assert n == 131073
    s1 = sum(int(v) for v in lines[0].tolist())
    s2 = sum((n - i) * int(v) for i, v in enumerate(lines[0].tolist()))  # the kernel's weights: n - position, the type byte at position 0
    assert s1 == 255 * 131072 and s2 > 2 ** 40
    for line in lines:
        h = E.block_header(line)
        assert [i for i, l in enumerate(h.lens) if l] == [0, 255, 256] and h.lens[255] == 1  # one literal apart from the type byte
        assert len(R.compressed_payload(line)) < len(R.stored_payload(line))


def test_many_rows_premise():
    img, filt = E.many_rows()
    assert img.shape == (32768, 1, 3) and filt == 0
    assert (32768 + 63) // 64 == 512  # rounds of k8_png_scan's loop
    frag, _, _, raw, payloads = R.fragment(img, filt)
    assert len(payloads) == 32768 and raw == 32768 * 4
    # one pixel per row: Sub is None and Paeth is Up, so the ties leave None and Up, and both occur
    assert {int(l[0]) for l in R.filtered_rows(img, filt)} == {0, 2}
    assert all(len(p) == 4 + 5 for p in payloads)  # every `up` one pixel, every chunk in form (b)


def test_tiny_shapes():
    assert len(E.TINY) == 36
    rowbytes = {W * ch for (W, H, ch, _) in E.TINY}
    assert rowbytes >= {3, 4, 255, 256, 258, 340, 344}  # one lane; one step less a byte, exactly, and more
    assert {H for (_, H, _, _) in E.TINY} >= {1, 2, 5, 64, 65}
    for c in E.TINY:
        img, filt = E.tiny(*c)
        assert img.shape == (c[1], c[0], c[2]) and filt == c[3] and filt in (0, 4)


def test_token_corners_cover_the_header_grammar():
    headers = [E.block_header(E.top_line(*E.token_corners(n))) for n in E.TOKEN_FRAMES]
    got = E.token_coverage([h.tokens for h in headers])
    assert got == sorted(
        ["symbol %d" % s for s in range(19)] + ["(18, 0)", "(18, 127)", "(17, 0)", "(17, 7)", "(16, 0)", "(16, 3)"]
        + ["zero run 1", "zero run 2", "zero run 10", "zero run 11", "zero run 138", "zero run 139", "zero run 140", "zero run 149"]
        + ["zero run 139 as (18, 127) 0", "zero run 140 as (18, 127) 0 0", "zero run 149 as (18, 127) (18, 0)"]
        + ["non-zero run 7", "non-zero run 8", "non-zero run 9", "non-zero run 10"])
    assert got == E.TOKEN_CORNERS
    depth = {n: h.cl_depth for n, h in zip(E.TOKEN_FRAMES, headers)}
    assert depth["deep_cl"] > R.CL_MAXBITS, depth  # the code-length code meets its own limit
    assert max(headers[E.TOKEN_FRAMES.index("deep_cl")].cllens) == R.CL_MAXBITS
    for n in E.TOKEN_FRAMES:  # every frame's scanlines take the compressed form: the header is emitted
        img, filt = E.token_corners(n)
        assert filt == 1 and all(f == "a" for _, f in _forms(img, filt)), n
    # the tokens spell the lengths back
    for h in headers:
        seq = []
        for s, _, ev in h.tokens:
            seq += [0] * (ev + 11) if s == 18 else [0] * (ev + 3) if s == 17 else [seq[-1]] * (ev + 3) if s == 16 else [s]
        assert seq == h.lens + [0]


def test_filter_ties_go_to_the_lower_type():
    for name, want in E.FILTER_TIES:
        img, filt = E.filter_ties(name)
        assert img.shape == (4, 97, 3) and filt == 0
        flat = img.reshape(4, -1)
        assert [int(l[0]) for l in R.filtered_rows(img, filt)] == [1] + [want] * 3
        for s in range(1, 4):
            cur, up = flat[3 - s], flat[4 - s]
            assert not np.array_equal(cur, up) or name == "up_paeth"
            c = {t: R.cost(R.residuals(cur, up, 3, t)) for t in R.FILTER_TYPES}
            if name == "up_paeth":
                assert c[2] == c[4] == 0 < min(c[0], c[1])
            else:
                assert c[1] == c[4] < min(c[0], c[2])


# ---------------------------------------------------------------- the expectation is a valid PNG
@pytest.mark.parametrize("cid", [c for c, _ in CASES])
def test_restatement_of_every_case_decodes(cid, tmp_path):
    img, filt, prefix = E.expected(cid)
    H, W, ch = img.shape
    assert len(prefix) <= R.bound(W, H, ch)
    data = R.png_file(W, H, ch, [prefix])
    assert data == imageio.png_from_fragments(W, H, ch, [prefix])
    body = chunks(data[8:])
    assert [c[0] for c in body] == [b"IHDR"] + [b"IDAT"] * (H + 2) + [b"IEND"]
    raw = zlib.decompress(b"".join(c[1] for c in body if c[0] == b"IDAT"))  # (verifies the Adler-32 of the header's two halves)
    assert raw == b"".join(l.tobytes() for l in R.filtered_rows(img, filt))
    path = tmp_path / "case.png"
    path.write_bytes(data)
    assert np.array_equal(imageio.read_png(str(path)), img)


def test_one_row_tiles_stitch(tmp_path):
    """the row-tiled case of the GPU tests: 97 x 3 x 3 as three tiles of one row, every scanline a first scanline"""
    img = R.noisy_frame(97, 3, 3, seed=97)
    results = [R.result_prefix(img[r:r + 1], 0) for r in (2, 1, 0)]
    assert all(int(R.filtered_rows(img[r:r + 1], 0)[0][0]) in (0, 1) for r in range(3))
    path = tmp_path / "tiles.png"
    path.write_bytes(R.png_file(97, 3, 3, results))
    assert np.array_equal(imageio.read_png(str(path)), img)


# ---------------------------------------------------------------- the restatement's two shortcuts
def test_filtered_rows_is_choose_filter_per_scanline():
    frames = [R.noisy_frame(97, 9, 3), R.noisy_frame(33, 5, 4), E.filter_ties("up_paeth")[0], E.filter_ties("sub_paeth")[0], E.tiny(1, 5, 3, 0)[0],
              np.zeros((4, 8, 3), np.uint8), E.many_rows()[0][:200]]
    for img in frames:
        rows, W, ch = img.shape
        flat = img.reshape(rows, W * ch)
        for filt in range(5):
            got = R.filtered_rows(img, filt)
            for s in range(rows):
                cur, up = flat[rows - 1 - s], (flat[rows - s] if s else None)
                t = R.choose_filter(cur, up, ch, filt)
                assert got[s][0] == t and np.array_equal(got[s][1:], R.residuals(cur, up, ch, t)), (img.shape, filt, s)


def test_min_compressed_bytes_is_a_lower_bound():
    rng = np.random.default_rng(12)
    skipped = 0
    for n in list(range(1, 40)) + [100, 300]:
        for trial in range(6):
            line = rng.integers(0, 256, n, dtype=np.uint8) if trial < 3 else np.full(n, rng.integers(0, 256), np.uint8)  # spread out; one symbol
            assert len(R.compressed_payload(line)) >= R.min_compressed_bytes(n), (n, trial)
            skipped += len(R.stored_payload(line)) < R.min_compressed_bytes(n)
    assert skipped and R.min_compressed_bytes(4) > 4 + 5  # many_rows' lines: form (b) without building form (a)
