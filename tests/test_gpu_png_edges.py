"""GPU (-m gpu; also under --hostsim): K8 at the edges tests/png_edge_cases.py names — the bit window at its fullest, tiny frames and rows that
straddle one step of the sweep, stored blocks of one and of three bytes, the choice between the two forms at equality, every header token,
filter ties, the largest Adler sums, 32768 chunks, tiles of one row — each with the premises tests/test_png_edges_cpu.py asserts.  For every
case ctx.export returns the planted bytes, ctx.png equals the restatement's result byte for byte (header included), and the wrapped file
decodes to the image.  No comparison here has a tolerance."""
import struct

import numpy as np
import pytest

import png_device_ref as R
import png_edge_cases as E
from rfx_amd.context import Context
from test_gpu_png import SRC, check, decode, plant

pytestmark = pytest.mark.gpu


def chunk_lengths(result):
    """the payload length of every IDAT chunk of a result buffer's fragment"""
    n = struct.unpack("<Q", bytes(result[:8]))[0]
    frag, out, pos = bytes(result[32:32 + n]), [], 0
    while pos < len(frag):
        k, tag = struct.unpack(">I4s", frag[pos:pos + 8])
        assert tag == b"IDAT"
        out.append(k)
        pos += 12 + k
    assert pos == len(frag)
    return out


def run_case(cid, tmp_path):
    img, filt, want = E.expected(cid)
    H, W, ch = img.shape
    ctx = Context(W, H)
    ctx.upload(SRC, plant(img))
    got = check(ctx, img, filt, want)
    ctx.close()
    assert np.array_equal(decode(tmp_path, W, H, ch, [got]), img)
    return img, got


@pytest.mark.parametrize("cid", [c for c, _ in E.all_cases()])
def test_edge_case_equals_the_restatement(cid, tmp_path):
    run_case(cid, tmp_path)


@pytest.mark.parametrize("edge", E.STORED_EDGES, ids=lambda e: "%dx%d-%dblocks" % e)
def test_stored_block_edges_fragment_length(edge, tmp_path):
    W, ch, blocks = edge
    img, got = run_case("stored-%dx2x%d" % (W, ch), tmp_path)
    n = 1 + W * ch
    assert struct.unpack("<Q", got[:8].tobytes())[0] == 2 * (12 + 5 * blocks + n)
    assert chunk_lengths(got) == [n + 5 * blocks] * 2  # every chunk in form (b)


def test_tie_goes_to_the_compressed_form(tmp_path):
    """len(compressed) - len(stored) = +1, 0, -1: the device's own choice, read off the chunk lengths"""
    n = 1 + 97 * 3
    stored = n + 5
    for k, diff in zip(E.TIE_K, E.TIE_DIFF):
        img, got = run_case("tie-k%d" % k, tmp_path)
        assert chunk_lengths(got) == [min(stored + diff, stored)] * 2, k
        first = bytes(got[32 + 8:32 + 8 + 3])  # the payload's first bytes: 00 LEN of a stored block, or BFINAL 0 BTYPE 2
        assert (first == b"\x00" + struct.pack("<H", n)) == (diff > 0) and (first[0] & 7 == 4) == (diff <= 0), k


@pytest.mark.parametrize("halo", [0, 1])
def test_tiles_of_one_row(halo, tmp_path):
    """97 x 3 x 3 as three tiles of one row each: every fragment is its own row's, with no upper neighbour; the stitched file is the frame"""
    W, H, ch = 97, 3, 3
    img = R.noisy_frame(W, H, ch, seed=97)
    a = plant(img)
    results = []
    for y0 in (2, 1, 0):  # top tile first (rfx_split_rows keeps tile boundaries on even rows: the tiles are laid out here)
        t = Context(W, H, tile_y0=y0, tile_rows=1, halo_rows=halo)
        r0, rn = t.held_rows(SRC)
        t.upload(SRC, a[r0:r0 + rn])
        results.append(check(t, img[y0:y0 + 1], 0).copy())
        t.close()
        assert len(chunk_lengths(results[-1])) == 1
    assert np.array_equal(decode(tmp_path, W, H, ch, results), img)


def test_staged_png_of_the_widest_shapes():
    """the download-stream path (stage_png / export_wait) at the two stored-block edges and the fullest window; a context has one size, so
    three contexts, each staging its frame twice over both of its buffers"""
    for cid in ["stored-%dx2x%d" % (W, ch) for (W, ch, _) in E.STORED_EDGES] + ["deep_row-lead0"]:
        img, filt, want = E.expected(cid)
        H, W, ch = img.shape
        ctx = Context(W, H)
        ctx.upload(SRC, plant(img))
        outs = [ctx.host_alloc((ctx.png_bound(ch),), np.uint8) for _ in range(2)]
        for o in outs:
            o[...] = 0xEE
        tickets = [ctx.stage_png(SRC, ch, filter=filt, out=o) for o in outs]
        assert tickets[1] == tickets[0] + 1
        for t in tickets:
            ctx.export_wait(t)
        ctx.close()
        for o in outs:
            assert o.nbytes == R.bound(W, H, ch) and o[:len(want)].tobytes() == want, cid
