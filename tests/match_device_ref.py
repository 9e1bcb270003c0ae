"""NumPy restatement of the match form (include/rfx.h "Match form", K8's scanline kernels with MATCHES over csrc/k8_coder.h): the token rule, form (c) of
a PNG payload and of an EXR chunk's data, the form choice, and the two result buffers with match_form_chunks.  The code-length rule, the
canonical codes, the header tokens and the bit packing are png_device_ref's, and the forms without matches are png_device_ref's and
exr_device_ref's, all by import.  Shared by the match tests; the device's result buffer must equal result_prefix_png / result_prefix_exr byte
for byte.  The token rule is stated here as the header states it — intervals cut into pieces — and not the way the kernel evaluates it."""
import struct
import zlib

import numpy as np

import exr_device_ref as X
import png_device_ref as R

PIECE = 258
NSYM = 286
# RFC 1951, 3.2.5: the length symbols 257..285, the first length of each and the count of its extra bits
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)


def length_symbol(length):
    """a match length 3..258 -> (symbol, extra bits, extra value)"""
    assert 3 <= length <= PIECE
    k = max(i for i, b in enumerate(LENGTH_BASE) if b <= length)
    return 257 + k, LENGTH_EXTRA[k], length - LENGTH_BASE[k]


def tokens_at(d):
    """the byte sequence -> (the position where each token ends, the tokens in stream order: 0..255 a literal, 256 + length a match of distance
    1), both int64"""
    d = np.asarray(d, np.uint8)
    n = d.size
    rep = np.zeros(n + 2, np.int8)  # (rep[1 + j]: position j is repeating; position 0 never is)
    rep[2:n + 1] = d[1:] == d[:-1]
    edges = np.diff(rep)
    tok, keep = d.astype(np.int64), np.ones(n, bool)
    for s, e in zip(np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)):  # the maximal intervals [s, e) of repeating positions
        for p in range(s, e, PIECE):
            q = min(p + PIECE, e)
            if q - p >= 3:  # one match stands for the piece (kept where the piece ends: the order among the literals is the same)
                keep[p:q - 1] = False
                tok[q - 1] = 256 + (q - p)
    return np.flatnonzero(keep), tok[keep]


def tokens(d):
    return tokens_at(d)[1]


def coded(d):
    """form (c)'s tokens and code for the sequence d -> (end positions, tokens, their symbols, extra bit counts, extra values, the 286 code
    lengths), or None when d holds no match"""
    pos, tok = tokens_at(d)
    if not (tok >= 256).any():
        return None
    sym, eb, ev = tok.copy(), np.zeros(tok.size, np.int64), np.zeros(tok.size, np.int64)
    for ln in np.unique(tok[tok >= 256]):
        sym[tok == ln], eb[tok == ln], ev[tok == ln] = length_symbol(int(ln) - 256)
    freq = np.bincount(sym, minlength=NSYM).astype(np.int64)
    freq[256] = 1
    return pos, tok, sym, eb, ev, R.code_lengths(freq, R.MAXBITS)


def expand(tok):
    """tokens -> the byte sequence (what a decoder does with distance 1)"""
    out = []
    for t in tok:
        out += [int(t)] if t < 256 else [out[-1]] * (int(t) - 256)
    return np.array(out, np.uint8)


def block_bits(d, first):
    """form (c)'s dynamic block for the sequence d behind the three header bits `first` -> ([values], [bit counts]) up to and including the
    end-of-block symbol, or None when d holds no match"""
    c = coded(d)
    if c is None:
        return None
    _, tok, sym, eb, ev, lens = c
    codes = R.canonical_codes(lens, R.MAXBITS)
    nlit = max(257, max(s for s in range(NSYM) if lens[s]) + 1)
    htok = R.length_tokens(lens[:nlit] + [1])  # the declared literal / length codes, then the one distance code of length 1
    clfreq = [0] * 19
    for t in htok:
        clfreq[t[0]] += 1
    cllens = R.code_lengths(clfreq, R.CL_MAXBITS)
    clcodes = R.canonical_codes(cllens, R.CL_MAXBITS)
    hclen = max(4, max(i + 1 for i, s in enumerate(R.CL_ORDER) if cllens[s]))
    v, n = [first, nlit - 257, 0, hclen - 4], [3, 5, 5, 4]
    for s in R.CL_ORDER[:hclen]:
        v.append(cllens[s])
        n.append(3)
    for s, b, x in htok:
        v.append(clcodes[s])
        n.append(cllens[s])
        if b:
            v.append(x)
            n.append(b)
    la, ca = np.asarray(lens, np.int64), np.asarray(codes, np.int64)
    match = tok >= 256
    # per token: its symbol's code, then (a match) the extra bits and the distance code `0` of one bit
    tv = np.stack([ca[sym], ev, np.zeros(tok.size, np.int64)], 1).reshape(-1)
    tn = np.stack([la[sym], eb, match.astype(np.int64)], 1).reshape(-1)
    v = np.concatenate([np.asarray(v, np.int64), tv[tn > 0], [codes[256]]])
    n = np.concatenate([np.asarray(n, np.int64), tn[tn > 0], [lens[256]]])
    return v, n


def png_payload_c(line):
    """form (c) of a PNG payload: the non-final block, the empty non-final stored block after padding to a byte; None without a match"""
    b = block_bits(line, 4)  # BFINAL 0 + BTYPE 2
    if b is None:
        return None
    body, _ = R.pack_bits(np.concatenate([b[0], [0]]), np.concatenate([b[1], [3]]))
    return body + b"\x00\x00\xff\xff"


def exr_data_c(d):
    """form (c) of an EXR chunk's data: 78 01, the FINAL block padded to a byte, the Adler-32 of d; None without a match"""
    b = block_bits(d, 5)  # BFINAL 1 + BTYPE 2
    if b is None:
        return None
    body, _ = R.pack_bits(*b)
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(np.asarray(d, np.uint8).tobytes()) & 0xFFFFFFFF)


def png_payload(line, matches=True):
    """-> (payload, in form (c)): (c) only with a match and strictly smaller than the smaller of (a) and (b)"""
    today = R.payload(line)
    c = png_payload_c(line) if matches else None
    return (c, True) if c is not None and len(c) < len(today) else (today, False)


def exr_data(raw, matches=True):
    """-> (data, in form (c)): (c) only with a match and strictly smaller than (a)-else-raw"""
    today = X.data(raw)
    c = exr_data_c(X.predict(raw)) if matches else None
    return (c, True) if c is not None and len(c) < len(today) else (today, False)


def png_chunks(tile, filt=0, matches=True):
    """tile: (rows, W, channels) uint8, row 0 = bottom -> [(payload, in form (c))], top scanline first"""
    return [png_payload(l, matches) for l in R.filtered_rows(np.asarray(tile, np.uint8), filt)]


def result_prefix_png(tile, filt=0, matches=True):
    """the PNG result buffer up to the fragment's end, with match_form_chunks in the first four of the header's last eight bytes"""
    lines = R.filtered_rows(np.asarray(tile, np.uint8), filt)
    parts = [png_payload(l, matches) for l in lines]
    frag = b"".join(R.chunk(b"IDAT", p) for p, _ in parts)
    raw = b"".join(l.tobytes() for l in lines)
    ad = zlib.adler32(raw) & 0xFFFFFFFF
    return struct.pack("<QIIQII", len(frag), ad & 0xFFFF, ad >> 16, len(raw), sum(c for _, c in parts), 0) + frag


def exr_chunks(tile, matches=True):
    """tile: (rows, W, channels) halfs, row 0 = bottom -> [(data, in form (c))], top scanline first"""
    return [exr_data(raw, matches) for raw in X.raw_blocks(tile)]


def result_prefix_exr(tile, first_y=0, matches=True):
    """the EXR result buffer up to the fragment's end, with match_form_chunks in the header's last four bytes"""
    rows, W, ch = np.asarray(tile).shape
    parts = exr_chunks(tile, matches)
    frag = b"".join(struct.pack("<ii", first_y + s, len(d)) + d for s, (d, _) in enumerate(parts))
    n = 2 * W * ch
    return struct.pack("<QIIQII", len(frag), rows, first_y, rows * n, sum(1 for d, c in parts if not c and len(d) == n), sum(c for _, c in parts)) + frag


def png_header_of(result):
    """(fragment_bytes, adler_a, adler_b, raw_bytes, match_form_chunks, zero)"""
    return struct.unpack("<QIIQII", bytes(result[:32]))


def png_payloads_of(result):
    """the IDAT payloads of a PNG result buffer"""
    nbytes = png_header_of(result)[0]
    body, out, at = bytes(result[32:32 + nbytes]), [], 0
    while at < nbytes:
        size = struct.unpack(">I", body[at:at + 4])[0]
        assert body[at + 4:at + 8] == b"IDAT"
        out.append(body[at + 8:at + 8 + size])
        at += 12 + size
    assert at == nbytes
    return out
