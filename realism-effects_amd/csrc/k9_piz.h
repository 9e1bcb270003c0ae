// K9 PIZ cores: what OpenEXR's PIZ compression stores in a block — a bitmap of the 16-bit values that occur, a canonical Huffman code of the
// wavelet-transformed, densely renumbered words with a run escape — decoded with no HIP dependency, in the manner of k9_inflate.h:
// k9_exr_import.hip instantiates the Huffman decode with the wave-wide IO (one wave per block, the state below wave-uniform) and runs the
// wavelet cells with one thread per quad; a plain x86 program (tests/test_piz_core_cpu.py builds one under the sanitizers) runs the same
// statements with K9PizHostIO.
//
// The block:   u16 min, max | the bitmap bytes min .. max (min > max: none; bit v & 7 of byte v >> 3 = value v occurs; value 0 always does) |
//              i32 hlen | the Huffman block of hlen bytes: u32 im, iM, tableLength, nBits, 0 | the code lengths of symbols im .. iM, 6 bits each,
//              MSB first (59 .. 62: 2 .. 5 symbols without a code, 63 + 8 bits: 6 .. 261 of them) | nBits bits of codes, MSB first.
// The code:    canonical, ascending within a length, LONGER codes first: start[58] = 0, start[l] = (start[l + 1] + count[l + 1]) >> 1.  Symbol iM is
//              the run escape: 8 bits follow, that many more copies of the previous word.  The words come channel-planar.
// The decode:  a primary table on the first K9_PIZ_FAST_BITS bits ((symbol << 6) | length, 0: none); a longer code by the walk over the lengths:
//              the first l bits are a code iff start[l] <= them < start[l] + count[l], and its symbol is symbol[offset[l] + them - start[l]] — the
//              list of the symbols with a code sorted by (length, symbol), 16 bits each: iM, the largest symbol, ends its length's group, so the
//              escape is known by its index and the list never has to hold 65536.
// The safety rules, which hold for ANY input bytes:
//   reads    every field is bounded by the block's size before it is read; the IO hands out zeros beyond the packed bytes, and no code or run
//            count may end behind min(nBits, the bits hlen holds) (K9_E_PIZ_TRUNCATED), so a zero that was not in the input is never consumed;
//   writes   a word goes to out[n] with n < nwords (K9_E_PIZ_WORDS, K9_E_PIZ_RUN); the symbol list and the primary table are written inside
//            their sizes: a code-length set must be complete, or hold at most one symbol (K9_E_PIZ_LENGTHS: what a writer's Huffman tree gives,
//            and what makes `start` a prefix code);
//   loops    every iteration of the two walks over the length table consumes at least 6 of its bits, every iteration of the decode at least
//            one bit, a step of the walk over the lengths one bit of the code it ends with (K9_ITER marks them).
// The IO concept is k9_inflate.h's `word` and `sync`, and
//   bool leader()                             one lane of the wave (the table counters in K9PizHuf are bumped by it alone)
//   uint32_t bcast(uint32_t v)                the leader's v
//   K9PizHuf &huf()                           the decode tables (LDS on the device)
//   void fast_fill(unsigned lo, unsigned n, uint32_t e)      huf().fast[lo + k] = e, k < n
//   void sym_put(unsigned i, unsigned v) / unsigned sym(unsigned i)   the sorted symbol list (device memory: the block's table scratch)
//   void put16(size_t n, unsigned v)          out[n] = v; words come in ascending n
//   void fill16(size_t n, unsigned v, unsigned len)          out[n + k] = v, k < len
//   void flush(size_t n)                      out[0, n) is stored
#pragma once
#include "k9_inflate.h"

enum {
    K9_E_PIZ_BITMAP = 15,     // the bitmap's range: min or max >= 8192
    K9_E_PIZ_HEADER = 16,     // the bitmap, hlen, the 20-byte header or the length table reach outside the block
    K9_E_PIZ_RANGE = 17,      // im or iM >= 65537
    K9_E_PIZ_TABLE = 18,      // the length table ends inside an entry, or a zero run passes iM
    K9_E_PIZ_LENGTHS = 19,    // over-subscribed, or incomplete with more than one symbol
    K9_E_PIZ_CODE = 20,       // a bit pattern that is no code
    K9_E_PIZ_RUN = 21,        // a run with nothing to repeat, or past nwords
    K9_E_PIZ_WORDS = 22,      // fewer or more words than the block holds
    K9_E_PIZ_TRUNCATED = 23   // the input ends inside a code or a run count
};

constexpr int K9_PIZ_FAST_BITS = 12, K9_PIZ_MAX_LEN = 58;
constexpr unsigned K9_PIZ_ENCSIZE = 65537u;  // 65536 word values + the run escape
constexpr int K9_PIZ_CELL = 64;              // the wavelet cell's side (see k9_piz_cell_level)
// 17.4 KiB: one wave's decode state in LDS
struct K9PizHuf {
    uint32_t fast[1 << K9_PIZ_FAST_BITS];
    uint64_t start[K9_PIZ_MAX_LEN + 1];
    uint32_t count[K9_PIZ_MAX_LEN + 1], offset[K9_PIZ_MAX_LEN + 1], next[K9_PIZ_MAX_LEN + 1];
};
// A block's table scratch in device memory: the reverse lookup table, the sorted symbols, the info words (mx).
constexpr size_t K9_PIZ_REV_BYTES = 65536 * 2, K9_PIZ_SYM_BYTES = (2 * (size_t)K9_PIZ_ENCSIZE + 255) & ~(size_t)255, K9_PIZ_INFO_BYTES = 256;
constexpr size_t K9_PIZ_TABLE_BYTES = K9_PIZ_REV_BYTES + K9_PIZ_SYM_BYTES + K9_PIZ_INFO_BYTES;

template <class IO>
K9_FN unsigned k9_piz_byte(IO &io, size_t i) { return (unsigned)(io.word(i >> 2) >> (8 * (unsigned)(i & 3))) & 255u; }
template <class IO>
K9_FN uint32_t k9_piz_u32(IO &io, size_t i) {
    return (uint32_t)k9_piz_byte(io, i) | (uint32_t)k9_piz_byte(io, i + 1) << 8 | (uint32_t)k9_piz_byte(io, i + 2) << 16 | (uint32_t)k9_piz_byte(io, i + 3) << 24;
}
K9_FN uint32_t k9_piz_swap(uint32_t w) { return (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24); }
// the 64 bits of the input from bit `bit` on (bit 0 = the MSB of byte 0), the first one in bit 63
template <class IO>
K9_FN uint64_t k9_piz_peek(IO &io, size_t bit) {
    const size_t w = bit >> 5;
    const unsigned s = (unsigned)(bit & 31);
    const uint64_t hi = (uint64_t)k9_piz_swap(io.word(w)) << 32 | (uint64_t)k9_piz_swap(io.word(w + 1));
    return s ? (hi << s) | (uint64_t)(k9_piz_swap(io.word(w + 2)) >> (32u - s)) : hi;
}

struct K9PizHead {
    unsigned bm_min, bm_max;  // the bitmap bytes present (bm_min > bm_max: none), at byte 4 of the block
    size_t huf_at, huf_len;   // the Huffman block
};
template <class IO>
K9_FN int k9_piz_head(IO &io, size_t in_len, K9PizHead *h) {
    if (in_len < 8) return K9_E_PIZ_HEADER;
    h->bm_min = k9_piz_byte(io, 0) | k9_piz_byte(io, 1) << 8;
    h->bm_max = k9_piz_byte(io, 2) | k9_piz_byte(io, 3) << 8;
    size_t pos = 4;
    if (h->bm_min <= h->bm_max) {
        if (h->bm_max >= 8192u) return K9_E_PIZ_BITMAP;
        pos += h->bm_max - h->bm_min + 1u;
    } else if (h->bm_min >= 8192u)
        return K9_E_PIZ_BITMAP;
    if (pos + 4 > in_len) return K9_E_PIZ_HEADER;
    const uint32_t hlen = k9_piz_u32(io, pos);
    pos += 4;
    if (hlen >= 0x80000000u || (size_t)hlen > in_len - pos) return K9_E_PIZ_HEADER;
    h->huf_at = pos;
    h->huf_len = hlen;
    return K9_OK;
}

// ---- the reverse lookup table: rev[k] = the k-th value whose bit is set (bit 0 forced on), zero behind them.  64 lanes, 1024 values each: a lane
// counts its bits, the counts of the lanes before it are where it writes.  bm: the bitmap bytes of the block (in + 4).
K9_FN uint32_t k9_piz_bitmap_word(const uint8_t *bm, unsigned bm_min, unsigned bm_max, unsigned j) {
    uint32_t w = j ? 0u : 1u;
    for (unsigned b = 0; b < 4; b++) {
        const unsigned at = 4u * j + b;
        if (at >= bm_min && at <= bm_max) w |= (uint32_t)bm[at - bm_min] << (8 * b);
    }
    return w;
}
K9_FN unsigned k9_piz_popcount(uint32_t w) {
    w = w - ((w >> 1) & 0x55555555u);
    w = (w & 0x33333333u) + ((w >> 2) & 0x33333333u);
    return (((w + (w >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24;
}
K9_FN unsigned k9_piz_rev_count(const uint8_t *bm, unsigned bm_min, unsigned bm_max, int lane) {
    unsigned n = 0;
    for (unsigned j = 0; j < 32; j++) n += k9_piz_popcount(k9_piz_bitmap_word(bm, bm_min, bm_max, 32u * (unsigned)lane + j));
    return n;
}
// base: the bits of the lanes before this one; total: of all lanes (mx = total - 1)
K9_FN void k9_piz_rev_write(const uint8_t *bm, unsigned bm_min, unsigned bm_max, int lane, unsigned base, unsigned total, uint16_t *rev) {
    for (unsigned j = 0; j < 32; j++) {
        const unsigned word = 32u * (unsigned)lane + j;
        const uint32_t w = k9_piz_bitmap_word(bm, bm_min, bm_max, word);
        for (unsigned b = 0; b < 32; b++)
            if (w >> b & 1u) rev[base++] = (uint16_t)(32u * word + b);  // (base < total <= 65536)
    }
    for (unsigned k = total + (unsigned)lane; k < 65536u; k += 64u) rev[k] = 0;
}

// ---- the Huffman block at bytes [at, at + len) of the input -> exactly nwords words.  K9_OK or the first error; what out[] holds after an error
// is unspecified (but inside nwords).
template <class IO>
K9_FN int k9_piz_huf_decode(IO &io, size_t at, size_t len, size_t nwords) {
    if (len < 20) return K9_E_PIZ_HEADER;
    const uint32_t im = k9_piz_u32(io, at), iM = k9_piz_u32(io, at + 4), tlen = k9_piz_u32(io, at + 8), nbits = k9_piz_u32(io, at + 12);
    if (im >= K9_PIZ_ENCSIZE || iM >= K9_PIZ_ENCSIZE) return K9_E_PIZ_RANGE;
    if ((size_t)tlen > len - 20) return K9_E_PIZ_HEADER;
    K9PizHuf &t = io.huf();
    const size_t tbit0 = 8 * (at + 20), tbits = 8 * (size_t)tlen;
    // the length table, first walk: how many symbols of every length
    io.sync();
    if (io.leader())
        for (int l = 0; l <= K9_PIZ_MAX_LEN; l++) t.count[l] = t.next[l] = 0u;
    io.fast_fill(0u, 1u << K9_PIZ_FAST_BITS, 0u);
    unsigned rl_len = 0;
    size_t tp = 0;
    for (uint32_t i = im; i <= iM;) {
        K9_ITER();
        if (tp + 6 > tbits) return K9_E_PIZ_TABLE;
        const unsigned ln = (unsigned)(k9_piz_peek(io, tbit0 + tp) >> 58);
        tp += 6;
        if (ln <= (unsigned)K9_PIZ_MAX_LEN) {
            if (ln && io.leader()) t.count[ln]++;
            if (i == iM) rl_len = ln;
            i++;
            continue;
        }
        uint32_t run = ln - 59u + 2u;
        if (ln == 63u) {
            if (tp + 8 > tbits) return K9_E_PIZ_TABLE;
            run = (uint32_t)(k9_piz_peek(io, tbit0 + tp) >> 56) + 6u;
            tp += 8;
        }
        if (run > iM + 1u - i) return K9_E_PIZ_TABLE;
        i += run;
    }
    io.sync();
    // the canonical code: where every length's codes start, and its group in the sorted list
    uint64_t c = 0;
    int64_t left = 1;
    uint32_t nsym = 0;
    int maxlen = 0;
    for (int l = 1; l <= K9_PIZ_MAX_LEN; l++) {
        const uint32_t n = t.count[l];
        left = 2 * left - (int64_t)n;  // (left <= 2^l)
        if (left < 0) return K9_E_PIZ_LENGTHS;
        if (n) maxlen = l;
        nsym += n;
    }
    if (left != 0 && nsym > 1u) return K9_E_PIZ_LENGTHS;
    if (io.leader()) {
        uint32_t off = 0;
        for (int l = 1; l <= K9_PIZ_MAX_LEN; l++) { t.offset[l] = off; off += t.count[l]; }
        for (int l = K9_PIZ_MAX_LEN; l >= 1; l--) { t.start[l] = c; c = (c + t.count[l]) >> 1; }
    }
    io.sync();
    const uint32_t rl_idx = rl_len ? t.offset[rl_len] + t.count[rl_len] - 1u : ~0u;
    // second walk: the symbols into the sorted list (ascending here, so ascending within a length), the short codes into the primary table
    tp = 0;
    for (uint32_t i = im; i <= iM;) {
        K9_ITER();
        const unsigned ln = (unsigned)(k9_piz_peek(io, tbit0 + tp) >> 58);
        tp += 6;
        if (ln <= (unsigned)K9_PIZ_MAX_LEN) {
            if (ln) {
                uint32_t rank = 0;
                if (io.leader()) { rank = t.next[ln]; t.next[ln] = rank + 1u; }
                rank = io.bcast(rank);  // (< count[ln])
                const uint64_t code = t.start[ln] + rank;
                if (code >> ln) return K9_E_PIZ_LENGTHS;  // (never for a complete set)
                if (ln <= (unsigned)K9_PIZ_FAST_BITS) io.fast_fill((unsigned)code << (K9_PIZ_FAST_BITS - ln), 1u << (K9_PIZ_FAST_BITS - ln), (i << 6) | ln);
                io.sym_put(t.offset[ln] + rank, i & 0xffffu);
            }
            i++;
            continue;
        }
        uint32_t run = ln - 59u + 2u;
        if (ln == 63u) {
            run = (uint32_t)(k9_piz_peek(io, tbit0 + tp) >> 56) + 6u;
            tp += 8;
        }
        i += run;
    }
    io.sync();
    // the codes
    const size_t dbit0 = tbit0 + tbits, held = 8 * (len - 20 - (size_t)tlen), limit = (size_t)nbits < held ? (size_t)nbits : held;
    size_t bp = 0, n = 0;
    uint32_t prev = 0;
    while (bp < (size_t)nbits) {
        K9_ITER();
        const uint64_t v = k9_piz_peek(io, dbit0 + bp);
        const uint32_t e = t.fast[v >> (64 - K9_PIZ_FAST_BITS)];
        unsigned ln = e & 63u;
        uint32_t sym = e >> 6;
        bool run = e && sym == iM;
        if (!e) {
            for (ln = K9_PIZ_FAST_BITS + 1;; ln++) {
                if ((int)ln > maxlen) return bp + (size_t)maxlen > limit ? K9_E_PIZ_TRUNCATED : K9_E_PIZ_CODE;  // (the bits left could not hold the longest code)
                K9_ITER();
                const uint64_t code = v >> (64u - ln);
                const uint32_t cnt = t.count[ln];
                if (cnt && code >= t.start[ln] && code - t.start[ln] < cnt) {
                    const uint32_t idx = t.offset[ln] + (uint32_t)(code - t.start[ln]);
                    run = idx == rl_idx;
                    sym = run ? iM : io.sym(idx);
                    break;
                }
            }
        }
        if (bp + ln > limit) return K9_E_PIZ_TRUNCATED;
        bp += ln;
        if (run) {
            if (bp + 8 > limit) return K9_E_PIZ_TRUNCATED;
            const unsigned cs = (unsigned)(k9_piz_peek(io, dbit0 + bp) >> 56);
            bp += 8;
            if (n == 0 || (size_t)cs > nwords - n) return K9_E_PIZ_RUN;
            io.fill16(n, prev, cs);
            n += cs;
        } else {
            if (n >= nwords) return K9_E_PIZ_WORDS;
            io.put16(n, sym);
            prev = sym;
            n++;
        }
    }
    io.flush(n);
    if (n != nwords) return K9_E_PIZ_WORDS;
    return K9_OK;
}

// ---- the wavelet, decoded cell by cell.  For a plane of nx x ny words, Q = the largest power of two <= min(nx, ny): the levels are p = Q / 2 .. 1,
// and everything level p does — the 2 x 2 steps on (x, x + p) x (y, y + p) at the multiples of 2 p, the 1-D steps of an odd column or row — stays
// inside a square of side 2 p <= Q aligned at the plane's origin.  So a cell of K9_PIZ_CELL x K9_PIZ_CELL words (a multiple of Q: the plans refuse
// Q > K9_PIZ_CELL) aligned there, clipped at the plane's edges, decodes through all levels on its own; within a level the steps touch disjoint words.
K9_FN int k9_piz_top_level(int nx, int ny) {  // Q / 2; 0: no level
    const int n = nx < ny ? nx : ny;
    int p = 1;
    while (2 * p <= n) p *= 2;
    return p / 2;
}
K9_FN void k9_piz_wdec14(uint16_t l, uint16_t h, uint16_t *a, uint16_t *b) {
    const int ls = (int16_t)l, hs = (int16_t)h, ai = ls + (hs & 1) + (hs >> 1);
    *a = (uint16_t)ai;
    *b = (uint16_t)(ai - hs);
}
K9_FN void k9_piz_wdec16(uint16_t l, uint16_t h, uint16_t *a, uint16_t *b) {
    const int bb = ((int)l - ((int)h >> 1)) & 65535;
    *a = (uint16_t)(((int)h + bb - 32768) & 65535);
    *b = (uint16_t)bb;
}
K9_FN void k9_piz_wdec(bool w14, uint16_t l, uint16_t h, uint16_t *a, uint16_t *b) {
    if (w14) k9_piz_wdec14(l, h, a, b);
    else k9_piz_wdec16(l, h, a, b);
}
// level p of the cell whose word (0, 0) is the plane's (x0, y0): cell[ly * K9_PIZ_CELL + lx]; thread t of nt takes every nt-th square
K9_FN void k9_piz_cell_level(uint16_t *cell, int x0, int y0, int nx, int ny, int p, bool w14, int t, int nt) {
    const int p2 = 2 * p, per = K9_PIZ_CELL / p2;
    for (int q = t; q < per * per; q += nt) {
        const int ly = (q / per) * p2, lx = (q % per) * p2, gx = x0 + lx, gy = y0 + ly;
        if (gx >= nx || gy >= ny) continue;
        const bool fx = gx + p2 <= nx, fy = gy + p2 <= ny;
        uint16_t *w = cell + ly * K9_PIZ_CELL + lx;
        if (fx && fy) {
            uint16_t a, b, c, d;
            k9_piz_wdec(w14, w[0], w[p * K9_PIZ_CELL], &a, &c);
            k9_piz_wdec(w14, w[p], w[p * K9_PIZ_CELL + p], &b, &d);
            k9_piz_wdec(w14, a, b, &w[0], &w[p]);
            k9_piz_wdec(w14, c, d, &w[p * K9_PIZ_CELL], &w[p * K9_PIZ_CELL + p]);
        } else if (fy && (nx & p)) {  // the odd column: 1-D in y
            uint16_t a, b;
            k9_piz_wdec(w14, w[0], w[p * K9_PIZ_CELL], &a, &b);
            w[0] = a; w[p * K9_PIZ_CELL] = b;
        } else if (fx && (ny & p)) {  // the odd row: 1-D in x
            uint16_t a, b;
            k9_piz_wdec(w14, w[0], w[p], &a, &b);
            w[0] = a; w[p] = b;
        }
    }
}

#ifndef K9_NO_HOST_IO
struct K9PizHostIO {
    const uint8_t *in;
    size_t in_len;
    uint16_t *out, *symbols;  // nwords words; K9_PIZ_ENCSIZE entries
    K9PizHuf t;
    uint32_t word(size_t i) const {
        uint32_t w = 0;
        for (int k = 0; k < 4; k++)
            if (4 * i + (size_t)k < in_len) w |= (uint32_t)in[4 * i + (size_t)k] << (8 * k);
        return w;
    }
    bool leader() const { return true; }
    uint32_t bcast(uint32_t v) const { return v; }
    K9PizHuf &huf() { return t; }
    void fast_fill(unsigned lo, unsigned n, uint32_t e) {
        for (unsigned k = 0; k < n; k++) t.fast[lo + k] = e;
    }
    void sym_put(unsigned i, unsigned v) { symbols[i] = (uint16_t)v; }
    unsigned sym(unsigned i) const { return symbols[i]; }
    void put16(size_t n, unsigned v) { out[n] = (uint16_t)v; }
    void fill16(size_t n, unsigned v, unsigned len) {
        for (unsigned k = 0; k < len; k++) out[n + k] = (uint16_t)v;
    }
    void flush(size_t) {}
    void sync() {}
};
// one plane of nx x ny words (x stride xs, y stride ys words) through every cell, as the device walks them
K9_FN void k9_piz_plane_host(uint16_t *plane, int nx, int ny, int xs, int ys, bool w14) {
    uint16_t cell[K9_PIZ_CELL * K9_PIZ_CELL] = {0};
    for (int y0 = 0; y0 < ny; y0 += K9_PIZ_CELL)
        for (int x0 = 0; x0 < nx; x0 += K9_PIZ_CELL) {
            for (int ly = 0; ly < K9_PIZ_CELL && y0 + ly < ny; ly++)
                for (int lx = 0; lx < K9_PIZ_CELL && x0 + lx < nx; lx++) cell[ly * K9_PIZ_CELL + lx] = plane[(size_t)(y0 + ly) * ys + (size_t)(x0 + lx) * xs];
            for (int p = k9_piz_top_level(nx, ny); p >= 1; p >>= 1)
                for (int t = 0; t < 64; t++) k9_piz_cell_level(cell, x0, y0, nx, ny, p, w14, t, 64);
            for (int ly = 0; ly < K9_PIZ_CELL && y0 + ly < ny; ly++)
                for (int lx = 0; lx < K9_PIZ_CELL && x0 + lx < nx; lx++) plane[(size_t)(y0 + ly) * ys + (size_t)(x0 + lx) * xs] = cell[ly * K9_PIZ_CELL + lx];
        }
}
#endif
