// K9 decoder core: a complete RFC 1950 / RFC 1951 decoder (zlib header, stored / fixed-Huffman / dynamic-Huffman blocks in any mix, the
// Adler-32 trailer) with no HIP dependency.  k9_exr_import.hip instantiates it with a wave-wide IO (one wave per chunk, the state below held
// wave-uniform, the stores spread over the lanes); a plain x86 program instantiates it with K9HostIO (tests/test_inflate_core_cpu.py builds one
// under the sanitizers).  Both run the same statements.
//
// The safety rules, which hold for ANY input bytes:
//   reads    the IO hands out the input as little-endian 32-bit words, zero beyond the packed size; the bit counter `used` may never pass
//            8 * in_len (K9_E_TRUNCATED), so a zero that was not in the input is never consumed;
//   writes   every byte goes to out[pos] with pos < out_len, the chunk's raw size known from the file header (K9_E_OVERRUN);
//   matches  a distance beyond the bytes produced so far is K9_E_DISTANCE;
//   loops    every iteration of a loop whose trip count depends on the input consumes at least one bit or produces at least one byte (K9_ITER
//            marks them: a test build counts); the others — a repeat of at most 138 code lengths, the table builds over at most 288 symbols and
//            1024 fast entries — are bounded by a constant;
//   codes    a code-length set is checked as zlib checks it: over-subscribed -> error; incomplete -> error, except a distance set with at most
//            one code of length 1; no end-of-block code -> error.
// The IO concept:
//   uint32_t word(size_t i)                         bytes [4 i, 4 i + 4) of the input, little-endian, zero beyond in_len
//   void put(size_t pos, unsigned byte)             out[pos] = byte
//   void copy(size_t pos, unsigned dist, unsigned len)   out[pos + k] = out[pos - dist + k], k ascending (dist < len repeats the pattern)
//   void copy_in(size_t pos, size_t src, unsigned len)   out[pos + k] = in[src + k]
//   uint32_t adler(size_t n)                        Adler-32 of out[0, n)
//   K9Tables &tables()                              the decode tables (LDS on the device)
//   void sync()                                     before the tables change role: no lane may still be reading what is overwritten
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef K9_FN
#define K9_FN static inline
#endif
#ifndef K9_ITER
#define K9_ITER() ((void)0)
#endif

enum {
    K9_OK = 0,
    K9_E_HEADER = 1,        // not a zlib header: CM != 8, window > 32 KiB, FCHECK, a preset dictionary
    K9_E_TRUNCATED = 2,     // the input ends inside the stream
    K9_E_BLOCK_TYPE = 3,    // block type 3
    K9_E_STORED_LEN = 4,    // LEN != ~NLEN
    K9_E_CODE_LENGTHS = 5,  // a bad code-length set (too many codes, a repeat with nothing to repeat or past the end, over-subscribed, incomplete, no end-of-block code)
    K9_E_SYMBOL = 6,        // a bit pattern that is no code of the set, or a length / distance symbol beyond 285 / 29
    K9_E_DISTANCE = 7,      // a match that starts before the first byte produced
    K9_E_OVERRUN = 8,       // more than out_len bytes
    K9_E_SHORT = 9,         // the stream ends with fewer than out_len bytes
    K9_E_ADLER = 10,        // the trailer does not match the bytes produced
    K9_E_TRAILING = 11      // bytes behind the trailer (a chunk's packed size is exact)
};

constexpr int K9_FAST_LIT_BITS = 10, K9_FAST_DIST_BITS = 8;
// 3.5 KiB: one wave's decode state in LDS.  A fast entry is (symbol << 4) | code length for a code of at most FAST bits, at every index whose
// low bits are the code (bit-reversed, as the stream delivers it); 0: a longer code or none, resolved by the canonical walk over count / symbol.
struct K9Tables {
    uint16_t lit_fast[1 << K9_FAST_LIT_BITS];
    uint16_t dist_fast[1 << K9_FAST_DIST_BITS];
    uint16_t lit_count[16], lit_symbol[288];
    uint16_t dist_count[16], dist_symbol[32];
    uint8_t lengths[352];  // the code lengths of the block header being read
};

struct K9Bits {
    uint64_t buf;      // the next `cnt` bits of the stream, least significant first
    int cnt;
    size_t next_word;  // of the input, not yet in buf
    size_t used, total;  // bits consumed; 8 * in_len
};

template <class IO>
K9_FN void k9_seek(IO &io, K9Bits &b, size_t byte) {
    b.next_word = byte >> 2;
    const int sh = 8 * (int)(byte & 3);
    b.buf = (uint64_t)(io.word(b.next_word++) >> sh);
    b.cnt = 32 - sh;
    b.used = 8 * byte;
}
// at least 33 bits in buf (zeros beyond the input: `used` guards them)
template <class IO>
K9_FN void k9_refill(IO &io, K9Bits &b) {
    if (b.cnt <= 32) {
        b.buf |= (uint64_t)io.word(b.next_word++) << b.cnt;
        b.cnt += 32;
    }
}
K9_FN bool k9_consume(K9Bits &b, int n) {
    if (b.used + (size_t)n > b.total) return false;
    b.buf >>= n;
    b.cnt -= n;
    b.used += (size_t)n;
    return true;
}
// n <= 16 bits; -1: the input ends first
template <class IO>
K9_FN int k9_bits(IO &io, K9Bits &b, int n) {
    k9_refill(io, b);
    const int v = (int)(b.buf & ((1u << n) - 1u));
    return k9_consume(b, n) ? v : -1;
}

// Canonical code of `n` symbols from lengths[0, n) (0: the symbol has no code).  Returns what is left of the code space: 0 complete,
// > 0 incomplete, < 0 over-subscribed (the tables are then not usable).
K9_FN int k9_build(const uint8_t *lengths, int n, uint16_t *count, uint16_t *symbol, uint16_t *fast, int fast_bits) {
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[lengths[s]]++;
    int left = 1;
    for (int l = 1; l < 16; l++) {
        left = 2 * left - (int)count[l];
        if (left < 0) return left;
    }
    uint16_t offs[16], code[16];
    offs[1] = 0;
    code[0] = 0; code[1] = 0;
    for (int l = 1; l < 15; l++) {
        offs[l + 1] = (uint16_t)(offs[l] + count[l]);
        code[l + 1] = (uint16_t)((code[l] + count[l]) << 1);
    }
    if (fast)
        for (int i = 0; i < (1 << fast_bits); i++) fast[i] = 0;
    for (int s = 0; s < n; s++) {
        const int l = lengths[s];
        if (!l) continue;
        symbol[offs[l]++] = (uint16_t)s;
        const unsigned c = code[l]++;
        if (fast && l <= fast_bits) {
            unsigned r = 0;
            for (int k = 0; k < l; k++) r |= ((c >> k) & 1u) << (l - 1 - k);
            for (unsigned j = r; j < (1u << fast_bits); j += 1u << l) fast[j] = (uint16_t)((s << 4) | l);
        }
    }
    return left;
}

// the next symbol, or -K9_E_*
template <class IO>
K9_FN int k9_symbol(IO &io, K9Bits &b, const uint16_t *count, const uint16_t *symbol, const uint16_t *fast, int fast_bits) {
    k9_refill(io, b);
    if (fast) {
        const unsigned e = fast[b.buf & ((1u << fast_bits) - 1u)];
        if (e) return k9_consume(b, (int)(e & 15u)) ? (int)(e >> 4) : -K9_E_TRUNCATED;
    }
    unsigned bits = (unsigned)(b.buf & 0x7fffu);
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; l++) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int n = count[l];
        if (code - n < first) return k9_consume(b, l) ? (int)symbol[index + (code - first)] : -K9_E_TRUNCATED;
        index += n;
        first = (first + n) << 1;
        code <<= 1;
    }
    return b.used + 15 > b.total ? -K9_E_TRUNCATED : -K9_E_SYMBOL;
}

template <class IO>
K9_FN int k9_read_dynamic(IO &io, K9Bits &b) {
    K9Tables &t = io.tables();
    const int hl = k9_bits(io, b, 14);
    if (hl < 0) return K9_E_TRUNCATED;
    const int nlen = (hl & 31) + 257, ndist = ((hl >> 5) & 31) + 1, ncode = ((hl >> 10) & 15) + 4;
    if (nlen > 286 || ndist > 30) return K9_E_CODE_LENGTHS;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; i++) t.lengths[i] = 0;
    for (int i = 0; i < ncode; i++) {
        const int v = k9_bits(io, b, 3);
        if (v < 0) return K9_E_TRUNCATED;
        t.lengths[order[i]] = (uint8_t)v;
    }
    // the code-length code borrows the literal set's canonical arrays (no fast table): it must be complete (zlib's rule for CODES)
    if (k9_build(t.lengths, 19, t.lit_count, t.lit_symbol, nullptr, 0) != 0) return K9_E_CODE_LENGTHS;
    // (the lengths move up by 19 entries while they are read: t.lengths[0, 19) is still the code-length code's own input)
    uint8_t *len = t.lengths + 19;
    int i = 0;
    while (i < nlen + ndist) {
        K9_ITER();
        const int s = k9_symbol(io, b, t.lit_count, t.lit_symbol, nullptr, 0);
        if (s < 0) return -s;
        if (s < 16) { len[i++] = (uint8_t)s; continue; }
        int prev = 0, rep;
        if (s == 16) {
            if (i == 0) return K9_E_CODE_LENGTHS;
            prev = len[i - 1];
            rep = k9_bits(io, b, 2);
            if (rep < 0) return K9_E_TRUNCATED;
            rep += 3;
        } else {
            rep = k9_bits(io, b, s == 17 ? 3 : 7);
            if (rep < 0) return K9_E_TRUNCATED;
            rep += s == 17 ? 3 : 11;
        }
        if (i + rep > nlen + ndist) return K9_E_CODE_LENGTHS;
        while (rep--) len[i++] = (uint8_t)prev;
    }
    if (len[256] == 0) return K9_E_CODE_LENGTHS;  // no end-of-block code
    io.sync();  // the code-length code goes: the literal set takes its arrays
    if (k9_build(len, nlen, t.lit_count, t.lit_symbol, t.lit_fast, K9_FAST_LIT_BITS) != 0) return K9_E_CODE_LENGTHS;
    const int left = k9_build(len + nlen, ndist, t.dist_count, t.dist_symbol, t.dist_fast, K9_FAST_DIST_BITS);
    // incomplete: only no code at all, or a single code of length 1 (its unused twin decodes to K9_E_SYMBOL)
    if (left < 0 || (left > 0 && ndist - (int)t.dist_count[0] > 1) || (left > 0 && ndist - (int)t.dist_count[0] == 1 && t.dist_count[1] != 1)) return K9_E_CODE_LENGTHS;
    return K9_OK;
}

template <class IO>
K9_FN void k9_read_fixed(IO &io) {
    K9Tables &t = io.tables();
    for (int s = 0; s < 288; s++) t.lengths[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < 30; s++) t.lengths[288 + s] = 5;
    k9_build(t.lengths, 288, t.lit_count, t.lit_symbol, t.lit_fast, K9_FAST_LIT_BITS);
    k9_build(t.lengths + 288, 30, t.dist_count, t.dist_symbol, t.dist_fast, K9_FAST_DIST_BITS);
}

// One zlib stream of exactly in_len bytes -> exactly out_len bytes.  K9_OK or the first error; what out[] holds after an error is unspecified
// (but inside out_len).
template <class IO>
K9_FN int k9_inflate_zlib(IO &io, size_t in_len, size_t out_len) {
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    K9Bits b;
    b.total = 8 * in_len;
    k9_seek(io, b, 0);
    const int head = k9_bits(io, b, 16);
    if (head < 0) return K9_E_TRUNCATED;
    const int cmf = head & 255, flg = head >> 8;
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return K9_E_HEADER;
    K9Tables &t = io.tables();
    size_t pos = 0;
    for (int last = 0; !last;) {
        K9_ITER();
        const int bh = k9_bits(io, b, 3);
        if (bh < 0) return K9_E_TRUNCATED;
        last = bh & 1;
        const int type = bh >> 1;
        if (type == 3) return K9_E_BLOCK_TYPE;
        if (type == 0) {
            if (!k9_consume(b, (int)((8 - (b.used & 7)) & 7))) return K9_E_TRUNCATED;
            const int len = k9_bits(io, b, 16);
            const int nlen = k9_bits(io, b, 16);
            if (len < 0 || nlen < 0) return K9_E_TRUNCATED;
            if ((len ^ nlen) != 0xffff) return K9_E_STORED_LEN;
            const size_t src = b.used >> 3;
            if (src + (size_t)len > in_len) return K9_E_TRUNCATED;
            if (pos + (size_t)len > out_len) return K9_E_OVERRUN;
            if (len) io.copy_in(pos, src, (unsigned)len);
            pos += (size_t)len;
            k9_seek(io, b, src + (size_t)len);
            continue;
        }
        io.sync();  // the previous block's tables go
        if (type == 1) k9_read_fixed(io);
        else if (const int e = k9_read_dynamic(io, b)) return e;
        io.sync();
        for (;;) {
            K9_ITER();
            int s = k9_symbol(io, b, t.lit_count, t.lit_symbol, t.lit_fast, K9_FAST_LIT_BITS);
            if (s < 0) return -s;
            if (s < 256) {
                if (pos >= out_len) return K9_E_OVERRUN;
                io.put(pos++, (unsigned)s);
                continue;
            }
            if (s == 256) break;
            s -= 257;
            if (s >= 29) return K9_E_SYMBOL;
            const int lx = k9_bits(io, b, lext[s]);
            if (lx < 0) return K9_E_TRUNCATED;
            const unsigned len = (unsigned)lbase[s] + (unsigned)lx;
            const int d = k9_symbol(io, b, t.dist_count, t.dist_symbol, t.dist_fast, K9_FAST_DIST_BITS);
            if (d < 0) return -d;
            if (d >= 30) return K9_E_SYMBOL;
            const int dx = k9_bits(io, b, dext[d]);
            if (dx < 0) return K9_E_TRUNCATED;
            const unsigned dist = (unsigned)dbase[d] + (unsigned)dx;
            if ((size_t)dist > pos) return K9_E_DISTANCE;
            if (pos + len > out_len) return K9_E_OVERRUN;
            io.copy(pos, dist, len);
            pos += len;
        }
    }
    if (!k9_consume(b, (int)((8 - (b.used & 7)) & 7))) return K9_E_TRUNCATED;
    const int a_hi = k9_bits(io, b, 16);
    const int a_lo = k9_bits(io, b, 16);
    if (a_hi < 0 || a_lo < 0) return K9_E_TRUNCATED;
    if (b.used != b.total) return K9_E_TRAILING;
    if (pos != out_len) return K9_E_SHORT;
    // big-endian in the stream: the 16-bit reads above each hold two bytes least significant first
    const uint32_t want = ((uint32_t)(a_hi & 255) << 24) | ((uint32_t)(a_hi >> 8) << 16) | ((uint32_t)(a_lo & 255) << 8) | (uint32_t)(a_lo >> 8);
    return io.adler(out_len) == want ? K9_OK : K9_E_ADLER;
}

#ifndef K9_NO_HOST_IO
// the host's IO: plain memory, one thread
struct K9HostIO {
    const uint8_t *in;
    size_t in_len;
    uint8_t *out;
    K9Tables t;
    uint32_t word(size_t i) const {
        uint32_t w = 0;
        for (int k = 0; k < 4; k++)
            if (4 * i + (size_t)k < in_len) w |= (uint32_t)in[4 * i + (size_t)k] << (8 * k);
        return w;
    }
    void put(size_t pos, unsigned byte) { out[pos] = (uint8_t)byte; }
    void copy(size_t pos, unsigned dist, unsigned len) {
        for (unsigned k = 0; k < len; k++) out[pos + k] = out[pos - dist + k];
    }
    void copy_in(size_t pos, size_t src, unsigned len) {
        for (unsigned k = 0; k < len; k++) out[pos + k] = in[src + k];
    }
    uint32_t adler(size_t n) const {
        uint32_t a = 1, b = 0;
        for (size_t i = 0; i < n; i++) {
            a = (a + out[i]) % 65521u;
            b = (b + a) % 65521u;
        }
        return (b << 16) | a;
    }
    K9Tables &tables() { return t; }
    void sync() {}
};
K9_FN int k9_inflate_host(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len) {
    K9HostIO io;
    io.in = in; io.in_len = in_len; io.out = out;
    return k9_inflate_zlib(io, in_len, out_len);
}
#endif
