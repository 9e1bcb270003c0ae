// k8_match.h — K8 with run-length matches: form (c) of include/rfx.h "Match form", for both fragment kinds.  Included by k7_export.hip behind
// k8_exr.h.  The literal-only kernels k8_png_rows / k8_exr_rows are not touched: these are second kernels the launchers select when the call
// asked for matches, and they share k8_build_code, the bit window, the wave helpers, the filter stage, the scans and the gather.
//
//   k8_png_rows_m  k8_png_rows / k8_exr_rows over the token rule: a histogram over the 286 literal / length symbols beside the literal one, a
//   k8_exr_rows_m  second code when the scanline holds a match, both forms' sizes before a bit is written, then the smaller form
//
// A scanline's byte sequence d[0, n) is swept 256 positions a step, four a lane, as in the literal kernels; position j is d[j] (PNG: d[0] is
// the type byte).  The rule is evaluated forward only: a token is emitted at the position where it ENDS, so a lane needs its own four bytes, the
// one before them and the two behind them (neighbour lanes by __shfl, the step's two ends from memory) and the position's offset in its
// repeating interval: the distance to the last non-repeating position, a wave max-scan, with the open interval's length carried from step to
// step as a wave-uniform value.  Wave operations: __shfl / __shfl_xor only.
//
// The bit window: a match end costs at most 15 + 5 + 1 = 21 bits and stands for three positions or more, so a step's bits are largest with one
// match that ends on the step's first position and 255 literals: 21 + 255 x 15 = 3846 bits, 3877 with the 31 carried ones — K8_WIN's 4096 hold.
// A lane's four positions can hold 21 + 3 x 15 = 66 bits: the accumulator is 96 bits wide here and leaves for up to four dwords.
#pragma once
#include "k8_exr.h"

namespace {

constexpr int K8M_NSYM = 286;          // literals, end of block, the 29 length symbols
constexpr int K8M_PIECE = 258;         // deflate's longest match
constexpr unsigned K8M_NONE = 0x1ffu;  // stands for d[j] outside [0, n): equal to no byte, and never repeating

struct K8MLds {
    K8Lds b;
    unsigned mfreq[K8_TABLE];  // the histogram of form (c)'s tokens
    unsigned mcode[K8_TABLE];  // ... and its code
};

// ---------------------------------------------------------------- the two byte sequences
struct K8PngSeq {  // the type byte, then the residuals
    const unsigned char *cur, *up;
    int bpp, type, n;
    RFX_DEV unsigned at(int j) const {
        if (j < 0 || j >= n) return K8M_NONE;
        if (j == 0) return (unsigned)type;
        int x, a, b, c;
        k8_fetch(cur, up, bpp, j - 1, x, a, b, c);
        return k8_residual(type, x, a, b, c);
    }
    RFX_DEV void load4(int j0, unsigned d[4]) const {
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = at(j0 + k);
    }
};
struct K8ExrSeq {  // the predicted bytes of the scanline's plane
    const unsigned char *t;
    int n;
    RFX_DEV unsigned at(int j) const {
        if (j < 0 || j >= n) return K8M_NONE;
        return j ? ((unsigned)t[j] - (unsigned)t[j - 1] + 128u) & 255u : (unsigned)t[0];
    }
    RFX_DEV void load4(int j0, unsigned d[4]) const {
        unsigned res[4];
        const int cnt = k8_exr_predict4(t, n, j0, res);
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = k < cnt ? res[k] : K8M_NONE;
    }
};

// ---------------------------------------------------------------- the token rule
// deflate's length symbol, the count of its extra bits and their value for a match of `len` (3..258)
RFX_DEV void k8m_length(int len, int &sym, int &eb, unsigned &ev) {
    const int l = len - 3;
    eb = 0; ev = 0;
    if (len == K8M_PIECE) { sym = 285; return; }
    if (l < 8) { sym = 257 + l; return; }
    eb = l < 16 ? 1 : l < 32 ? 2 : l < 64 ? 3 : l < 128 ? 4 : 5;
    sym = 261 + 4 * eb + ((l >> eb) & 3);
    ev = (unsigned)l & ((1u << eb) - 1u);
}
RFX_DEV int k8m_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// The tokens that end on the lane's four positions base + lane * 4 + k: -1 none, 0..255 a literal, 256 + length a match.  d: the positions'
// bytes (K8M_NONE outside the sequence).  `open`: the count of repeating positions that end just before the step, wave-uniform, in and out.
template <class Seq>
RFX_DEV void k8m_tokens(const Seq &S, int base, int lane, int &open, unsigned d[4], int tok[4]) {
    S.load4(base + lane * 4, d);
    unsigned e[7];
    e[0] = (unsigned)__shfl((int)d[3], lane ? lane - 1 : 0);
    e[5] = (unsigned)__shfl((int)d[0], lane < 63 ? lane + 1 : 63);
    e[6] = (unsigned)__shfl((int)d[1], lane < 63 ? lane + 1 : 63);
    if (lane == 0) e[0] = S.at(base - 1);
    if (lane == 63) { e[5] = S.at(base + 256); e[6] = S.at(base + 257); }
#pragma unroll
    for (int k = 0; k < 4; k++) e[1 + k] = d[k];
    bool rep[6];  // position base + lane * 4 + k repeats its predecessor
#pragma unroll
    for (int k = 0; k < 6; k++) rep[k] = e[k + 1] == e[k] && e[k + 1] != K8M_NONE;
    // the step's last non-repeating position at or before each position: a max-scan over the lanes, then along the lane's four
    int last = -1;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (!rep[k]) last = lane * 4 + k;
    int inc = last;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int t = __shfl(inc, lane >= m ? lane - m : lane);
        if (lane >= m) inc = max(inc, t);
    }
    last = __shfl(inc, lane ? lane - 1 : 0);
    if (lane == 0) last = -1;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int p = lane * 4 + k;
        if (!rep[k]) last = p;
        c = last >= 0 ? p - last : p + 1 + open;  // repeating positions up to and including this one
        tok[k] = -1;
        if (d[k] == K8M_NONE) continue;
        if (c == 0) { tok[k] = (int)d[k]; continue; }
        const int om = (c - 1) % K8M_PIECE;  // the position's offset in its piece
        if (om == 0) { if (!(rep[k + 1] && rep[k + 2])) tok[k] = (int)d[k]; }  // a last piece of 1 or 2 positions is literals
        else if (om == 1) { if (!rep[k + 1]) tok[k] = (int)d[k]; }
        else if (om == K8M_PIECE - 1 || !rep[k + 1]) tok[k] = 256 + om + 1;
    }
    open = __shfl(c, 63);
}

// both histograms (L.b.freq: every byte a literal; L.mfreq: the tokens) and the Adler partial sums; returns the scanline's count of matches
template <class Seq>
RFX_DEV int k8m_histogram(K8MLds &L, const Seq &S, int lane, unsigned long long &s1, unsigned long long &s2) {
    int open = 0, nm = 0;
    for (int base = 0; base < S.n; base += 256) {
        unsigned d[4];
        int tok[4];
        k8m_tokens(S, base, lane, open, d, tok);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (d[k] != K8M_NONE) {
                atomicAdd(&L.b.freq[d[k]], 1u);
                s1 += d[k];
                s2 += (unsigned long long)(S.n - (base + lane * 4 + k)) * d[k];
            }
            if (tok[k] >= 256) {
                int sym, eb;
                unsigned ev;
                k8m_length(tok[k] - 256, sym, eb, ev);
                atomicAdd(&L.mfreq[sym], 1u);
                nm++;
            } else if (tok[k] >= 0) atomicAdd(&L.mfreq[tok[k]], 1u);
        }
    }
    return k8_wave_sum(nm);
}

// ---------------------------------------------------------------- the block header for a code of `nlit` literal / length lengths and one distance length
// The header-token rule over code[0, nlit) and `dlen`, the tokens' code; returns the header's bits after BFINAL / BTYPE.  Ends with a barrier.
RFX_DEV unsigned k8m_header(K8MLds &M, const unsigned *code, int nlit, unsigned dlen, int lane, int &hclen) {
    K8Lds &L = M.b;
    if (lane == 0) {
        for (int i = 0; i < 32; i++) L.clfreq[i] = 0;
        int nt = 0, i = 0;
        const int total = nlit + 1;
        while (i < total) {
            const unsigned v = i < nlit ? code[i] >> 16 : dlen;
            int j = i;
            while (j < total && (j < nlit ? code[j] >> 16 : dlen) == v) j++;
            int r = j - i;
            if (v == 0) {
                while (r >= 11) { const int k = min(r, 138); L.tokens[nt++] = (unsigned short)(18 | ((k - 11) << 8)); L.clfreq[18]++; r -= k; }
                if (r >= 3) { L.tokens[nt++] = (unsigned short)(17 | ((r - 3) << 8)); L.clfreq[17]++; r = 0; }
                for (; r > 0; r--) { L.tokens[nt++] = 0; L.clfreq[0]++; }
            } else {
                L.tokens[nt++] = (unsigned short)v; L.clfreq[v]++; r--;
                while (r >= 3) { const int k = min(r, 6); L.tokens[nt++] = (unsigned short)(16 | ((k - 3) << 8)); L.clfreq[16]++; r -= k; }
                for (; r > 0; r--) { L.tokens[nt++] = (unsigned short)v; L.clfreq[v]++; }
            }
            i = j;
        }
        L.ntokens = nt;
    }
    __syncthreads();
    k8_build_code(L, L.clfreq, K8_NCL, K8_CL_MAXBITS, L.clcode, lane);
    hclen = 4;
    for (int i = 0; i < K8_NCL; i++)
        if (L.clcode[k8_cl_order[i]] >> 16) hclen = max(hclen, i + 1);
    unsigned bits = 5u + 5u + 4u + 3u * (unsigned)hclen;
    for (int i = 0; i < L.ntokens; i++) {
        const int sym = L.tokens[i] & 255;
        bits += (L.clcode[sym] >> 16) + (sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u);
    }
    __syncthreads();  // (every lane has read the tokens before a second header may overwrite them)
    return bits;
}
RFX_DEV void k8m_put_header(K8MLds &M, unsigned &pos, int nlit, int hclen, bool w) {
    K8Lds &L = M.b;
    k8_put(L, pos, (unsigned)(nlit - 257), 5, w);  // HLIT
    k8_put(L, pos, 0u, 5, w);                      // HDIST: 1 code
    k8_put(L, pos, (unsigned)(hclen - 4), 4, w);
    for (int i = 0; i < hclen; i++) k8_put(L, pos, L.clcode[k8_cl_order[i]] >> 16, 3, w);
    const int ntokens = L.ntokens;
    for (int i = 0; i < ntokens; i++) {
        const unsigned t = L.tokens[i], sym = t & 255u, c = L.clcode[sym];
        k8_put(L, pos, c & 0xffffu, (int)(c >> 16), w);
        k8_put(L, pos, t >> 8, sym == 16u ? 2 : sym == 17u ? 3 : sym == 18u ? 7 : 0, w);
    }
}
// the bits of the tokens counted in freq[0, n) under `code`: the code's bits, a length symbol's extra bits and its distance bit
RFX_DEV unsigned k8m_body_bits(const unsigned *freq, const unsigned *code, int n, int lane) {
    int bits = 0;
    for (int i = lane; i < n; i += 64) bits += (int)(freq[i] * ((code[i] >> 16) + (i > 256 ? 1u + (unsigned)k8m_extra_bits(i) : 0u)));
    return (unsigned)k8_wave_sum(bits);
}

// ---------------------------------------------------------------- the tokens' bits through the window
RFX_DEV void k8m_add(unsigned long long &lo, unsigned &hi, int &nb, unsigned v, int bits) {  // v: at most 32 - 11 bits
    if (nb < 64) {
        lo |= (unsigned long long)v << nb;
        if (nb + bits > 64) hi |= v >> (64 - nb);
    } else hi |= v << (nb - 64);
    nb += bits;
}
// `matches`: the tokens of form (c) under its code; else every position a literal (form (a))
template <class Seq>
RFX_DEV void k8m_emit(K8MLds &M, const Seq &S, const unsigned *code, bool matches, unsigned *out, unsigned cap, unsigned &outdw, unsigned &pos, int lane) {
    K8Lds &L = M.b;
    int open = 0;
    for (int base = 0; base < S.n; base += 256) {
        unsigned d[4];
        int tok[4];
        if (matches) k8m_tokens(S, base, lane, open, d, tok);
        else {
            S.load4(base + lane * 4, d);
#pragma unroll
            for (int k = 0; k < 4; k++) tok[k] = d[k] == K8M_NONE ? -1 : (int)d[k];
        }
        unsigned long long lo = 0;
        unsigned hi = 0;
        int nb = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (tok[k] >= 256) {
                int sym, eb;
                unsigned ev;
                k8m_length(tok[k] - 256, sym, eb, ev);
                const unsigned c = code[sym];
                const int l = (int)(c >> 16);
                k8m_add(lo, hi, nb, (c & 0xffffu) | (ev << l), l + eb + 1);  // the symbol, its extra bits, the distance code `0`
            } else if (tok[k] >= 0) {
                const unsigned c = code[tok[k]];
                k8m_add(lo, hi, nb, c & 0xffffu, (int)(c >> 16));
            }
        }
        int total;
        const unsigned o = pos + (unsigned)k8_wave_scan(nb, lane, total);
        if (nb) {
            const unsigned wi = o >> 5, sh = o & 31u;
            const unsigned x0 = (unsigned)lo, x1 = (unsigned)(lo >> 32);
            const unsigned w0 = x0 << sh;
            const unsigned w1 = sh ? (x1 << sh) | (x0 >> (32u - sh)) : x1;
            const unsigned w2 = sh ? (hi << sh) | (x1 >> (32u - sh)) : hi;
            const unsigned w3 = sh ? hi >> (32u - sh) : 0u;
            if (w0) atomicOr(&L.win[wi], w0);
            if (w1) atomicOr(&L.win[wi + 1], w1);
            if (w2) atomicOr(&L.win[wi + 2], w2);
            if (w3) atomicOr(&L.win[wi + 3], w3);
        }
        pos += (unsigned)total;
        k8_flush(L, out, cap, outdw, pos, lane, false);
    }
}

// The forms' sizes in bits after BFINAL / BTYPE, before a bit is written.  On return L.b.code holds form (a)'s code, and, when the scanline has
// a match, L.mcode form (c)'s; the header tokens in LDS are form (c)'s then, form (a)'s otherwise.
RFX_DEV void k8m_sizes(K8MLds &L, int nmatch, int lane, unsigned &abits, int &ahclen, unsigned &cbits, int &chclen, int &nlit) {
    k8_build_code(L.b, L.b.freq, K8_NSYM, K8_MAXBITS, L.b.code, lane);
    abits = k8m_header(L, L.b.code, K8_NSYM, 0u, lane, ahclen) + k8m_body_bits(L.b.freq, L.b.code, K8_NSYM, lane);
    cbits = 0; chclen = 0; nlit = K8_NSYM;
    if (nmatch) {
        k8_build_code(L.b, L.mfreq, K8M_NSYM, K8_MAXBITS, L.mcode, lane);
        for (int i = K8M_NSYM - 1; i >= K8_NSYM; i--)
            if (L.mcode[i] >> 16) { nlit = i + 1; break; }
        cbits = k8m_header(L, L.mcode, nlit, 1u, lane, chclen) + k8m_body_bits(L.mfreq, L.mcode, K8M_NSYM, lane);
    }
}

__global__ __launch_bounds__(64) void k8_png_rows_m(K8Args A) {
    __shared__ K8MLds L;
    const int lane = (int)threadIdx.x;
    const int s = (int)blockIdx.x;  // PNG scanline of the tile, 0 = top = stream row rows - 1
    const int rowbytes = A.rowbytes, bpp = A.bpp, n = rowbytes + 1;
    const unsigned char *cur = A.src + (size_t)(A.rows - 1 - s) * (size_t)rowbytes;
    const unsigned char *up = s ? cur + rowbytes : nullptr;
    unsigned char *slot = A.slots + (size_t)s * A.slot_stride;
    unsigned *out = (unsigned *)(slot + 8);
    const unsigned cap = (A.slot_stride - 8u) / 4u;

    K8PngSeq S;
    S.cur = cur; S.up = up; S.bpp = bpp; S.n = n;
    S.type = k8_choose_filter(cur, up, rowbytes, bpp, A.filter, lane);

    for (int i = lane; i < K8_TABLE; i += 64) { L.b.freq[i] = 0; L.mfreq[i] = 0; }
    for (int i = lane; i < K8_WIN; i += 64) L.b.win[i] = 0;
    for (int i = lane; i < 256; i += 64) {
        unsigned c = (unsigned)i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ K8_CRC_POLY : c >> 1;
        L.b.crc_table[i] = c;
    }
    __syncthreads();
    if (lane == 0) { L.b.freq[256] = 1; L.mfreq[256] = 1; }
    unsigned long long s1 = 0, s2 = 0;
    const int nmatch = k8m_histogram(L, S, lane, s1, s2);
    const unsigned ad1 = (unsigned)k8_wave_sum((int)(s1 % K8_ADLER)) % K8_ADLER;
    const unsigned ad2 = (unsigned)k8_wave_sum((int)(s2 % K8_ADLER)) % K8_ADLER;
    __syncthreads();

    unsigned abits, cbits;
    int hclen, chclen, nlit;
    k8m_sizes(L, nmatch, lane, abits, hclen, cbits, chclen, nlit);
    const unsigned nblk = ((unsigned)n + 65534u) / 65535u;
    const unsigned stored_bytes = (unsigned)n + 5u * nblk;
    const unsigned a_bytes = (3u + abits + 3u + 7u) / 8u + 4u, c_bytes = (3u + cbits + 3u + 7u) / 8u + 4u;
    const bool form_c = nmatch && c_bytes < min(a_bytes, stored_bytes);
    unsigned plen;

    if (form_c || a_bytes <= stored_bytes) {
        // (c) or (a): the block header, the tokens, end of block and the empty stored block
        if (nmatch && !form_c) k8m_header(L, L.b.code, K8_NSYM, 0u, lane, hclen);  // (the tokens in LDS were form (c)'s)
        const unsigned *code = form_c ? L.mcode : L.b.code;
        unsigned pos = 0, outdw = 0;
        const bool w = lane == 0;
        k8_put(L.b, pos, 4u, 3, w);  // BFINAL 0, BTYPE 2
        k8m_put_header(L, pos, form_c ? nlit : K8_NSYM, form_c ? chclen : hclen, w);
        k8_flush(L.b, out, cap, outdw, pos, lane, false);
        k8m_emit(L, S, code, form_c, out, cap, outdw, pos, lane);
        const unsigned ce = code[256];
        k8_put(L.b, pos, ce & 0xffffu, (int)(ce >> 16), w);
        k8_put(L.b, pos, 0u, 3, w);  // BFINAL 0, BTYPE 0
        pos = (pos + 7u) & ~7u;
        k8_put(L.b, pos, 0x0000u, 16, w);
        k8_put(L.b, pos, 0xffffu, 16, w);
        plen = min(outdw * 4u + pos / 8u, stored_bytes);  // (= c_bytes or a_bytes: the sizes above are the emission's)
        k8_flush(L.b, out, cap, outdw, pos, lane, true);
    } else {
        // (b) stored blocks of at most 65535 filtered bytes: 00, LEN, ~LEN, the bytes
        unsigned char *p = slot + 8;
        for (unsigned k = (unsigned)lane; k < nblk; k += 64u) {
            const unsigned len = min(65535u, (unsigned)n - k * 65535u), at = k * 65540u;
            p[at] = 0;
            p[at + 1] = (unsigned char)(len & 255u); p[at + 2] = (unsigned char)(len >> 8);
            p[at + 3] = (unsigned char)(~len & 255u); p[at + 4] = (unsigned char)((~len >> 8) & 255u);
        }
        for (int base = 0; base < n; base += 256) {
            unsigned d[4];
            S.load4(base + lane * 4, d);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (d[k] != K8M_NONE) {
                    const unsigned q = (unsigned)(base + lane * 4 + k);
                    p[q + 5u * (q / 65535u + 1u)] = (unsigned char)d[k];
                }
            }
        }
        plen = stored_bytes;
        __syncthreads();
    }

    // the chunk's CRC-32, as k8_png_rows
    {
        const unsigned char *p = slot + 8;
        const unsigned seg = (plen + 63u) / 64u;
        const unsigned b0 = min(plen, (unsigned)lane * seg), b1 = min(plen, b0 + seg);
        unsigned crc = 0;
        if (b1 > b0) {
            crc = 0xffffffffu;
            for (unsigned i = b0; i < b1; i++) crc = L.b.crc_table[(crc ^ p[i]) & 255u] ^ (crc >> 8);
            crc = k8_crc_shift(~crc, plen - b1);
        }
        if (lane == 0) crc ^= k8_crc_shift(K8_CRC_IDAT, plen);
        crc = k8_wave_xor(crc);
        if (lane == 0) {
            ((unsigned *)slot)[0] = ((plen & 255u) << 24) | ((plen & 0xff00u) << 8) | ((plen >> 8) & 0xff00u) | (plen >> 24);  // big-endian
            ((unsigned *)slot)[1] = 0x54414449u;  // "IDAT"
            unsigned char *e = slot + 8 + plen;
            e[0] = (unsigned char)(crc >> 24); e[1] = (unsigned char)(crc >> 16); e[2] = (unsigned char)(crc >> 8); e[3] = (unsigned char)crc;
            unsigned *m = A.meta + 4 * (size_t)s;
            m[0] = plen + 12u; m[1] = ad1; m[2] = ad2; m[3] = form_c ? 1u : 0u;
        }
    }
}

__global__ __launch_bounds__(64) void k8_exr_rows_m(K8ExrArgs A) {
    __shared__ K8MLds L;
    const int lane = (int)threadIdx.x;
    const int s = (int)blockIdx.x;
    const int n = 2 * A.width * A.channels;
    unsigned char *slot = A.slots + (size_t)s * A.slot_stride;
    unsigned *out = (unsigned *)(slot + 8);
    const unsigned cap = (A.slot_stride - 8u) / 4u;
    K8ExrSeq S;
    S.t = A.planes + (size_t)s * A.plane_stride; S.n = n;

    for (int i = lane; i < K8_TABLE; i += 64) { L.b.freq[i] = 0; L.mfreq[i] = 0; }
    for (int i = lane; i < K8_WIN; i += 64) L.b.win[i] = 0;
    __syncthreads();
    if (lane == 0) { L.b.freq[256] = 1; L.mfreq[256] = 1; }
    unsigned long long s1 = 0, s2 = 0;
    const int nmatch = k8m_histogram(L, S, lane, s1, s2);
    const unsigned ad1 = (1u + (unsigned)k8_wave_sum((int)(s1 % K8_ADLER))) % K8_ADLER;
    const unsigned ad2 = ((unsigned)(n % (int)K8_ADLER) + (unsigned)k8_wave_sum((int)(s2 % K8_ADLER))) % K8_ADLER;
    __syncthreads();

    unsigned abits, cbits;
    int hclen, chclen, nlit;
    k8m_sizes(L, nmatch, lane, abits, hclen, cbits, chclen, nlit);
    const unsigned a_bytes = 2u + (3u + abits + 7u) / 8u + 4u, c_bytes = 2u + (3u + cbits + 7u) / 8u + 4u;
    const bool form_c = nmatch && c_bytes < min(a_bytes, (unsigned)n);
    unsigned size;

    if (form_c || a_bytes < (unsigned)n) {
        // (c) or (a): 78 01, the FINAL dynamic block: header, tokens, end of block; padding to a byte; the Adler-32, big-endian
        if (nmatch && !form_c) k8m_header(L, L.b.code, K8_NSYM, 0u, lane, hclen);  // (the tokens in LDS were form (c)'s)
        const unsigned *code = form_c ? L.mcode : L.b.code;
        unsigned pos = 0, outdw = 0;
        const bool w = lane == 0;
        k8_put(L.b, pos, 0x0178u, 16, w);
        k8_put(L.b, pos, 5u, 3, w);  // BFINAL 1, BTYPE 2
        k8m_put_header(L, pos, form_c ? nlit : K8_NSYM, form_c ? chclen : hclen, w);
        k8_flush(L.b, out, cap, outdw, pos, lane, false);
        k8m_emit(L, S, code, form_c, out, cap, outdw, pos, lane);
        const unsigned ce = code[256];
        k8_put(L.b, pos, ce & 0xffffu, (int)(ce >> 16), w);
        pos = (pos + 7u) & ~7u;
        k8_put(L.b, pos, ((ad2 >> 8) & 255u) | ((ad2 & 255u) << 8), 16, w);
        k8_put(L.b, pos, ((ad1 >> 8) & 255u) | ((ad1 & 255u) << 8), 16, w);
        size = outdw * 4u + pos / 8u;  // (= c_bytes or a_bytes: the sizes above are the emission's)
        k8_flush(L.b, out, cap, outdw, pos, lane, true);
    } else {
        // (b) the raw block: half j of the scanline is t[j] | t[n / 2 + j] << 8
        unsigned short *p = (unsigned short *)(slot + 8);
        const int m = n / 2;
        for (int j = lane; j < m; j += 64) p[j] = (unsigned short)((unsigned)S.t[j] | ((unsigned)S.t[m + j] << 8));
        size = (unsigned)n;
    }
    if (lane == 0) {
        ((int *)slot)[0] = A.first_y + s;
        ((unsigned *)slot)[1] = size;
        unsigned *mt = A.meta + 4 * (size_t)s;
        mt[0] = size + 8u; mt[1] = (!form_c && size == (unsigned)n) ? 1u : 0u; mt[2] = form_c ? 1u : 0u; mt[3] = 0;
    }
}

}  // namespace

hipError_t rfx_launch_k8_rows_m(const K8Args &A, hipStream_t stream) {
    hipLaunchKernelGGL(k8_png_rows_m, dim3(A.rows), dim3(64), 0, stream, A);
    return hipGetLastError();
}
hipError_t rfx_launch_k8_exr_rows_m(const K8ExrArgs &A, hipStream_t stream) {
    hipLaunchKernelGGL(k8_exr_rows_m, dim3(A.rows), dim3(64), 0, stream, A);
    return hipGetLastError();
}
