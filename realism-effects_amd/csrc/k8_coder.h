// k8_coder.h — K8's deflate coder: everything the scanline kernels of k8_png.h and k8_exr.h share, none of which knows which fragment it
// serves.  A scanline is a byte sequence S: S.n bytes, S.at(j) byte j (K8_NONE outside [0, n)), S.load4(j0, d) four of them and how many of
// the four lie inside, Seq::LEAD bytes in front of what its pre-transform produces (k8_first).  The coder sweeps it 256 positions a step,
// four a lane, one wave (a workgroup of 64 lanes) per scanline, and every rule is written once, for both forms of the dynamic block
// (include/rfx.h "PNG fragments", "Match form"):
//
//   (a) every byte a literal               MATCHES false: K8Lds alone, a 64-bit accumulator; also what a scanline without a match gets
//   (c) runs of one byte value as matches  MATCHES true: K8MLds (the token histogram and its code beside form (a)'s), the token rule, a
//                                          96-bit accumulator; both forms' sizes are known before a bit is written, the kernel takes the smaller
//
//   k8_build_code                 the code-length rule of rfx.h and the canonical codes
//   k8_put, k8_flush              the bit window
//   k8m_length, k8m_tokens        the token rule
//   k8_histogram                  the sweep that counts: both histograms and the Adler partial sums
//   k8_header, k8_put_header      the header-token rule (16 / 17 / 18) and the block header's emission
//   k8_body_bits, k8_sizes        the forms' sizes
//   k8_emit                       the sweep that packs the tokens' bits
//   k8_block                      the dynamic block behind BFINAL / BTYPE: header, tokens, end of block
//
// The sequence is never staged in LDS (a 32768 x 4 row is 131 073 bytes): it is read three times — filter costs (PNG), histogram, codes — from
// L2, where K7 just put it.  Bits are assembled in a 512-byte LDS window with atomicOr and leave it as whole dwords.  The window: a literal
// costs at most 15 bits, a match end at most 15 + 5 + 1 = 21 and stands for three positions or more, so a step's bits are largest with one
// match that ends on the step's first position and 255 literals: 21 + 255 x 15 = 3846 bits, 3877 with the 31 carried ones — K8_WIN's 4096 hold
// (the header, at most 287 tokens, stays below 2200).  A lane's four positions hold at most 60 bits as literals and 21 + 3 x 15 = 66 with a
// match, hence the two accumulators.  The rule is evaluated forward only: a token is emitted at the position where it ENDS, so a lane needs
// its own four bytes, the one before them and the two behind them (neighbour lanes by __shfl, the step's two ends from memory) and the
// position's offset in its repeating interval: the distance to the last non-repeating position, a wave max-scan, with the open interval's
// length carried from step to step as a wave-uniform value.  Wave operations: __shfl / __shfl_xor only.
#pragma once
#include <type_traits>
#include "rfx_device.h"
#include "rfx_kernels.h"

namespace {

constexpr int K8_NSYM = 257, K8_NCL = 19, K8_MAXBITS = 15, K8_CL_MAXBITS = 7;
constexpr int K8_TABLE = 288;         // a code's tables: 257 symbols (286 with the length symbols) rounded up
constexpr int K8_WIN = 128;           // the bit window, dwords
constexpr unsigned K8_ADLER = 65521u;
constexpr int K8M_NSYM = 286;         // literals, end of block, the 29 length symbols
constexpr int K8M_PIECE = 258;        // deflate's longest match
constexpr unsigned K8_NONE = 0x1ffu;  // stands for S.at(j) outside [0, n): equal to no byte, and never repeating
__constant__ int k8_cl_order[K8_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct K8Lds {
    unsigned freq[K8_TABLE];           // the scanline's histogram: 256 literals and the end-of-block symbol
    unsigned code[K8_TABLE];           // bit-reversed canonical code | length << 16
    unsigned work[K8_TABLE];           // Moffat-Katajainen's array
    unsigned short sorted[K8_TABLE];   // used symbols by rank: frequency descending, symbol ascending
    unsigned short tokens[K8_TABLE];   // the code-length sequence: symbol | extra value << 8
    unsigned clfreq[32], clcode[32];
    unsigned win[K8_WIN];
    unsigned crc_table[256];           // (the PNG chunk's)
    int count[K8_MAXBITS + 1];
    unsigned next_code[K8_MAXBITS + 1];
    int ntokens;
};
struct K8MLds {
    K8Lds b;
    unsigned mfreq[K8_TABLE];  // the histogram of form (c)'s tokens
    unsigned mcode[K8_TABLE];  // ... and its code
};
template <bool MATCHES> using K8LdsFor = std::conditional_t<MATCHES, K8MLds, K8Lds>;
RFX_DEV K8Lds &k8_base(K8Lds &L) { return L; }
RFX_DEV K8Lds &k8_base(K8MLds &L) { return L.b; }

// ---------------------------------------------------------------- wave helpers (64 lanes, every lane present)
RFX_DEV int k8_wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
RFX_DEV unsigned k8_wave_xor(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v ^= (unsigned)__shfl_xor((int)v, m);
    return v;
}
// exclusive prefix sum over the lanes; `total` = the wave's sum
RFX_DEV int k8_wave_scan(int v, int lane, int &total) {
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl(inc, lane >= d ? lane - d : lane);
        if (lane >= d) inc += t;
    }
    total = __shfl(inc, 63);
    return inc - v;
}

// ---------------------------------------------------------------- the code-length rule of rfx.h, and the canonical codes
// freq[0, n) -> code[0, n) (bit-reversed code | length << 16; 0 for an unused symbol).  The ranking is spread over the lanes; the tree, the
// length limit and the code assignment are one lane's serial pass.  Ends with a barrier.
RFX_DEV void k8_build_code(K8Lds &L, const unsigned *freq, int n, int maxbits, unsigned *code, int lane) {
    for (int s = lane; s < n; s += 64) {
        const unsigned f = freq[s];
        if (f) {
            int r = 0;
#pragma unroll 4  // (all 19 compares of the code-length code in flight at once run the kernel out of scalar registers)
            for (int j = 0; j < n; j++) {
                const unsigned fj = freq[j];
                r += (fj > f || (fj == f && j < s)) ? 1 : 0;
            }
            L.sorted[r] = (unsigned short)s;
        }
    }
    __syncthreads();
    if (lane == 0) {
        int m = 0;
        for (int s = 0; s < n; s++) { m += freq[s] ? 1 : 0; code[s] = 0; }
        int *count = L.count;
        for (int i = 0; i <= maxbits; i++) count[i] = 0;
        if (m == 1) {
            count[1] = 1;
        } else if (m > 1) {
            unsigned *A = L.work;  // ascending frequencies: A[i] = the frequency of rank m - 1 - i
            for (int i = 0; i < m; i++) A[i] = freq[L.sorted[m - 1 - i]];
            A[0] += A[1];
            int root = 0, leaf = 2;
            for (int next = 1; next < m - 1; next++) {
                if (leaf >= m || A[root] <= A[leaf]) { A[next] = A[root]; A[root++] = (unsigned)next; } else A[next] = A[leaf++];
                if (leaf >= m || (root < next && A[root] <= A[leaf])) { A[next] += A[root]; A[root++] = (unsigned)next; } else A[next] += A[leaf++];
            }
            A[m - 2] = 0;
            for (int next = m - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
            int avbl = 1, used = 0, dpth = 0;
            root = m - 2;
            int next = m - 1;
            while (avbl > 0) {
                while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
                while (avbl > used) { A[next--] = (unsigned)dpth; avbl--; }
                avbl = 2 * used; dpth++; used = 0;
            }
            for (int i = 0; i < m; i++) count[min((int)A[i], maxbits)]++;
            unsigned total = 0;
            for (int i = 1; i <= maxbits; i++) total += (unsigned)count[i] << (maxbits - i);
            while (total > (1u << maxbits)) {
                count[maxbits]--;
                for (int i = maxbits - 1; i > 0; i--)
                    if (count[i]) { count[i]--; count[i + 1] += 2; break; }
                total--;
            }
        }
        // lengths by rank, shortest first; then deflate's canonical codes in symbol order
        int k = 0;
        for (int i = 1; i <= maxbits; i++)
            for (int j = 0; j < count[i]; j++) code[L.sorted[k++]] = (unsigned)i << 16;
        unsigned *next_code = L.next_code;
        unsigned c = 0;
        count[0] = 0;
        for (int b = 1; b <= maxbits; b++) { c = (c + (unsigned)count[b - 1]) << 1; next_code[b] = c; }
        for (int s = 0; s < n; s++) {
            const int l = (int)(code[s] >> 16);
            if (!l) continue;
            const unsigned v = next_code[l]++;
            unsigned rev = 0;
            for (int b = 0; b < l; b++) rev |= ((v >> b) & 1u) << (l - 1 - b);
            code[s] = rev | ((unsigned)l << 16);
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------- the bit window
// every lane keeps the same `pos` (bits in the window); one lane writes
RFX_DEV void k8_put(K8Lds &L, unsigned &pos, unsigned value, int nbits, bool writer) {
    if (writer && nbits) {
        const unsigned w = pos >> 5, sh = pos & 31u;
        L.win[w] |= value << sh;
        if (sh + (unsigned)nbits > 32u) L.win[w + 1] |= value >> (32u - sh);
    }
    pos += (unsigned)nbits;
}
// whole dwords leave the window for out[outdw ...] (never past `cap` dwords); the bits of the last, partial dword stay as the window's first.
// `final`: the partial dword leaves too.
RFX_DEV void k8_flush(K8Lds &L, unsigned *out, unsigned cap, unsigned &outdw, unsigned &pos, int lane, bool final) {
    __syncthreads();
    const unsigned full = final ? (pos + 31u) >> 5 : pos >> 5;
    for (unsigned i = (unsigned)lane; i < full; i += 64u)
        if (outdw + i < cap) out[outdw + i] = L.win[i];
    const unsigned carry = final ? 0u : L.win[full];
    __syncthreads();
    for (int i = lane; i < K8_WIN; i += 64) L.win[i] = 0;
    if (lane == 0) L.win[0] = carry;
    __syncthreads();
    outdw += full;
    pos = final ? 0u : (pos & 31u);
}

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
// bytes (K8_NONE outside the sequence), returns how many lie inside.  `open`: the count of repeating positions that end just before the
// step, wave-uniform, in and out.
template <class Seq>
RFX_DEV int k8m_tokens(const Seq &S, int base, int lane, int &open, unsigned d[4], int tok[4]) {
    const int cnt = S.load4(base + lane * 4, d);
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
    for (int k = 0; k < 6; k++) rep[k] = e[k + 1] == e[k] && e[k + 1] != K8_NONE;
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
        if (d[k] == K8_NONE) continue;
        if (c == 0) { tok[k] = (int)d[k]; continue; }
        const int om = (c - 1) % K8M_PIECE;  // the position's offset in its piece
        if (om == 0) { if (!(rep[k + 1] && rep[k + 2])) tok[k] = (int)d[k]; }  // a last piece of 1 or 2 positions is literals
        else if (om == 1) { if (!rep[k + 1]) tok[k] = (int)d[k]; }
        else if (om == K8M_PIECE - 1 || !rep[k + 1]) tok[k] = 256 + om + 1;
    }
    open = __shfl(c, 63);
    return cnt;
}

// ---------------------------------------------------------------- the sweep that counts
// The tables and the window start at zero; the caller's barrier follows.
template <class Lds>
RFX_DEV void k8_clear(Lds &L, int lane) {
    K8Lds &B = k8_base(L);
    for (int i = lane; i < K8_TABLE; i += 64) {
        B.freq[i] = 0;
        if constexpr (std::is_same_v<Lds, K8MLds>) L.mfreq[i] = 0;
    }
    for (int i = lane; i < K8_WIN; i += 64) B.win[i] = 0;
}
// Where the sweeps start.  The token rule needs every position in the sweep; the literals' sweep starts behind the sequence's Seq::LEAD bytes
// (the PNG type byte), which lane 0 takes beside it, so that its steps are 256 of the bytes the pre-transform produces.
template <bool MATCHES, class Seq>
constexpr int k8_first() { return MATCHES ? 0 : Seq::LEAD; }
// The histogram of the sequence's bytes and of end of block (freq: every byte a literal; with MATCHES the tokens' beside it, mfreq) and the
// Adler partial sums: sum of bytes, sum of (n - position) * byte, per lane.  Returns the scanline's count of matches.
template <bool MATCHES, class Seq>
RFX_DEV int k8_histogram(K8LdsFor<MATCHES> &L, const Seq &S, int lane, unsigned long long &s1, unsigned long long &s2) {
    K8Lds &B = k8_base(L);
    constexpr int first = k8_first<MATCHES, Seq>();
    if (lane == 0) {
        B.freq[256] = 1;
        if constexpr (MATCHES) L.mfreq[256] = 1;
        for (int j = 0; j < first; j++) {
            const unsigned v = S.at(j);
            atomicAdd(&B.freq[v], 1u);
            s1 += v;
            s2 += (unsigned long long)(S.n - j) * v;
        }
    }
    int open = 0, nm = 0;
    for (int base = first; base < S.n; base += 256) {
        const int j0 = base + lane * 4;
        unsigned d[4];
        int cnt;
        if constexpr (MATCHES) {
            int tok[4];
            cnt = k8m_tokens(S, base, lane, open, d, tok);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (tok[k] >= 256) {
                    int sym, eb;
                    unsigned ev;
                    k8m_length(tok[k] - 256, sym, eb, ev);
                    atomicAdd(&L.mfreq[sym], 1u);
                    nm++;
                } else if (tok[k] >= 0) atomicAdd(&L.mfreq[tok[k]], 1u);
            }
        } else cnt = S.load4(j0, d);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < cnt) {
                atomicAdd(&B.freq[d[k]], 1u);
                s1 += d[k];
                s2 += (unsigned long long)(S.n - (j0 + k)) * d[k];
            }
        }
    }
    if constexpr (MATCHES) nm = k8_wave_sum(nm);
    return nm;
}

// ---------------------------------------------------------------- the block header for a code of `nlit` literal / length lengths and one distance length
// The header-token rule over code[0, nlit) and `dlen`, the tokens' code; returns the header's bits after BFINAL / BTYPE.  Ends with a barrier.
RFX_DEV unsigned k8_header(K8Lds &L, const unsigned *code, int nlit, unsigned dlen, int lane, int &hclen) {
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
RFX_DEV void k8_put_header(K8Lds &L, unsigned &pos, int nlit, int hclen, bool w) {
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

// ---------------------------------------------------------------- the forms' sizes
// the bits of the tokens counted in freq[0, n) under `code`: the code's bits, a length symbol's extra bits and its distance bit
RFX_DEV unsigned k8_body_bits(const unsigned *freq, const unsigned *code, int n, int lane) {
    int bits = 0;
    for (int i = lane; i < n; i += 64) bits += (int)(freq[i] * ((code[i] >> 16) + (i > 256 ? 1u + (unsigned)k8m_extra_bits(i) : 0u)));
    return (unsigned)k8_wave_sum(bits);
}
struct K8Forms {
    unsigned abits, cbits;  // form (a)'s and form (c)'s bits after BFINAL / BTYPE (cbits: 0 without a match)
    int ahclen, chclen, nlit, nmatch;
};
// Both codes and both sizes, before a bit is written.  On return freq's code is form (a)'s, and, when the scanline has a match, mcode form
// (c)'s; the header tokens in LDS are form (c)'s then, form (a)'s otherwise.
template <bool MATCHES>
RFX_DEV K8Forms k8_sizes(K8LdsFor<MATCHES> &L, int nmatch, int lane) {
    K8Lds &B = k8_base(L);
    K8Forms F = {0u, 0u, 0, 0, K8_NSYM, nmatch};
    k8_build_code(B, B.freq, K8_NSYM, K8_MAXBITS, B.code, lane);
    F.abits = k8_header(B, B.code, K8_NSYM, 0u, lane, F.ahclen) + k8_body_bits(B.freq, B.code, K8_NSYM, lane);
    if constexpr (MATCHES) {
        if (nmatch) {
            k8_build_code(B, L.mfreq, K8M_NSYM, K8_MAXBITS, L.mcode, lane);
            for (int i = K8M_NSYM - 1; i >= K8_NSYM; i--)
                if (L.mcode[i] >> 16) { F.nlit = i + 1; break; }
            F.cbits = k8_header(B, L.mcode, F.nlit, 1u, lane, F.chclen) + k8_body_bits(L.mfreq, L.mcode, K8M_NSYM, lane);
        }
    }
    return F;
}

// ---------------------------------------------------------------- the sweep that packs
// a lane's bits of one step: `lo` alone for literals, `hi` behind it with matches (v: at most 32 - 11 bits)
template <bool MATCHES>
RFX_DEV void k8_add(unsigned long long &lo, unsigned &hi, int &nb, unsigned v, int bits) {
    if constexpr (MATCHES) {
        if (nb < 64) {
            lo |= (unsigned long long)v << nb;
            if (nb + bits > 64) hi |= v >> (64 - nb);
        } else hi |= v << (nb - 64);
    } else lo |= (unsigned long long)v << nb;
    nb += bits;
}
// The sequence's tokens under `code` through the window, from position k8_first on.  `form_c` (MATCHES only): the tokens of form (c); else
// every position a literal.
template <bool MATCHES, class Seq>
RFX_DEV void k8_emit(K8Lds &L, const Seq &S, const unsigned *code, bool form_c, unsigned *out, unsigned cap, unsigned &outdw, unsigned &pos, int lane) {
    [[maybe_unused]] int open = 0;
    for (int base = k8_first<MATCHES, Seq>(); base < S.n; base += 256) {
        unsigned d[4];
        int tok[4];
        bool literals = true;
        if constexpr (MATCHES) {
            if (form_c) { k8m_tokens(S, base, lane, open, d, tok); literals = false; }
        }
        if (literals) {
            const int cnt = S.load4(base + lane * 4, d);
#pragma unroll
            for (int k = 0; k < 4; k++) tok[k] = k < cnt ? (int)d[k] : -1;
        }
        unsigned long long lo = 0;
        unsigned hi = 0;
        int nb = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if constexpr (MATCHES) {
                if (tok[k] >= 256) {
                    int sym, eb;
                    unsigned ev;
                    k8m_length(tok[k] - 256, sym, eb, ev);
                    const unsigned c = code[sym];
                    const int l = (int)(c >> 16);
                    k8_add<true>(lo, hi, nb, (c & 0xffffu) | (ev << l), l + eb + 1);  // the symbol, its extra bits, the distance code `0`
                    continue;
                }
            }
            if (tok[k] >= 0) {
                const unsigned c = code[tok[k]];
                k8_add<MATCHES>(lo, hi, nb, c & 0xffffu, (int)(c >> 16));
            }
        }
        int total;
        const unsigned o = pos + (unsigned)k8_wave_scan(nb, lane, total);
        if (nb) {
            const unsigned wi = o >> 5, sh = o & 31u;
            const unsigned long long l = lo << sh;
            const unsigned w0 = (unsigned)l, w1 = (unsigned)(l >> 32);
            unsigned w2 = sh ? (unsigned)(lo >> (64u - sh)) : 0u;
            if constexpr (MATCHES) {
                w2 |= hi << sh;
                const unsigned w3 = sh ? hi >> (32u - sh) : 0u;
                if (w3) atomicOr(&L.win[wi + 3], w3);
            }
            if (w0) atomicOr(&L.win[wi], w0);
            if (w1) atomicOr(&L.win[wi + 1], w1);
            if (w2) atomicOr(&L.win[wi + 2], w2);
        }
        pos += (unsigned)total;
        k8_flush(L, out, cap, outdw, pos, lane, false);
    }
}

// The dynamic block behind BFINAL / BTYPE in the form the kernel chose: header, tokens, end of block.
template <bool MATCHES, class Seq>
RFX_DEV void k8_block(K8LdsFor<MATCHES> &L, const Seq &S, const K8Forms &F, bool form_c, unsigned *out, unsigned cap, unsigned &outdw, unsigned &pos, int lane) {
    K8Lds &B = k8_base(L);
    const bool w = lane == 0;
    const unsigned *code = B.code;
    int nlit = K8_NSYM, hclen = F.ahclen;
    if constexpr (MATCHES) {
        if (form_c) { code = L.mcode; nlit = F.nlit; hclen = F.chclen; }
        else if (F.nmatch) k8_header(B, B.code, K8_NSYM, 0u, lane, hclen);  // (the tokens in LDS were form (c)'s)
    }
    k8_put_header(B, pos, nlit, hclen, w);
    for (int j = 0; j < k8_first<MATCHES, Seq>(); j++) {  // the lead bytes' codes go out with the header
        const unsigned c = code[S.at(j)];
        k8_put(B, pos, c & 0xffffu, (int)(c >> 16), w);
    }
    k8_flush(B, out, cap, outdw, pos, lane, false);
    k8_emit<MATCHES>(B, S, code, form_c, out, cap, outdw, pos, lane);
    const unsigned ce = code[256];
    k8_put(B, pos, ce & 0xffffu, (int)(ce >> 16), w);
}

}  // namespace
