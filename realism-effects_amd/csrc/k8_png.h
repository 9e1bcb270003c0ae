// k8_png.h — K8: the PNG fragment of include/rfx.h "PNG fragments", encoded on the device from K7's staged U8 stream.  Included by
// k7_export.hip (one translation unit with K7).  All of it is integer arithmetic: the fragment is a pure function of the input bytes.
//
//   k8_png_rows    one wave (a workgroup of 64 lanes) per scanline: filter choice, histogram, code lengths, block header, bit packing into
//                  the scanline's slot of a scratch buffer (a whole chunk: length, "IDAT", payload, CRC-32), Adler partial sums
//   k8_png_scan    one wave: exclusive scan of the chunk sizes, the tile's Adler-32 from the partial sums, the count of match-form chunks,
//                  the 32-byte result header
//   k8_png_gather  one workgroup per chunk: slot -> its place in the contiguous fragment
//
// The row is never staged in LDS (a 32768 x 4 row is 131 073 bytes): it is read three times — costs, histogram, codes — from L2, where K7
// just put it.  Bits are assembled in a 512-byte LDS window with atomicOr (64 lanes x 4 symbols x at most 15 bits per step, plus the bits
// carried over from the step before) and leave it as whole dwords.  Wave operations: __shfl / __shfl_xor only.
#pragma once
#include "rfx_device.h"
#include "rfx_kernels.h"

namespace {

constexpr int K8_NSYM = 257, K8_NCL = 19, K8_MAXBITS = 15, K8_CL_MAXBITS = 7;
constexpr int K8_TABLE = 288;        // a code's tables: 257 symbols rounded up
constexpr int K8_WIN = 128;          // the bit window, dwords: 31 carried bits + 256 x 15 = 3871 bits at most; the block header is below 2000
constexpr unsigned K8_ADLER = 65521u;
constexpr unsigned K8_CRC_POLY = 0xedb88320u;
constexpr unsigned K8_CRC_IDAT = 0x35af061eu;  // CRC-32 of "IDAT"
// x^(2^k) mod the CRC-32 polynomial, bit-reflected: a CRC moved past 2^k zero bits is its product with entry k
__constant__ unsigned k8_x2n[32] = {
    0x40000000u, 0x20000000u, 0x08000000u, 0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u, 0xed627daeu, 0x88d14467u, 0xd7bbfe6au,
    0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u, 0x09fe548fu, 0x83852d0fu, 0x30362f1au, 0x7b5a9cc3u, 0x31fec169u, 0x9fec022au, 0x6c8dedc4u,
    0x15d6874du, 0x5fde7a4eu, 0xbad90e37u, 0x2e4e5eefu, 0x4eaba214u, 0xa8a472c0u, 0x429a969eu, 0x148d302au, 0xc40ba6d0u, 0xc4e22c3cu};
__constant__ int k8_cl_order[K8_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct K8Lds {
    unsigned freq[K8_TABLE];           // the scanline's histogram: 256 literals and the end-of-block symbol
    unsigned code[K8_TABLE];           // bit-reversed canonical code | length << 16
    unsigned work[K8_TABLE];           // Moffat-Katajainen's array
    unsigned short sorted[K8_TABLE];   // used symbols by rank: frequency descending, symbol ascending
    unsigned short tokens[K8_TABLE];   // the code-length sequence: symbol | extra value << 8
    unsigned clfreq[32], clcode[32];
    unsigned win[K8_WIN];
    unsigned crc_table[256];
    int count[K8_MAXBITS + 1];
    unsigned next_code[K8_MAXBITS + 1];
    int ntokens;
};

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

// ---------------------------------------------------------------- the filter stage (separate from the coder: another pre-transform can take its place)
RFX_DEV int k8_abs(int v) { return v < 0 ? -v : v; }
RFX_DEV int k8_paeth(int a, int b, int c) {
    const int pa = k8_abs(b - c), pb = k8_abs(a - c), pc = k8_abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// PNG filter type 0 None, 1 Sub, 2 Up, 4 Paeth
RFX_DEV unsigned k8_residual(int type, int x, int a, int b, int c) {
    const int p = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : k8_paeth(a, b, c);
    return (unsigned)(x - p) & 255u;
}
// byte i of the scanline and its neighbours: a left (bpp back), b above, c above left; 0 outside the row and above the tile's first scanline
RFX_DEV void k8_fetch(const unsigned char *cur, const unsigned char *up, int bpp, int i, int &x, int &a, int &b, int &c) {
    x = cur[i];
    a = i >= bpp ? cur[i - bpp] : 0;
    b = up ? up[i] : 0;
    c = (up && i >= bpp) ? up[i - bpp] : 0;
}
// the residuals of bytes [i0, i0 + 4) under `type`; returns how many lie inside the row
RFX_DEV int k8_filter4(const unsigned char *cur, const unsigned char *up, int rowbytes, int bpp, int type, int i0, unsigned res[4]) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        res[k] = 0;
        if (i0 + k < rowbytes) {
            int x, a, b, c;
            k8_fetch(cur, up, bpp, i0 + k, x, a, b, c);
            res[k] = k8_residual(type, x, a, b, c);
            n = k + 1;
        }
    }
    return n;
}
RFX_DEV int k8_cost(unsigned r) { return r < 128u ? (int)r : 256 - (int)r; }
// filter 0: the smallest sum of |residual as int8|, ties to the lowest type number, None / Sub only without an upper neighbour; 1..4 forced
RFX_DEV int k8_choose_filter(const unsigned char *cur, const unsigned char *up, int rowbytes, int bpp, int filter, int lane) {
    if (filter) {
        const int t = filter == 1 ? 0 : filter == 2 ? 1 : filter == 3 ? 2 : 4;
        return (!up && t >= 2) ? 1 : t;
    }
    int c0 = 0, c1 = 0, c2 = 0, c4 = 0;
    for (int base = 0; base < rowbytes; base += 256) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = base + lane * 4 + k;
            if (i < rowbytes) {
                int x, a, b, c;
                k8_fetch(cur, up, bpp, i, x, a, b, c);
                c0 += k8_cost(k8_residual(0, x, a, b, c));
                c1 += k8_cost(k8_residual(1, x, a, b, c));
                c2 += k8_cost(k8_residual(2, x, a, b, c));
                c4 += k8_cost(k8_residual(4, x, a, b, c));
            }
        }
    }
    c0 = k8_wave_sum(c0); c1 = k8_wave_sum(c1); c2 = k8_wave_sum(c2); c4 = k8_wave_sum(c4);
    int best = 0, cost = c0;
    if (c1 < cost) { best = 1; cost = c1; }
    if (up && c2 < cost) { best = 2; cost = c2; }
    if (up && c4 < cost) { best = 4; cost = c4; }
    return best;
}

// ---------------------------------------------------------------- the code-length rule of rfx.h, and the canonical codes
// freq[0, n) -> code[0, n) (bit-reversed code | length << 16; 0 for an unused symbol).  The ranking is spread over the lanes; the tree, the
// length limit and the code assignment are one lane's serial pass.  Ends with a barrier.
RFX_DEV void k8_build_code(K8Lds &L, const unsigned *freq, int n, int maxbits, unsigned *code, int lane) {
    for (int s = lane; s < n; s += 64) {
        const unsigned f = freq[s];
        if (f) {
            int r = 0;
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

// ---------------------------------------------------------------- CRC-32 over GF(2)
RFX_DEV unsigned k8_crc_mul(unsigned a, unsigned b) {  // a * b mod the polynomial (reflected)
    unsigned p = 0;
    for (unsigned m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ K8_CRC_POLY : b >> 1;
    }
    return p;
}
// the CRC-32 of X followed by `bytes` more bytes = k8_crc_shift(crc(X), bytes) ^ crc(those bytes)
RFX_DEV unsigned k8_crc_shift(unsigned crc, unsigned bytes) {
    unsigned p = 1u << 31;
    for (int k = 3; bytes; bytes >>= 1, k++)
        if (bytes & 1u) p = k8_crc_mul(k8_x2n[k & 31], p);
    return k8_crc_mul(p, crc);
}

__global__ __launch_bounds__(64) void k8_png_rows(K8Args A) {
    __shared__ K8Lds L;
    const int lane = (int)threadIdx.x;
    const int s = (int)blockIdx.x;  // PNG scanline of the tile, 0 = top = stream row rows - 1
    const int rowbytes = A.rowbytes, bpp = A.bpp, n = rowbytes + 1;
    const unsigned char *cur = A.src + (size_t)(A.rows - 1 - s) * (size_t)rowbytes;
    const unsigned char *up = s ? cur + rowbytes : nullptr;
    unsigned char *slot = A.slots + (size_t)s * A.slot_stride;
    unsigned *out = (unsigned *)(slot + 8);
    const unsigned cap = (A.slot_stride - 8u) / 4u;

    const int type = k8_choose_filter(cur, up, rowbytes, bpp, A.filter, lane);

    // histogram of the filtered bytes (the type byte is one of them) and their Adler partial sums: sum of bytes, sum of (n - position) * byte
    for (int i = lane; i < K8_TABLE; i += 64) L.freq[i] = 0;
    for (int i = lane; i < K8_WIN; i += 64) L.win[i] = 0;
    for (int i = lane; i < 256; i += 64) {
        unsigned c = (unsigned)i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ K8_CRC_POLY : c >> 1;
        L.crc_table[i] = c;
    }
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    if (lane == 0) {
        atomicAdd(&L.freq[type], 1u);
        L.freq[256] = 1;
        s1 = (unsigned long long)type;
        s2 = (unsigned long long)n * (unsigned long long)type;
    }
    for (int base = 0; base < rowbytes; base += 256) {
        const int i0 = base + lane * 4;
        unsigned res[4];
        const int cnt = k8_filter4(cur, up, rowbytes, bpp, type, i0, res);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < cnt) {
                atomicAdd(&L.freq[res[k]], 1u);
                s1 += res[k];
                s2 += (unsigned long long)(n - (1 + i0 + k)) * res[k];
            }
        }
    }
    const unsigned ad1 = (unsigned)k8_wave_sum((int)(s1 % K8_ADLER)) % K8_ADLER;
    const unsigned ad2 = (unsigned)k8_wave_sum((int)(s2 % K8_ADLER)) % K8_ADLER;
    __syncthreads();

    k8_build_code(L, L.freq, K8_NSYM, K8_MAXBITS, L.code, lane);

    // the code-length sequence (257 literal / length codes and one unused distance code) as run-length tokens, and their histogram
    if (lane == 0) {
        for (int i = 0; i < 32; i++) L.clfreq[i] = 0;
        int nt = 0, i = 0;
        const int total = K8_NSYM + 1;
        while (i < total) {
            const unsigned v = i < K8_NSYM ? L.code[i] >> 16 : 0u;
            int j = i;
            while (j < total && (j < K8_NSYM ? L.code[j] >> 16 : 0u) == v) j++;
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

    // the two forms' sizes
    const int ntokens = L.ntokens;
    int hclen = 4;
    for (int i = 0; i < K8_NCL; i++)
        if (L.clcode[k8_cl_order[i]] >> 16) hclen = max(hclen, i + 1);
    unsigned dynbits = 3u + 5u + 5u + 4u + 3u * (unsigned)hclen;
    for (int i = 0; i < ntokens; i++) {
        const int sym = L.tokens[i] & 255;
        dynbits += (L.clcode[sym] >> 16) + (sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u);
    }
    int litbits = 0;
    for (int i = lane; i < K8_NSYM; i += 64) litbits += (int)(L.freq[i] * (L.code[i] >> 16));
    dynbits += (unsigned)k8_wave_sum(litbits);
    const unsigned nblk = ((unsigned)n + 65534u) / 65535u;
    const unsigned stored_bytes = (unsigned)n + 5u * nblk;
    const unsigned comp_bytes = (dynbits + 3u + 7u) / 8u + 4u;
    unsigned plen;

    if (comp_bytes <= stored_bytes) {
        // (a) the block header, then the literals, then end of block and the empty stored block
        unsigned pos = 0, outdw = 0;
        const bool w = lane == 0;
        k8_put(L, pos, 4u, 3, w);  // BFINAL 0, BTYPE 2
        k8_put(L, pos, 0u, 5, w);  // HLIT: 257 codes
        k8_put(L, pos, 0u, 5, w);  // HDIST: 1 code
        k8_put(L, pos, (unsigned)(hclen - 4), 4, w);
        for (int i = 0; i < hclen; i++) k8_put(L, pos, L.clcode[k8_cl_order[i]] >> 16, 3, w);
        for (int i = 0; i < ntokens; i++) {
            const unsigned t = L.tokens[i], sym = t & 255u, c = L.clcode[sym];
            k8_put(L, pos, c & 0xffffu, (int)(c >> 16), w);
            k8_put(L, pos, t >> 8, sym == 16u ? 2 : sym == 17u ? 3 : sym == 18u ? 7 : 0, w);
        }
        const unsigned ct = L.code[type];
        k8_put(L, pos, ct & 0xffffu, (int)(ct >> 16), w);
        k8_flush(L, out, cap, outdw, pos, lane, false);
        for (int base = 0; base < rowbytes; base += 256) {
            unsigned res[4];
            const int cnt = k8_filter4(cur, up, rowbytes, bpp, type, base + lane * 4, res);
            unsigned long long acc = 0;
            int nb = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (k < cnt) {
                    const unsigned c = L.code[res[k]];
                    acc |= (unsigned long long)(c & 0xffffu) << nb;
                    nb += (int)(c >> 16);
                }
            }
            int total;
            const unsigned o = pos + (unsigned)k8_wave_scan(nb, lane, total);
            if (nb) {
                const unsigned wi = o >> 5, sh = o & 31u;
                const unsigned long long lo = acc << sh;
                const unsigned w0 = (unsigned)lo, w1 = (unsigned)(lo >> 32), w2 = sh ? (unsigned)(acc >> (64u - sh)) : 0u;
                if (w0) atomicOr(&L.win[wi], w0);
                if (w1) atomicOr(&L.win[wi + 1], w1);
                if (w2) atomicOr(&L.win[wi + 2], w2);
            }
            pos += (unsigned)total;
            k8_flush(L, out, cap, outdw, pos, lane, false);
        }
        const unsigned ce = L.code[256];
        k8_put(L, pos, ce & 0xffffu, (int)(ce >> 16), w);
        k8_put(L, pos, 0u, 3, w);  // BFINAL 0, BTYPE 0
        pos = (pos + 7u) & ~7u;
        k8_put(L, pos, 0x0000u, 16, w);
        k8_put(L, pos, 0xffffu, 16, w);
        plen = min(outdw * 4u + pos / 8u, stored_bytes);  // (= comp_bytes: the sizes above are the emission's)
        k8_flush(L, out, cap, outdw, pos, lane, true);
    } else {
        // (b) stored blocks of at most 65535 filtered bytes: 00, LEN, ~LEN, the bytes
        unsigned char *p = slot + 8;
        for (unsigned k = (unsigned)lane; k < nblk; k += 64u) {
            const unsigned len = min(65535u, (unsigned)n - k * 65535u), at = k * 65540u;
            p[at] = 0;
            p[at + 1] = (unsigned char)(len & 255u); p[at + 2] = (unsigned char)(len >> 8);
            p[at + 3] = (unsigned char)(~len & 255u); p[at + 4] = (unsigned char)((~len >> 8) & 255u);
        }
        if (lane == 0) p[5] = (unsigned char)type;
        for (int base = 0; base < rowbytes; base += 256) {
            const int i0 = base + lane * 4;
            unsigned res[4];
            const int cnt = k8_filter4(cur, up, rowbytes, bpp, type, i0, res);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (k < cnt) {
                    const unsigned q = 1u + (unsigned)(i0 + k);
                    p[q + 5u * (q / 65535u + 1u)] = (unsigned char)res[k];
                }
            }
        }
        plen = stored_bytes;
        __syncthreads();
    }

    // the chunk's CRC-32: each lane takes a run of the payload as it now stands in memory, moves its CRC past the bytes behind it; XOR joins them
    {
        const unsigned char *p = slot + 8;
        const unsigned seg = (plen + 63u) / 64u;
        const unsigned b0 = min(plen, (unsigned)lane * seg), b1 = min(plen, b0 + seg);
        unsigned crc = 0;
        if (b1 > b0) {
            crc = 0xffffffffu;
            for (unsigned i = b0; i < b1; i++) crc = L.crc_table[(crc ^ p[i]) & 255u] ^ (crc >> 8);
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
            m[0] = plen + 12u; m[1] = ad1; m[2] = ad2; m[3] = 0;
        }
    }
}

// chunk sizes -> chunk offsets; the Adler-32 (initial value 1) of the tile's rows * n filtered bytes from the scanlines' partial sums:
// A = 1 + sum s1,  B = N + sum over scanlines of (s2 + bytes behind the scanline * s1); the result header
__global__ __launch_bounds__(64) void k8_png_scan(K8Args A) {
    const int lane = (int)threadIdx.x;
    const unsigned long long n = (unsigned long long)A.rowbytes + 1ull;
    unsigned long long running = 0, a = 0, b = 0;
    int matched = 0;  // chunks in the match form (k8_match.h); none from k8_png_rows
    for (int base = 0; base < A.rows; base += 64) {
        const int s = base + lane;
        int len = 0;
        if (s < A.rows) {
            const unsigned *m = A.meta + 4 * (size_t)s;
            len = (int)m[0];
            matched += (int)m[3];
            a += m[1];
            b += m[2] + ((unsigned long long)(A.rows - 1 - s) * n) % K8_ADLER * m[1];
        }
        int total;
        const int off = k8_wave_scan(len, lane, total);
        if (s < A.rows) A.offsets[s] = running + (unsigned long long)off;
        running += (unsigned long long)total;
    }
    const unsigned long long N = (unsigned long long)A.rows * n;
    const unsigned sa = (unsigned)k8_wave_sum((int)(a % K8_ADLER)), sb = (unsigned)k8_wave_sum((int)(b % K8_ADLER));
    matched = k8_wave_sum(matched);
    if (lane == 0) {
        unsigned *h = (unsigned *)A.result;
        h[0] = (unsigned)running; h[1] = (unsigned)(running >> 32);
        h[2] = (1u + sa) % K8_ADLER;
        h[3] = (unsigned)((N + sb) % K8_ADLER);
        h[4] = (unsigned)N; h[5] = (unsigned)(N >> 32);
        h[6] = (unsigned)matched; h[7] = 0;
    }
}

__global__ __launch_bounds__(256) void k8_png_gather(K8Args A) {
    const int s = (int)blockIdx.x;
    const unsigned len = A.meta[4 * (size_t)s];
    const unsigned long long off = A.offsets[s];
    if (off + len > A.fragment_cap) return;  // (cannot happen: every chunk is at most its stored form)
    const unsigned char *src = A.slots + (size_t)s * A.slot_stride;
    unsigned char *dst = A.result + 32 + off;
    for (unsigned i = threadIdx.x; i < len; i += 256u) dst[i] = src[i];
}

}  // namespace

hipError_t rfx_launch_k8(const K8Args &A, hipStream_t stream, bool matches) {
    if (A.rows <= 0 || A.rowbytes <= 0 || (A.bpp != 3 && A.bpp != 4) || A.filter < 0 || A.filter > 4) return hipErrorInvalidValue;
    if (matches) {
        const hipError_t e = rfx_launch_k8_rows_m(A, stream);  // k8_match.h
        if (e != hipSuccess) return e;
    } else hipLaunchKernelGGL(k8_png_rows, dim3(A.rows), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k8_png_scan, dim3(1), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k8_png_gather, dim3(A.rows), dim3(256), 0, stream, A);
    return hipGetLastError();
}
