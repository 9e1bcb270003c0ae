// k8_png.h — K8: the PNG fragment of include/rfx.h "PNG fragments", encoded on the device from K7's staged U8 stream.  Included by
// k7_export.hip (one translation unit with K7).  All of it is integer arithmetic: the fragment is a pure function of the input bytes.  The
// deflate coder is k8_coder.h's; here are the pre-transform (the filter stage and the scanline's byte sequence), the chunk around the coder's
// block and the fragment around the chunks.
//
//   k8_png_rows<MATCHES>  one wave (a workgroup of 64 lanes) per scanline: filter choice, histogram(s), code lengths, the forms' sizes, then
//                         the smallest form — the dynamic block of literals (a), stored blocks (b) or, with MATCHES, the dynamic block with
//                         run-length matches (c) — into the scanline's slot of a scratch buffer (a whole chunk: length, "IDAT", payload,
//                         CRC-32), Adler partial sums.  <false> is the kernel of the calls without flags; a chunk without a match is
//                         byte-identical from both
//   k8_png_scan           one wave: exclusive scan of the chunk sizes, the tile's Adler-32 from the partial sums, the count of match-form
//                         chunks, the 32-byte result header
//   k8_png_gather         one workgroup per chunk: slot -> its place in the contiguous fragment (the EXR fragment's gather too)
#pragma once
#include "k8_coder.h"

namespace {

constexpr unsigned K8_CRC_POLY = 0xedb88320u;
constexpr unsigned K8_CRC_IDAT = 0x35af061eu;  // CRC-32 of "IDAT"
// x^(2^k) mod the CRC-32 polynomial, bit-reflected: a CRC moved past 2^k zero bits is its product with entry k
__constant__ unsigned k8_x2n[32] = {
    0x40000000u, 0x20000000u, 0x08000000u, 0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u, 0xed627daeu, 0x88d14467u, 0xd7bbfe6au,
    0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u, 0x09fe548fu, 0x83852d0fu, 0x30362f1au, 0x7b5a9cc3u, 0x31fec169u, 0x9fec022au, 0x6c8dedc4u,
    0x15d6874du, 0x5fde7a4eu, 0xbad90e37u, 0x2e4e5eefu, 0x4eaba214u, 0xa8a472c0u, 0x429a969eu, 0x148d302au, 0xc40ba6d0u, 0xc4e22c3cu};

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
// the scanline's byte sequence for the coder: the type byte, then the residuals
struct K8PngSeq {
    static constexpr int LEAD = 1;  // the type byte: a literal step is 256 residuals
    const unsigned char *cur, *up;
    int bpp, type, n;
    RFX_DEV unsigned at(int j) const {
        if (j < 0 || j >= n) return K8_NONE;
        if (j == 0) return (unsigned)type;
        int x, a, b, c;
        k8_fetch(cur, up, bpp, j - 1, x, a, b, c);
        return k8_residual(type, x, a, b, c);
    }
    RFX_DEV int load4(int j0, unsigned d[4]) const {
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            d[k] = K8_NONE;
            if (j0 + k < n) {
                d[k] = at(j0 + k);
                cnt = k + 1;
            }
        }
        return cnt;
    }
};

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

template <bool MATCHES>
__global__ __launch_bounds__(64) void k8_png_rows(K8Args A) {
    __shared__ K8LdsFor<MATCHES> L;
    K8Lds &B = k8_base(L);
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

    // histogram(s) of the filtered bytes (the type byte is one of them) and their Adler partial sums
    k8_clear(L, lane);
    for (int i = lane; i < 256; i += 64) {
        unsigned c = (unsigned)i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ K8_CRC_POLY : c >> 1;
        B.crc_table[i] = c;
    }
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    const int nmatch = k8_histogram<MATCHES>(L, S, lane, s1, s2);
    const unsigned ad1 = (unsigned)k8_wave_sum((int)(s1 % K8_ADLER)) % K8_ADLER;
    const unsigned ad2 = (unsigned)k8_wave_sum((int)(s2 % K8_ADLER)) % K8_ADLER;
    __syncthreads();

    // the forms' sizes: a dynamic block is followed by the empty stored block
    const K8Forms F = k8_sizes<MATCHES>(L, nmatch, lane);
    const unsigned nblk = ((unsigned)n + 65534u) / 65535u;
    const unsigned stored_bytes = (unsigned)n + 5u * nblk;
    const unsigned a_bytes = (3u + F.abits + 3u + 7u) / 8u + 4u, c_bytes = (3u + F.cbits + 3u + 7u) / 8u + 4u;
    const bool form_c = MATCHES && nmatch && c_bytes < min(a_bytes, stored_bytes);
    unsigned plen;

    if (form_c || a_bytes <= stored_bytes) {
        // (c) or (a): the block header, the tokens, end of block and the empty stored block
        unsigned pos = 0, outdw = 0;
        const bool w = lane == 0;
        k8_put(B, pos, 4u, 3, w);  // BFINAL 0, BTYPE 2
        k8_block<MATCHES>(L, S, F, form_c, out, cap, outdw, pos, lane);
        k8_put(B, pos, 0u, 3, w);  // BFINAL 0, BTYPE 0
        pos = (pos + 7u) & ~7u;
        k8_put(B, pos, 0x0000u, 16, w);
        k8_put(B, pos, 0xffffu, 16, w);
        plen = min(outdw * 4u + pos / 8u, stored_bytes);  // (= c_bytes or a_bytes: the sizes above are the emission's)
        k8_flush(B, out, cap, outdw, pos, lane, true);
    } else {
        // (b) stored blocks of at most 65535 filtered bytes: 00, LEN, ~LEN, the bytes
        unsigned char *p = slot + 8;
        for (unsigned k = (unsigned)lane; k < nblk; k += 64u) {
            const unsigned len = min(65535u, (unsigned)n - k * 65535u), at = k * 65540u;
            p[at] = 0;
            p[at + 1] = (unsigned char)(len & 255u); p[at + 2] = (unsigned char)(len >> 8);
            p[at + 3] = (unsigned char)(~len & 255u); p[at + 4] = (unsigned char)((~len >> 8) & 255u);
        }
        constexpr int first = k8_first<MATCHES, K8PngSeq>();  // (the type byte beside the sweep or in it, as in the coder's)
        if (first && lane == 0) p[5] = (unsigned char)S.type;
        for (int base = first; base < n; base += 256) {
            unsigned d[4];
            const int cnt = S.load4(base + lane * 4, d);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (k < cnt) {
                    const unsigned q = (unsigned)(base + lane * 4 + k);
                    p[q + 5u * (q / 65535u + 1u)] = (unsigned char)d[k];
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
            for (unsigned i = b0; i < b1; i++) crc = B.crc_table[(crc ^ p[i]) & 255u] ^ (crc >> 8);
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

// chunk sizes -> chunk offsets; the Adler-32 (initial value 1) of the tile's rows * n filtered bytes from the scanlines' partial sums:
// A = 1 + sum s1,  B = N + sum over scanlines of (s2 + bytes behind the scanline * s1); the result header
__global__ __launch_bounds__(64) void k8_png_scan(K8Args A) {
    const int lane = (int)threadIdx.x;
    const unsigned long long n = (unsigned long long)A.rowbytes + 1ull;
    unsigned long long running = 0, a = 0, b = 0;
    int matched = 0;  // chunks in the match form; none from k8_png_rows<false>
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

// what the gather reads of either fragment kind's arguments
struct K8GatherArgs {
    unsigned char *result;
    const unsigned char *slots;
    const unsigned *meta;
    const unsigned long long *offsets;
    unsigned long long fragment_cap;
    int rows;
    unsigned slot_stride;
};
template <class Args>
K8GatherArgs k8_gather_args(const Args &A) { return {A.result, A.slots, A.meta, A.offsets, A.fragment_cap, A.rows, A.slot_stride}; }

__global__ __launch_bounds__(256) void k8_png_gather(K8GatherArgs A) {
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
    if (matches) hipLaunchKernelGGL(k8_png_rows<true>, dim3(A.rows), dim3(64), 0, stream, A);
    else hipLaunchKernelGGL(k8_png_rows<false>, dim3(A.rows), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k8_png_scan, dim3(1), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k8_png_gather, dim3(A.rows), dim3(256), 0, stream, k8_gather_args(A));
    return hipGetLastError();
}
