// k8_exr.h — K8's second pre-transform: the EXR fragment of include/rfx.h "EXR fragments" (ZIPS chunks, one per scanline), encoded on the device
// from K7's staged F16 stream.  Included by k7_export.hip behind k8_png.h, whose coder it shares unchanged: k8_build_code, the header tokens,
// the bit window, the wave helpers, k8_png_gather.  All of it is integer arithmetic: the fragment is a pure function of the staged halfs.
//
//   k8_exr_planes  one lane per pixel: K7's pixel-interleaved halfs -> the scanline's `t` bytes (every channel's low bytes in alphabetical
//                  channel order, then every channel's high bytes) in a scratch plane; reads and the byte-plane stores are coalesced
//   k8_exr_rows    one wave per scanline: the predicted bytes d (each t byte's difference to its predecessor + 128), histogram, the Adler-32's
//                  partial sums, code lengths, block header, bit packing into the scanline's slot — a whole chunk: y, size, data — or, when the
//                  zlib stream would not be smaller than the raw block, the raw block
//   k8_exr_scan    one wave: exclusive scan of the chunk sizes, the counts of raw and of match-form chunks, the 32-byte result header
//   k8_png_gather  slot -> its place in the contiguous fragment (k8_png.h)
//
// The zlib stream goes through the bit window whole: its two header bytes are the window's first 16 bits, the Adler-32 its last 32.
#pragma once
#include "k8_png.h"

namespace {

// the t bytes [i0, i0 + 4) of a scanline's plane (i0 a multiple of 4; the plane is dword-aligned and padded to whole dwords) as predicted
// bytes: d[0] = t[0], d[i] = t[i] - t[i - 1] + 128.  Returns how many lie inside the scanline.
RFX_DEV int k8_exr_predict4(const unsigned char *t, int n, int i0, unsigned res[4]) {
    res[0] = res[1] = res[2] = res[3] = 0;
    if (i0 >= n) return 0;
    const unsigned w = *(const unsigned *)(t + i0);
    unsigned prev = i0 ? (unsigned)t[i0 - 1] : 128u;  // (128: d[0] = t[0] - 128 + 128)
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (i0 + k < n) {
            const unsigned b = (w >> (8 * k)) & 255u;
            res[k] = (b - prev + 128u) & 255u;
            prev = b;
            cnt = k + 1;
        }
    }
    return cnt;
}

__global__ __launch_bounds__(256) void k8_exr_planes(K8ExrArgs A) {
    const int x = (int)(blockIdx.x * 256u + threadIdx.x);
    const int s = (int)blockIdx.y;  // scanline of the tile, 0 = top = stream row rows - 1
    if (x >= A.width) return;
    const int ch = A.channels, m = A.width * ch;
    const unsigned short *px = A.src + ((size_t)(A.rows - 1 - s) * (size_t)A.width + (size_t)x) * (size_t)ch;
    unsigned char *t = A.planes + (size_t)s * A.plane_stride;
    for (int c = 0; c < ch; c++) {  // alphabetical: (A) B G R = the stream's channels backwards
        const unsigned h = px[ch - 1 - c];
        t[c * A.width + x] = (unsigned char)(h & 255u);
        t[m + c * A.width + x] = (unsigned char)(h >> 8);
    }
}

__global__ __launch_bounds__(64) void k8_exr_rows(K8ExrArgs A) {
    __shared__ K8Lds L;
    const int lane = (int)threadIdx.x;
    const int s = (int)blockIdx.x;
    const int n = 2 * A.width * A.channels;
    const unsigned char *t = A.planes + (size_t)s * A.plane_stride;
    unsigned char *slot = A.slots + (size_t)s * A.slot_stride;
    unsigned *out = (unsigned *)(slot + 8);
    const unsigned cap = (A.slot_stride - 8u) / 4u;

    // histogram of the predicted bytes and the Adler partial sums: sum of bytes, sum of (n - position) * byte
    for (int i = lane; i < K8_TABLE; i += 64) L.freq[i] = 0;
    for (int i = lane; i < K8_WIN; i += 64) L.win[i] = 0;
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    if (lane == 0) L.freq[256] = 1;
    for (int base = 0; base < n; base += 256) {
        const int i0 = base + lane * 4;
        unsigned res[4];
        const int cnt = k8_exr_predict4(t, n, i0, res);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < cnt) {
                atomicAdd(&L.freq[res[k]], 1u);
                s1 += res[k];
                s2 += (unsigned long long)(n - (i0 + k)) * res[k];
            }
        }
    }
    const unsigned ad1 = (1u + (unsigned)k8_wave_sum((int)(s1 % K8_ADLER))) % K8_ADLER;
    const unsigned ad2 = ((unsigned)(n % (int)K8_ADLER) + (unsigned)k8_wave_sum((int)(s2 % K8_ADLER))) % K8_ADLER;
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

    // the zlib stream's size
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
    const unsigned comp_bytes = 2u + (dynbits + 7u) / 8u + 4u;
    unsigned size;

    if (comp_bytes < (unsigned)n) {
        // (a) 78 01, the FINAL dynamic block: header, literals, end of block; padding to a byte; the Adler-32, big-endian
        unsigned pos = 0, outdw = 0;
        const bool w = lane == 0;
        k8_put(L, pos, 0x0178u, 16, w);
        k8_put(L, pos, 5u, 3, w);  // BFINAL 1, BTYPE 2
        k8_put(L, pos, 0u, 5, w);  // HLIT: 257 codes
        k8_put(L, pos, 0u, 5, w);  // HDIST: 1 code
        k8_put(L, pos, (unsigned)(hclen - 4), 4, w);
        for (int i = 0; i < hclen; i++) k8_put(L, pos, L.clcode[k8_cl_order[i]] >> 16, 3, w);
        for (int i = 0; i < ntokens; i++) {
            const unsigned tk = L.tokens[i], sym = tk & 255u, c = L.clcode[sym];
            k8_put(L, pos, c & 0xffffu, (int)(c >> 16), w);
            k8_put(L, pos, tk >> 8, sym == 16u ? 2 : sym == 17u ? 3 : sym == 18u ? 7 : 0, w);
        }
        k8_flush(L, out, cap, outdw, pos, lane, false);
        for (int base = 0; base < n; base += 256) {
            unsigned res[4];
            const int cnt = k8_exr_predict4(t, n, base + lane * 4, res);
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
        pos = (pos + 7u) & ~7u;
        k8_put(L, pos, ((ad2 >> 8) & 255u) | ((ad2 & 255u) << 8), 16, w);
        k8_put(L, pos, ((ad1 >> 8) & 255u) | ((ad1 & 255u) << 8), 16, w);
        size = outdw * 4u + pos / 8u;  // (= comp_bytes: the size above is the emission's)
        k8_flush(L, out, cap, outdw, pos, lane, true);
    } else {
        // (b) the raw block: half j of the scanline is t[j] | t[n / 2 + j] << 8
        unsigned short *p = (unsigned short *)(slot + 8);
        const int m = n / 2;
        for (int j = lane; j < m; j += 64) p[j] = (unsigned short)((unsigned)t[j] | ((unsigned)t[m + j] << 8));
        size = (unsigned)n;
    }
    if (lane == 0) {
        ((int *)slot)[0] = A.first_y + s;
        ((unsigned *)slot)[1] = size;
        unsigned *mt = A.meta + 4 * (size_t)s;
        mt[0] = size + 8u; mt[1] = size == (unsigned)n ? 1u : 0u; mt[2] = 0; mt[3] = 0;
    }
}

// chunk sizes -> chunk offsets; the result header
__global__ __launch_bounds__(64) void k8_exr_scan(K8ExrArgs A) {
    const int lane = (int)threadIdx.x;
    unsigned long long running = 0;
    int raw = 0, matched = 0;
    for (int base = 0; base < A.rows; base += 64) {
        const int s = base + lane;
        int len = 0;
        if (s < A.rows) {
            const unsigned *m = A.meta + 4 * (size_t)s;
            len = (int)m[0];
            raw += (int)m[1];
            matched += (int)m[2];  // chunks in the match form (k8_match.h); none from k8_exr_rows
        }
        int total;
        const int off = k8_wave_scan(len, lane, total);
        if (s < A.rows) A.offsets[s] = running + (unsigned long long)off;
        running += (unsigned long long)total;
    }
    raw = k8_wave_sum(raw);
    matched = k8_wave_sum(matched);
    if (lane == 0) {
        const unsigned long long N = (unsigned long long)A.rows * (unsigned long long)(2 * A.width * A.channels);
        unsigned *h = (unsigned *)A.result;
        h[0] = (unsigned)running; h[1] = (unsigned)(running >> 32);
        h[2] = (unsigned)A.rows;
        h[3] = (unsigned)A.first_y;
        h[4] = (unsigned)N; h[5] = (unsigned)(N >> 32);
        h[6] = (unsigned)raw; h[7] = (unsigned)matched;
    }
}

}  // namespace

hipError_t rfx_launch_k8_exr(const K8ExrArgs &A, hipStream_t stream, bool matches) {
    if (A.rows <= 0 || A.rows > 65535 || A.width <= 0 || (A.channels != 3 && A.channels != 4)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k8_exr_planes, dim3((A.width + 255) / 256, A.rows), dim3(256), 0, stream, A);
    if (matches) {
        const hipError_t e = rfx_launch_k8_exr_rows_m(A, stream);  // k8_match.h
        if (e != hipSuccess) return e;
    } else hipLaunchKernelGGL(k8_exr_rows, dim3(A.rows), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k8_exr_scan, dim3(1), dim3(64), 0, stream, A);
    K8Args G = {};  // the gather reads the chunk sizes, the offsets and the slots only
    G.result = A.result; G.slots = A.slots; G.meta = A.meta; G.offsets = A.offsets;
    G.fragment_cap = A.fragment_cap; G.rows = A.rows; G.slot_stride = A.slot_stride;
    hipLaunchKernelGGL(k8_png_gather, dim3(A.rows), dim3(256), 0, stream, G);
    return hipGetLastError();
}
