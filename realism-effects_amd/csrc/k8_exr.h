// k8_exr.h — K8's second pre-transform: the EXR fragment of include/rfx.h "EXR fragments" (ZIPS chunks, one per scanline), encoded on the device
// from K7's staged F16 stream.  Included by k7_export.hip behind k8_png.h: the coder is k8_coder.h's, the gather k8_png.h's.  All of it is
// integer arithmetic: the fragment is a pure function of the staged halfs.
//
//   k8_exr_planes         one lane per pixel: K7's pixel-interleaved halfs -> the scanline's `t` bytes (every channel's low bytes in
//                         alphabetical channel order, then every channel's high bytes) in a scratch plane; reads and the byte-plane stores
//                         are coalesced
//   k8_exr_rows<MATCHES>  one wave per scanline: the predicted bytes d (each t byte's difference to its predecessor + 128), histogram(s), the
//                         Adler-32's partial sums, code lengths, the forms' sizes, then the smallest form into the scanline's slot — a whole
//                         chunk: y, size, data — the zlib stream of literals (a) or, with MATCHES, with run-length matches (c), or, when
//                         neither is smaller than the raw block, the raw block (b).  <false> is the kernel of the calls without flags
//   k8_exr_scan           one wave: exclusive scan of the chunk sizes, the counts of raw and of match-form chunks, the 32-byte result header
//   k8_png_gather         slot -> its place in the contiguous fragment (k8_png.h)
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
// the scanline's byte sequence for the coder: the predicted bytes of its plane
struct K8ExrSeq {
    static constexpr int LEAD = 0;
    const unsigned char *t;
    int n;
    RFX_DEV unsigned at(int j) const {
        if (j < 0 || j >= n) return K8_NONE;
        return j ? ((unsigned)t[j] - (unsigned)t[j - 1] + 128u) & 255u : (unsigned)t[0];
    }
    RFX_DEV int load4(int j0, unsigned d[4]) const {
        unsigned res[4];
        const int cnt = k8_exr_predict4(t, n, j0, res);
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = k < cnt ? res[k] : K8_NONE;
        return cnt;
    }
};

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

template <bool MATCHES>
__global__ __launch_bounds__(64) void k8_exr_rows(K8ExrArgs A) {
    __shared__ K8LdsFor<MATCHES> L;
    K8Lds &B = k8_base(L);
    const int lane = (int)threadIdx.x;
    const int s = (int)blockIdx.x;
    const int n = 2 * A.width * A.channels;
    unsigned char *slot = A.slots + (size_t)s * A.slot_stride;
    unsigned *out = (unsigned *)(slot + 8);
    const unsigned cap = (A.slot_stride - 8u) / 4u;
    K8ExrSeq S;
    S.t = A.planes + (size_t)s * A.plane_stride; S.n = n;

    // histogram(s) of the predicted bytes and the stream's Adler-32 (initial value 1) from the partial sums
    k8_clear(L, lane);
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    const int nmatch = k8_histogram<MATCHES>(L, S, lane, s1, s2);
    const unsigned ad1 = (1u + (unsigned)k8_wave_sum((int)(s1 % K8_ADLER))) % K8_ADLER;
    const unsigned ad2 = ((unsigned)(n % (int)K8_ADLER) + (unsigned)k8_wave_sum((int)(s2 % K8_ADLER))) % K8_ADLER;
    __syncthreads();

    // the zlib streams' sizes
    const K8Forms F = k8_sizes<MATCHES>(L, nmatch, lane);
    const unsigned a_bytes = 2u + (3u + F.abits + 7u) / 8u + 4u, c_bytes = 2u + (3u + F.cbits + 7u) / 8u + 4u;
    const bool form_c = MATCHES && nmatch && c_bytes < min(a_bytes, (unsigned)n);
    unsigned size;

    if (form_c || a_bytes < (unsigned)n) {
        // (c) or (a): 78 01, the FINAL dynamic block: header, tokens, end of block; padding to a byte; the Adler-32, big-endian
        unsigned pos = 0, outdw = 0;
        const bool w = lane == 0;
        k8_put(B, pos, 0x0178u, 16, w);
        k8_put(B, pos, 5u, 3, w);  // BFINAL 1, BTYPE 2
        k8_block<MATCHES>(L, S, F, form_c, out, cap, outdw, pos, lane);
        pos = (pos + 7u) & ~7u;
        k8_put(B, pos, ((ad2 >> 8) & 255u) | ((ad2 & 255u) << 8), 16, w);
        k8_put(B, pos, ((ad1 >> 8) & 255u) | ((ad1 & 255u) << 8), 16, w);
        size = outdw * 4u + pos / 8u;  // (= c_bytes or a_bytes: the sizes above are the emission's)
        k8_flush(B, out, cap, outdw, pos, lane, true);
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
            matched += (int)m[2];  // chunks in the match form; none from k8_exr_rows<false>
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
    if (matches) hipLaunchKernelGGL(k8_exr_rows<true>, dim3(A.rows), dim3(64), 0, stream, A);
    else hipLaunchKernelGGL(k8_exr_rows<false>, dim3(A.rows), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k8_exr_scan, dim3(1), dim3(64), 0, stream, A);
    hipLaunchKernelGGL(k8_png_gather, dim3(A.rows), dim3(256), 0, stream, k8_gather_args(A));
    return hipGetLastError();
}
