// K9 — EXR import: the chunks of an OpenEXR AOV file — scanline chunks or tiles —, as they sit in the file, -> the typed staging planes of
// rfx_stage_aov, on the device (include/rfx.h "streamed EXR frames", "EXR blocks").  The inverse of K8's EXR fragment (k8_exr.h) for any deflate stream a writer may produce.
//   k9_inflate     one wave per chunk.  The decoder is k9_inflate.h's, statement for statement the one the CPU tests run under the sanitizers;
//                  here its state (bit buffer, positions, symbols) is wave-uniform — every lane computes the same values — and the IO below spreads
//                  the memory work over the lanes: the input is read 256 bytes at a time, one dword per lane, and handed out by lane index; a literal
//                  is stored by the lane its position names, a match or a stored run by all lanes, 64 bytes per step.  The chunk's scratch slot in
//                  device memory is the output and the LZ77 window.  Decode tables: 3.5 KiB of LDS per wave (k9_inflate.h K9Tables), so LDS is not
//                  what limits residency: the kernel's 112 VGPRs are, at 4 waves per SIMD, 16 per CU.  The parallelism is the number of chunks.  A chunk whose packed size is its raw size is copied.
//                  ZIP, ZIPS and PXR24 streams alike (a PXR24 stream must inflate to 3 bytes per FLOAT sample: K9Chunk.expect); it returns at once
//                  for an RLE stream.
//   k9_rle         one wave per chunk, which returns at once for every chunk that is not an RLE stream: k9_rle.h's expander on the same IO — the
//                  walk over the count bytes is wave-uniform, a run or a literal (up to 128 bytes) is stored by all lanes.  What it leaves in the
//                  scratch slot is what the inflate leaves for ZIP: the predicted, split bytes.
//   k9_exr_planes  one block per chunk: t[i] = t[i-1] + d[i] - 128 is a byte prefix sum (4 KiB tiles, 16 bytes per thread, a block scan of the
//                  thread sums), in place; the even/odd byte split is undone while the samples are read; every mapped channel's row goes to its
//                  plane at (x + i, y + r) — a chunk is a rectangle of the frame, a scanline chunk one with x = 0, cols = W —, row 0 = bottom (EXR
//                  scanlines run top-down), halves widened where the plane is F32.  A PXR24 stream instead: one segmented scan per (row, channel)
//                  of the k-byte differences (k9_pxr24.h), the segments dealt to the block's four waves, 64 samples per step with a carry,
//                  written straight into the planes.
//   k9_piz_huf     one wave per PIZ chunk (launched when the band has one; every other chunk returns at once, as PIZ chunks do from k9_inflate): the
//                  reverse lookup table from the bitmap, the canonical Huffman tables and the decode of k9_piz.h on the same wave-wide input IO:
//                  the chunk's words, channel-planar, into its scratch slot.
//   k9_piz_planes  eight workgroups per PIZ chunk: the 2-D wavelet in cells of 64 x 64 words in LDS, the lookup, and k9_exr_planes' scatter — PIZ has
//                  no predictor and no byte split, so k9_exr_planes returns at once for a PIZ chunk that decoded.
//   k9_exr_finish  the rectangle of a chunk that did not decode: depth 1 (not covered), everything else 0 (written by k9_exr_planes); the status words.
// All integer work: nothing here depends on contraction.
#include "rfx_device.h"
#include "rfx_kernels.h"
#include "rfx_launch.h"

#define K9_FN RFX_DEV
#define K9_NO_HOST_IO
#include "k9_inflate.h"
#include "k9_rle.h"
#include "k9_pxr24.h"
#include "k9_piz.h"

namespace {

// what one lane stored becomes visible to the other lanes of its wave (global memory and LDS), and the wave is back in step
#if defined(__HIP_DEVICE_COMPILE__)
#define K9_WAVE_FENCE() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); RFX_WAVE_JOIN(); } while (0)
#else
#define K9_WAVE_FENCE() RFX_WAVE_JOIN()
#endif

struct K9WaveIO {
    const unsigned char *in;
    size_t in_len, nwords;  // nwords = ceil(in_len / 4)
    unsigned char *out;
    K9Tables *t;
    unsigned int *red;      // 128 words of LDS: the Adler sums of the lanes
    int lane;
    size_t win_base;        // the 64 input words [win_base, win_base + 64) sit one per lane in `win`
    unsigned int win;
    size_t synced;          // out[0, synced) is visible to every lane

    RFX_DEV unsigned int word(size_t i) {
        if (i >= nwords) return 0u;
        const size_t base = i & ~(size_t)63;
        if (base != win_base) {
            const size_t k = base + (size_t)lane;
            unsigned int w = 0u;
            if (4 * k + 4 <= in_len) w = ((const unsigned int *)in)[k];  // (the packed bytes start 256-byte aligned)
            else
                for (int j = 0; j < 4; j++)
                    if (4 * k + (size_t)j < in_len) w |= (unsigned int)in[4 * k + (size_t)j] << (8 * j);
            win = w;
            win_base = base;
        }
        return (unsigned int)__shfl((int)win, (int)(i & 63));
    }
    RFX_DEV void put(size_t pos, unsigned int byte) {
        if (lane == (int)(pos & 63)) out[pos] = (unsigned char)byte;
    }
    RFX_DEV void copy(size_t pos, unsigned int dist, unsigned int len) {
        const unsigned int span = dist < len ? dist : len;  // the source bytes: [pos - dist, pos - dist + span)
        if (pos - dist + span > synced) {
            K9_WAVE_FENCE();
            synced = pos;
        }
        const unsigned char *src = out + (pos - dist);
        for (unsigned int k = (unsigned int)lane; k < len; k += 64u) out[pos + k] = src[dist >= len ? k : k % dist];
    }
    RFX_DEV void copy_in(size_t pos, size_t src, unsigned int len) {
        for (unsigned int k = (unsigned int)lane; k < len; k += 64u) out[pos + k] = in[src + k];
    }
    RFX_DEV void fill(size_t pos, unsigned int byte, unsigned int len) {
        for (unsigned int k = (unsigned int)lane; k < len; k += 64u) out[pos + k] = (unsigned char)byte;
    }
    // 256 bytes per step, one dword per lane: a piece of m bytes ending e bytes before the end adds (sum, sum of (m - j) byte_j + e * sum) to (a, b).
    // The sums stay below 2^64 for n < 2^30 (rfx_stage_exr_aov refuses a larger chunk) and are reduced once.
    RFX_DEV unsigned int adler(size_t n) {
        K9_WAVE_FENCE();
        unsigned long long a = 0ull, b = 0ull;
        for (size_t at = 4 * (size_t)lane; at < n; at += 256) {
            const unsigned int m = n - at < 4 ? (unsigned int)(n - at) : 4u;
            unsigned int by[4] = {0u, 0u, 0u, 0u};
            if (m == 4u) {
                const unsigned int w = *(const unsigned int *)(out + at);  // (the slot starts 256-byte aligned)
                by[0] = w & 255u; by[1] = (w >> 8) & 255u; by[2] = (w >> 16) & 255u; by[3] = w >> 24;
            } else
                for (unsigned int j = 0; j < m; j++) by[j] = out[at + j];
            const unsigned int s = by[0] + by[1] + by[2] + by[3];
            unsigned int wsum = 0u;
            for (unsigned int j = 0; j < m; j++) wsum += (m - j) * by[j];
            a += s;
            b += wsum + (unsigned long long)s * (unsigned long long)(n - at - m);
        }
        red[lane] = (unsigned int)(a % 65521ull);
        red[64 + lane] = (unsigned int)(b % 65521ull);
        K9_WAVE_FENCE();
        unsigned long long ta = 1ull, tb = (unsigned long long)(n % 65521);
        for (int l = 0; l < 64; l++) { ta += red[l]; tb += red[64 + l]; }
        K9_WAVE_FENCE();  // (red is free again)
        return ((unsigned int)(tb % 65521ull) << 16) | (unsigned int)(ta % 65521ull);
    }
    RFX_DEV K9Tables &tables() { return *t; }
    RFX_DEV void sync() { K9_WAVE_FENCE(); }
};

RFX_DEV bool k9_raw_form(const K9Chunk &ck, const K9Part &pt) { return pt.compression == RFX_EXR_NONE || ck.packed == ck.raw; }
RFX_DEV bool k9_rle_form(const K9Chunk &ck, const K9Part &pt) { return pt.compression == RFX_EXR_RLE && ck.packed != ck.raw; }
RFX_DEV bool k9_piz_form(const K9Chunk &ck, const K9Part &pt) { return pt.compression == RFX_EXR_PIZ && ck.packed != ck.raw; }

// k9_piz.h's IO on the wave: the tables in LDS, the sorted symbols in the block's table scratch; the words leave in groups of 64 — lane l holds
// the word of position (pstart & ~63) + l until its group is full or a run follows —, a run is stored by all lanes.
struct K9PizWaveIO : K9WaveIO {
    K9PizHuf *h;
    unsigned short *symbols, *out16;
    unsigned int pend;
    size_t pstart;  // out16[0, pstart) is stored; the words of [pstart, n) wait in `pend`, all in one group of 64
    RFX_DEV bool leader() const { return lane == 0; }
    RFX_DEV unsigned int bcast(unsigned int v) { return (unsigned int)__shfl((int)v, 0); }
    RFX_DEV K9PizHuf &huf() { return *h; }
    RFX_DEV void fast_fill(unsigned int lo, unsigned int n, unsigned int e) {
        for (unsigned int k = (unsigned int)lane; k < n; k += 64u) h->fast[lo + k] = e;
    }
    RFX_DEV void sym_put(unsigned int i, unsigned int v) {
        if (lane == 0) symbols[i] = (unsigned short)v;
    }
    RFX_DEV unsigned int sym(unsigned int i) const { return symbols[i]; }
    RFX_DEV void flush(size_t n) {
        const size_t pos = (pstart & ~(size_t)63) + (size_t)lane;
        if (pos >= pstart && pos < n) out16[pos] = (unsigned short)pend;
        pstart = n;
    }
    RFX_DEV void put16(size_t n, unsigned int v) {
        if (lane == (int)(n & 63)) pend = v;
        if ((n & 63) == 63) flush(n + 1);
    }
    RFX_DEV void fill16(size_t n, unsigned int v, unsigned int len) {
        flush(n);
        for (unsigned int k = (unsigned int)lane; k < len; k += 64u) out16[n + k] = (unsigned short)v;
        pstart = n + len;
    }
};

__global__ __launch_bounds__(64) void k9_inflate(K9Args A) {
    __shared__ K9Tables tables;
    __shared__ unsigned int red[128];
    const K9Chunk ck = A.chunks[blockIdx.x];
    const K9Part pt = A.parts[ck.part];
    if (k9_rle_form(ck, pt) || k9_piz_form(ck, pt)) return;  // k9_rle's, k9_piz_huf's
    const int lane = (int)threadIdx.x;
    const unsigned char *in = A.packed + ck.src;
    unsigned char *out = A.scratch + ck.dst;
    int code = K9_OK;
    if (k9_raw_form(ck, pt)) {  // (packed == raw: checked by the host for a NONE part)
        const unsigned int words = ck.raw / 4u;
        for (unsigned int k = (unsigned int)lane; k < words; k += 64u) ((unsigned int *)out)[k] = ((const unsigned int *)in)[k];
        for (unsigned int k = words * 4u + (unsigned int)lane; k < ck.raw; k += 64u) out[k] = in[k];
    } else {
        K9WaveIO io;
        io.in = in; io.in_len = ck.packed; io.nwords = ((size_t)ck.packed + 3) / 4; io.out = out; io.t = &tables; io.red = red; io.lane = lane;
        io.win_base = ~(size_t)0; io.win = 0u; io.synced = 0;
        code = k9_inflate_zlib(io, (size_t)ck.packed, (size_t)ck.expect);  // (expect <= raw, the slot's size)
    }
    if (lane == 0) A.err[blockIdx.x] = code;
}

__global__ __launch_bounds__(64) void k9_rle(K9Args A) {
    const K9Chunk ck = A.chunks[blockIdx.x];
    const K9Part pt = A.parts[ck.part];
    if (!k9_rle_form(ck, pt)) return;  // k9_inflate's
    K9WaveIO io;
    io.in = A.packed + ck.src; io.in_len = ck.packed; io.nwords = ((size_t)ck.packed + 3) / 4; io.out = A.scratch + ck.dst; io.t = nullptr; io.red = nullptr;
    io.lane = (int)threadIdx.x; io.win_base = ~(size_t)0; io.win = 0u; io.synced = 0;
    const int code = k9_rle_expand(io, (size_t)ck.packed, (size_t)ck.raw);
    if (threadIdx.x == 0) A.err[blockIdx.x] = code;
}

// frame row fy of `plane`: the segment that stages it, or -1
RFX_DEV int k9_segment(const K9Args &A, int plane, int fy) {
    for (int s = 0; s < A.nseg; s++)
        if (fy >= A.seg_row0[s] && fy < A.seg_row0[s] + A.seg_rows[s] && A.seg_plane[s][plane]) return s;
    return -1;
}

// One wave per PIZ block: the reverse lookup table from the bitmap (a lane counts the bits of its 1024 values, the counts before it are where it
// writes), then k9_piz.h's Huffman decode: the block's words, channel-planar, into its scratch slot.  17 824 bytes of LDS per wave: 9 waves per CU.
__global__ __launch_bounds__(64) void k9_piz_huf(K9Args A) {
    __shared__ K9PizHuf huf;
    __shared__ unsigned int bits[64];
    const K9Chunk ck = A.chunks[blockIdx.x];
    const K9Part pt = A.parts[ck.part];
    if (!k9_piz_form(ck, pt)) return;
    const int lane = (int)threadIdx.x;
    unsigned char *tab = A.piz_tables + (size_t)ck.piz * K9_PIZ_TABLE_BYTES;
    K9PizWaveIO io;
    io.in = A.packed + ck.src; io.in_len = ck.packed; io.nwords = ((size_t)ck.packed + 3) / 4; io.out = A.scratch + ck.dst; io.t = nullptr; io.red = nullptr;
    io.lane = lane; io.win_base = ~(size_t)0; io.win = 0u; io.synced = 0;
    io.h = &huf; io.symbols = (unsigned short *)(tab + K9_PIZ_REV_BYTES); io.out16 = (unsigned short *)io.out; io.pend = 0u; io.pstart = 0;
    K9PizHead hd;
    int code = k9_piz_head(io, (size_t)ck.packed, &hd);
    if (!code) {
        const unsigned char *bm = io.in + 4;  // (k9_piz_head: bytes [4, 4 + bm_max - bm_min] lie inside the block)
        bits[lane] = k9_piz_rev_count(bm, hd.bm_min, hd.bm_max, lane);
        K9_WAVE_FENCE();
        unsigned int base = 0u, total = 0u;
        for (int l = 0; l < 64; l++) {
            if (l < lane) base += bits[l];
            total += bits[l];
        }
        k9_piz_rev_write(bm, hd.bm_min, hd.bm_max, lane, base, total, (unsigned short *)tab);
        if (lane == 0) *(int *)(tab + K9_PIZ_REV_BYTES + K9_PIZ_SYM_BYTES) = (int)total - 1;  // mx
        code = k9_piz_huf_decode(io, hd.huf_at, hd.huf_len, (size_t)ck.raw / 2);
    }
    if (lane == 0) A.err[blockIdx.x] = code;
}

// The parallel part of a PIZ block: one workgroup per (channel, cell) in turn — K9_PIZ_SLICES workgroups share a block's cells —: the cell of each of
// the channel's word planes (HALF: one; FLOAT: two, interleaved in x, the low word first) into LDS, the wavelet levels from the coarsest to the
// finest (k9_piz.h k9_piz_cell_level, one thread per square), the reverse lookup, and the samples to the staging planes as k9_exr_planes scatters.
constexpr int K9_PIZ_SLICES = 8, K9_PIZ_BLOCK = 256;
static_assert(K9_PIZ_CELL == RFX_EXR_PIZ_CELL, "the plan's cell is the kernel's");
__global__ __launch_bounds__(K9_PIZ_BLOCK) void k9_piz_planes(K9Args A) {
    __shared__ unsigned short cell[2][K9_PIZ_CELL * K9_PIZ_CELL];
    const K9Chunk ck = A.chunks[blockIdx.x];
    const K9Part pt = A.parts[ck.part];
    if (!k9_piz_form(ck, pt) || A.err[blockIdx.x]) return;  // (a bad block: k9_exr_planes writes its zeros)
    const int tid = (int)threadIdx.x;
    const unsigned short *words = (const unsigned short *)(A.scratch + ck.dst);
    const unsigned char *tab = A.piz_tables + (size_t)ck.piz * K9_PIZ_TABLE_BYTES;
    const unsigned short *rev = (const unsigned short *)tab;
    const bool w14 = *(const int *)(tab + K9_PIZ_REV_BYTES + K9_PIZ_SYM_BYTES) < (1 << 14);
    const int cols = ck.cols, rows = ck.rows, cx = (cols + K9_PIZ_CELL - 1) / K9_PIZ_CELL, cy = (rows + K9_PIZ_CELL - 1) / K9_PIZ_CELL;
    const int top = k9_piz_top_level(cols, rows), items = pt.nchan * cx * cy;
    for (int it = (int)blockIdx.y; it < items; it += (int)gridDim.y) {  // (every condition on the way to a barrier is uniform over the workgroup)
        const int c = it / (cx * cy), rem = it - c * cx * cy, y0 = (rem / cx) * K9_PIZ_CELL, x0 = (rem % cx) * K9_PIZ_CELL;
        const K9Chan ch = A.chans[pt.chan0 + c];
        if (ch.plane < 0) continue;
        const int size = ch.half ? 1 : 2;
        const int w = cols - x0 < K9_PIZ_CELL ? cols - x0 : K9_PIZ_CELL, h = rows - y0 < K9_PIZ_CELL ? rows - y0 : K9_PIZ_CELL;
        const unsigned short *plane = words + (size_t)rows * (size_t)cols * (ch.off / 2u);  // (channel-planar: ch.off / 2 words per texel before it)
        __syncthreads();  // the cell of the previous turn has been read
        for (int i = tid; i < h * w * size; i += K9_PIZ_BLOCK) {
            const int ly = i / (w * size), k = i - ly * (w * size);
            cell[k % size][ly * K9_PIZ_CELL + k / size] = plane[(size_t)(y0 + ly) * (size_t)(cols * size) + (size_t)(x0 * size + k)];
        }
        __syncthreads();
        for (int p = top; p >= 1; p >>= 1) {
            for (int j = 0; j < size; j++) k9_piz_cell_level(cell[j], x0, y0, cols, rows, p, w14, tid, K9_PIZ_BLOCK);
            __syncthreads();
        }
        for (int i = tid; i < h * w; i += K9_PIZ_BLOCK) {
            const int ly = i / w, lx = i - ly * w;
            const int fy = A.H - 1 - (ck.y + y0 + ly);
            const int s = k9_segment(A, ch.plane, fy);
            if (s < 0) continue;
            unsigned int bits = rev[cell[0][ly * K9_PIZ_CELL + lx]];
            if (size == 2) bits |= (unsigned int)rev[cell[1][ly * K9_PIZ_CELL + lx]] << 16;
            const size_t dst = ((size_t)(fy - A.seg_row0[s]) * A.W + (size_t)(ck.x + x0 + lx)) * A.plane_ch[ch.plane] + ch.comp;
            if (A.plane_half[ch.plane]) ((unsigned short *)A.seg_plane[s][ch.plane])[dst] = (unsigned short)bits;
            else ((float *)A.seg_plane[s][ch.plane])[dst] = ch.half ? rfx_h2f((unsigned short)bits) : __uint_as_float(bits);
        }
    }
}

constexpr int K9_PLANES_BLOCK = 256, K9_SCAN_BYTES = 16;
__global__ __launch_bounds__(K9_PLANES_BLOCK) void k9_exr_planes(K9Args A) {
    __shared__ unsigned int scan[K9_PLANES_BLOCK];
    const K9Chunk ck = A.chunks[blockIdx.x];
    const K9Part pt = A.parts[ck.part];
    unsigned char *buf = A.scratch + ck.dst;
    const int tid = (int)threadIdx.x;
    const int err = A.err[blockIdx.x];
    const bool raw_form = k9_raw_form(ck, pt);
    if (k9_piz_form(ck, pt) && !err) return;  // k9_piz_planes' (PIZ has no predictor and no byte split; a bad block's zeros are written below)
    const unsigned int n = ck.raw;
    const unsigned int cols = (unsigned int)ck.cols;
    if (pt.compression == RFX_EXR_PXR24 && !raw_form && !err) {
        // buf: per row and channel the k byte planes of the differences.  One (row, channel) segment per wave and turn; everything that decides
        // whether a segment is walked is wave-uniform, so the shuffles below see all 64 lanes.
        const int wave = tid >> 6, lane = tid & 63, nsegs = ck.rows * pt.nchan;
        for (int sg = wave; sg < nsegs; sg += K9_PLANES_BLOCK / 64) {
            const int r = sg / pt.nchan;
            const K9Chan ch = A.chans[pt.chan0 + (sg - r * pt.nchan)];
            if (ch.plane < 0) continue;
            const int fy = A.H - 1 - (ck.y + r);
            const int s = k9_segment(A, ch.plane, fy);
            if (s < 0) continue;
            const unsigned char *seg = buf + (size_t)r * cols * pt.pxr_bytes + (size_t)cols * ch.pxr_off;
            const unsigned int k = k9_pxr24_planes(ch.half);
            const size_t row = ((size_t)(fy - A.seg_row0[s]) * A.W + (size_t)ck.x) * A.plane_ch[ch.plane] + ch.comp;
            unsigned int carry = 0u;
            for (unsigned int base = 0; base < cols; base += 64u) {
                const unsigned int i = base + (unsigned int)lane;
                unsigned int sum = k9_pxr24_diff(seg, cols, k, i);
                for (int off = 1; off < 64; off <<= 1) sum = k9_pxr24_scan_step(lane, off, sum, (unsigned int)__shfl((int)sum, lane - off));
                sum += carry;
                carry = (unsigned int)__shfl((int)sum, 63);
                if (i >= cols) continue;
                const unsigned int bits = k9_pxr24_bits(sum, ch.half);
                const size_t dst = row + (size_t)i * A.plane_ch[ch.plane];
                if (A.plane_half[ch.plane]) ((unsigned short *)A.seg_plane[s][ch.plane])[dst] = (unsigned short)bits;
                else ((float *)A.seg_plane[s][ch.plane])[dst] = ch.half ? rfx_h2f((unsigned short)bits) : __uint_as_float(bits);
            }
        }
        return;
    }
    if (!raw_form && !err) {
        unsigned int carry = 0u;  // the sum of every d[j] - 128 before the tile, mod 256
        for (unsigned int tile = 0; tile < n; tile += K9_PLANES_BLOCK * K9_SCAN_BYTES) {
            const unsigned int at = tile + (unsigned int)tid * K9_SCAN_BYTES;
            const unsigned int m = at >= n ? 0u : (n - at < K9_SCAN_BYTES ? n - at : (unsigned int)K9_SCAN_BYTES);
            unsigned char d[K9_SCAN_BYTES];
            if (m == K9_SCAN_BYTES) {
                const uint4 w = *(const uint4 *)(buf + at);  // (the slot starts 256-byte aligned)
                const unsigned int ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int k = 0; k < K9_SCAN_BYTES; k++) d[k] = (unsigned char)(ws[k >> 2] >> (8 * (k & 3)));
            } else
                for (unsigned int k = 0; k < m; k++) d[k] = buf[at + k];
            unsigned int run = 0u;
            for (unsigned int k = 0; k < m; k++) {
                run = (run + d[k] + 128u) & 255u;  // (+128 = -128 mod 256)
                d[k] = (unsigned char)run;
            }
            scan[tid] = run;
            __syncthreads();
            for (int off = 1; off < K9_PLANES_BLOCK; off <<= 1) {
                const unsigned int v = tid >= off ? scan[tid - off] : 0u;
                __syncthreads();
                scan[tid] += v;
                __syncthreads();
            }
            const unsigned int before = (carry + scan[tid] - run) & 255u;  // every byte before this thread's run
            carry = (carry + scan[K9_PLANES_BLOCK - 1]) & 255u;
            for (unsigned int k = 0; k < m; k++) buf[at + k] = (unsigned char)(before + d[k] + 128u);  // t[i] = 128 + the sum of d[j] - 128, j <= i
            __syncthreads();
        }
    }
    __syncthreads();
    const unsigned int half_n = (n + 1u) / 2u;  // the even-indexed bytes of the raw block come first
    const auto raw_byte = [&](unsigned int p) -> unsigned int { return raw_form ? buf[p] : ((p & 1u) ? buf[half_n + (p >> 1)] : buf[p >> 1]); };
    const unsigned int per_row = (unsigned int)pt.nchan * cols, total = (unsigned int)ck.rows * per_row, row_bytes = cols * pt.texel_bytes;
    for (unsigned int i = (unsigned int)tid; i < total; i += K9_PLANES_BLOCK) {
        const unsigned int r = i / per_row, rem = i - r * per_row, c = rem / cols, x = rem - c * cols;
        const K9Chan ch = A.chans[pt.chan0 + (int)c];
        if (ch.plane < 0) continue;
        const int fy = A.H - 1 - (ck.y + (int)r);
        const int s = k9_segment(A, ch.plane, fy);
        if (s < 0) continue;
        const size_t dst = ((size_t)(fy - A.seg_row0[s]) * A.W + (size_t)ck.x + x) * A.plane_ch[ch.plane] + ch.comp;
        unsigned int bits;
        if (err) {
            bits = 0u;
        } else {
            const unsigned int p = r * row_bytes + cols * ch.off + x * (ch.half ? 2u : 4u);
            bits = raw_byte(p) | (raw_byte(p + 1u) << 8);
            if (!ch.half) bits |= (raw_byte(p + 2u) << 16) | (raw_byte(p + 3u) << 24);
        }
        if (A.plane_half[ch.plane]) ((unsigned short *)A.seg_plane[s][ch.plane])[dst] = (unsigned short)bits;  // (every channel of the plane is HALF)
        else ((float *)A.seg_plane[s][ch.plane])[dst] = ch.half ? rfx_h2f((unsigned short)bits) : __uint_as_float(bits);
    }
}

__global__ __launch_bounds__(256) void k9_exr_finish(K9Args A) {
    const int err = A.err[blockIdx.x];
    if (!err) return;
    const K9Chunk ck = A.chunks[blockIdx.x];
    if (threadIdx.x == 0) {
        atomicAdd((unsigned int *)A.status, 1u);
        atomicMax(A.status + 1, 0x7fffffff - ((ck.index << 8) | err));
    }
    const unsigned int cols = (unsigned int)ck.cols, total = (unsigned int)ck.rows * cols;
    for (unsigned int i = threadIdx.x; i < total; i += 256u) {
        const unsigned int r = i / cols, x = i - r * cols;
        const int fy = A.H - 1 - (ck.y + (int)r);
        const int s = k9_segment(A, RFX_AOV_DEPTH, fy);
        if (s < 0) continue;
        const size_t dst = (size_t)(fy - A.seg_row0[s]) * A.W + (size_t)ck.x + x;
        const int dc = A.plane_ch[RFX_AOV_DEPTH];
        for (int ch = 0; ch < dc; ch++) {
            if (A.plane_half[RFX_AOV_DEPTH]) ((unsigned short *)A.seg_plane[s][RFX_AOV_DEPTH])[dst * dc + ch] = (unsigned short)(A.depth_bad_nan ? 0x7e00u : 0x3c00u);
            else ((unsigned int *)A.seg_plane[s][RFX_AOV_DEPTH])[dst * dc + ch] = A.depth_bad_nan ? 0x7fc00000u : 0x3f800000u;
        }
    }
}

}  // namespace

hipError_t rfx_launch_k9(const K9Args &A, hipStream_t stream) {
    if (A.nchunks <= 0 || !A.chunks || !A.parts || !A.chans || !A.packed || !A.scratch || !A.err || !A.status) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k9_inflate, dim3(A.nchunks), dim3(64), 0, stream, A);
    if (A.rle_chunks > 0) hipLaunchKernelGGL(k9_rle, dim3(A.nchunks), dim3(64), 0, stream, A);  // (a frame without an RLE stream: nothing to do)
    if (A.piz_chunks > 0) {
        if (!A.piz_tables) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k9_piz_huf, dim3(A.nchunks), dim3(64), 0, stream, A);
        hipLaunchKernelGGL(k9_piz_planes, dim3(A.nchunks, K9_PIZ_SLICES), dim3(K9_PIZ_BLOCK), 0, stream, A);
    }
    hipLaunchKernelGGL(k9_exr_planes, dim3(A.nchunks), dim3(K9_PLANES_BLOCK), 0, stream, A);
    hipLaunchKernelGGL(k9_exr_finish, dim3(A.nchunks), dim3(256), 0, stream, A);
    return hipGetLastError();
}
