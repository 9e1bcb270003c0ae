// K6 — MotionBlurEffect's mainImage, src/motion-blur/shader/motion_blur.frag:11-45 (blueNoise: src/utils/shader/blue_noise.glsl:37-45).
// One lane per pixel on 16 x 16 tiles: the samples + 1 LINEAR taps of a streak in any direction stay near the tile's other taps in L1.
// Every expression keeps the GLSL's operation order and rounding: this file is compiled with contraction on, so the arithmetic below
// is written uncontracted and the fused operations the reference GL performs (its sampler's lerps) are explicit fmas.
#include "rfx_device.h"
#include "rfx_kernels.h"
#include "rfx_blocks.h"

namespace {

// textureLod(inputTexture, uv, 0.) on an RGBA32F texture, LinearFilter, CLAMP_TO_EDGE, as the reference GL's sampler computes it:
// llvmpipe's coordinates (rfx_linear_coord_fast: rfx_linear_coord's (i0, w) for every finite coordinate; NaN clamps to texel 0)
// and its fused lerps.  The ADDRESS half of the fetch — which four texels, which weights — is k6_footprint: the draw loads them, the reach
// reduction of a row-tiled run (k6_motion_blur_reach) names them, both from this one function.
struct K6Foot {
    int x0, x1, y0, y1;  // the footprint's columns and frame rows
    float wx, wy;
};
RFX_DEV K6Foot k6_footprint(const FrameDims &d, float u, float v) {
#pragma clang fp contract(off)
    const float cx = u * d.fW, cy = v * d.fH;
    const LinearCoord lx = rfx_linear_coord_fast(cx, d.fW - 0.5f), ly = rfx_linear_coord_fast(cy, d.fH - 0.5f);
    K6Foot f;
    f.x0 = lx.i0; f.y0 = ly.i0;
    f.x1 = min(lx.i0 + 1, d.W - 1); f.y1 = min(ly.i0 + 1, d.H - 1);
    f.wx = lx.w; f.wy = ly.w;
    return f;
}
// .rgb only: the effect never reads a tap's alpha.  `t` is a whole-frame plane (frame row y at y * W).
RFX_DEV float3 k6_tap(const float4 *t, const FrameDims &d, float u, float v) {
#pragma clang fp contract(off)
    const K6Foot f = k6_footprint(d, u, v);
    const unsigned int r0 = (unsigned int)__mul24(f.y0, d.W), r1 = (unsigned int)__mul24(f.y1, d.W);
    const float4 t00 = rfx_gather<float4>(t, r0 + f.x0), t10 = rfx_gather<float4>(t, r0 + f.x1);
    const float4 t01 = rfx_gather<float4>(t, r1 + f.x0), t11 = rfx_gather<float4>(t, r1 + f.x1);
    const float wx = f.wx, wy = f.wy;
    const float r0x = __builtin_fmaf(wx, t10.x - t00.x, t00.x), r1x = __builtin_fmaf(wx, t11.x - t01.x, t01.x);
    const float r0y = __builtin_fmaf(wx, t10.y - t00.y, t00.y), r1y = __builtin_fmaf(wx, t11.y - t01.y, t01.y);
    const float r0z = __builtin_fmaf(wx, t10.z - t00.z, t00.z), r1z = __builtin_fmaf(wx, t11.z - t01.z, t01.z);
    return make_float3(__builtin_fmaf(wy, r1x - r0x, r0x), __builtin_fmaf(wy, r1y - r0y, r0y), __builtin_fmaf(wy, r1z - r0z, r0z));
}
// the same fetch with alpha: inputColor in the effect's own EffectPass, texture2D(inputBuffer, vUv)
RFX_DEV float4 k6_center_linear(const float4 *t, const FrameDims &d, float u, float v) {
#pragma clang fp contract(off)
    const K6Foot f = k6_footprint(d, u, v);
    const unsigned int r0 = (unsigned int)__mul24(f.y0, d.W), r1 = (unsigned int)__mul24(f.y1, d.W);
    const float4 t00 = rfx_gather<float4>(t, r0 + f.x0), t10 = rfx_gather<float4>(t, r0 + f.x1);
    const float4 t01 = rfx_gather<float4>(t, r1 + f.x0), t11 = rfx_gather<float4>(t, r1 + f.x1);
    const float wx = f.wx, wy = f.wy;
    float4 r;
    const float a0 = __builtin_fmaf(wx, t10.w - t00.w, t00.w), a1 = __builtin_fmaf(wx, t11.w - t01.w, t01.w);
    const float3 c = k6_tap(t, d, u, v);
    r.x = c.x; r.y = c.y; r.z = c.z;
    r.w = __builtin_fmaf(wy, a1 - a0, a0);
    return r;
}
// The streak of a moved fragment, motion_blur.frag:20-32: startUv and endUv - startUv.  Shared by the draw and the reach reduction.
struct K6Streak { float su, sv, du, dv; };
RFX_DEV K6Streak k6_streak(const K6Args &A, float u, float v, float vx, float vy) {
#pragma clang fp contract(off)
    vx *= A.intensity;  // :20
    vy *= A.intensity;
    // :22 blueNoise(vUv, frame): ivec2(vUv * resolution), shifted by the frame's pcg4d round (frame 0: the table at uv * resolution /
    // blueNoiseSize, NEAREST + REPEAT — the same texel, the division by 128 being exact); vUv * resolution >= 0: truncation = floor
    const float4 bn = rfx_blue_noise(A.blue, (int)(u * A.resX), (int)(v * A.resY), A.shift_x, A.shift_y);
    const float jx = (A.jitter * vx) * bn.x, jy = (A.jitter * vy) * bn.y;  // :23
    const float hx = vx * 0.5f, hy = vy * 0.5f;
    // :28-32
    const float su = rfx_max_raw(0.0f, u + (jx - hx) * A.frameSpeed), sv = rfx_max_raw(0.0f, v + (jy - hy) * A.frameSpeed);
    const float eu = rfx_min_raw(1.0f, u + (jx + hx) * A.frameSpeed), ev = rfx_min_raw(1.0f, v + (jy + hy) * A.frameSpeed);
    K6Streak s;
    s.su = su; s.sv = sv; s.du = eu - su; s.dv = ev - sv;
    return s;
}
// :36-37 the uv of tap i: mix(startUv, endUv, i / samplesFloat) with the quotient correctly rounded and the mix as the reference GL lowers it,
// a + t * (b - a), two roundings (tools/probe_motion_blur_gl.py)
RFX_DEV float2 k6_tap_uv(const K6Args &A, const K6Streak &s, int i) {
#pragma clang fp contract(off)
    const float t = rfx_div_const_impl((float)i, A.samplesF, A.rcpSamplesF);
    return make_float2(s.su + t * s.du, s.sv + t * s.dv);
}
// :13-18 is the fragment moved?  (NaN: not moved)
RFX_DEV bool k6_moved(float vx, float vy) {
#pragma clang fp contract(off)
    return vx * vx + vy * vy > 0.000000001f;
}

template <bool TILED>
RFX_DEV void k6_motion_blur_body(const K6Args &A, const FrameDims &d) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 16 + threadIdx.x, y = A.y0 + blockIdx.y * 16 + threadIdx.y;
    if (x >= d.W || y >= A.y1) return;
    const float u = rfx_frag_u(d.uv, x, y), v = rfx_frag_v(d.uv, y);
    const unsigned int idx = (unsigned int)__mul24(y, d.W) + (unsigned int)x;
    // the pixel's own texel in the planes a row-tiled context holds as bands
    const unsigned int vidx = TILED ? (unsigned int)__mul24(rfx_local_row(d, A.vel_row0, A.vel_rows, y), d.W) + (unsigned int)x : idx;
    const unsigned int oidx = TILED ? (unsigned int)__mul24(rfx_local_row(d, A.out_row0, A.out_rows, y), d.W) + (unsigned int)x : idx;
    // inputColor: TRAA's NEAREST target texel (README form) or the LINEAR fetch of the pass's input buffer at vUv
    float4 o;
    if (TILED) {  // (a LINEAR centre of a row-tiled draw is the source's own: `center` is the whole-frame plane then, rfx_motion_blur)
        o = A.center_nearest ? rfx_gather<float4>(A.center, (unsigned int)__mul24(rfx_local_row(d, A.center_row0, A.center_rows, y), d.W) + (unsigned int)x)
                             : k6_center_linear(A.center, d, u, v);
    } else {
        o = A.center_nearest ? rfx_gather<float4>(A.center, idx) : k6_center_linear(A.center, d, u, v);
    }
    if (A.center_alpha_one) o.w = 1.0f;  // traa_compose.frag:6
    const float4 vel = rfx_gather<float4>(A.velocity, vidx);  // :12 textureLod(velocityTexture, vUv, 0.0).xy, NEAREST
    if (k6_moved(vel.x, vel.y)) {
        const K6Streak s = k6_streak(A, u, v, vel.x, vel.y);
        float3 acc = make_float3(o.x, o.y, o.z);  // :34
        for (int i = 0; i <= A.samples; i++) {  // :35-40
            const float2 tuv = k6_tap_uv(A, s, i);
            const float3 c = k6_tap(A.src, d, tuv.x, tuv.y);
            acc.x = acc.x + c.x;
            acc.y = acc.y + c.y;
            acc.z = acc.z + c.z;
        }
        // :42 motionBlurredColor /= samplesFloat + 2. (IEEE division: any sum, infinities and subnormal quotients included)
        o.x = acc.x / A.div2;
        o.y = acc.y / A.div2;
        o.z = acc.z / A.div2;
    }
    if (A.target_half) o = rfx_round_half4(o, A.half_rtz != 0);  // HalfFloatType composer buffer
    A.out[oidx] = o;
}

__global__ __launch_bounds__(256) void k6_motion_blur(K6Args A) {
    k6_motion_blur_body<false>(A, A.dims);
}

// The row-tiled form: the same fragment with velocity, an explicit (NEAREST) centre and the output addressed through their bands; the taps and
// the `center == -1` fetch read RFX_TEX_BLUR_SOURCE, held whole.
__global__ __launch_bounds__(256) void k6_motion_blur_tiled(K6Args A) {
    FrameDims d = A.dims;
    d.viol = 0;
    k6_motion_blur_body<true>(A, d);
    rfx_flush_violations(d);
}

// ---- the reach reduction of a row-tiled blur (rfx_motion_blur_reach_mask / rfx_motion_blur_gather): the texels of `src` the draw above will
// LOAD for rows [y0, y1), as the bounded history gather's row mask (k1_hit_mask in k1_ssgi.hip: one word per frame row, bit b = column block
// b, rfx_blocks.h).  The same k6_moved / k6_streak / k6_tap_uv / k6_footprint as the draw, without the loads — so the mask is
// exact (zero-weight footprint texels included: the draw loads them, and 0 * NaN is NaN), not a bound derived from the velocity's magnitude.
// One lane per pixel, one wave per 64 pixels of a row.
// Guarded as k1_hit_mask's: a set bit is never set again.  The test is a plain load, which the L1 may serve from a stale copy (the atomics
// execute in the L2) at the cost of a redundant atomic; reading the word past the L1 instead was measured and is slower
// (profiles/motion_blur/tiled.md).
RFX_DEV void k6_mark(unsigned int *mask, int row, unsigned int bits) {
    if ((mask[row] & bits) != bits) atomicOr(&mask[row], bits);
}
// What a lane has named and not yet written: the two rows of its last footprints (packed, -1 = nothing) and their column-block bits.  A
// streak's consecutive taps mostly stay on the same two rows, so the mask is touched once per change of rows, not once per tap.
struct K6Pending {
    int rows;
    unsigned int bits;
};
// One wave = 64 pixels of a frame row, ALL lanes here (`want`: the lane has something to write).  Where the lanes that write agree on the two
// rows (a pan) the bits are OR-reduced across the wave and one lane touches the mask.
RFX_DEV void k6_flush_wave(unsigned int *mask, const K6Pending &p, bool want) {
    const unsigned long long lv = __ballot(want);
    if (!lv) return;  // (wave-uniform)
    const int first = __shfl(p.rows, (int)__builtin_ctzll(lv));
    if (__ballot(want && p.rows != first) == 0) {
        int b = want ? (int)p.bits : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) b |= __shfl_xor(b, o);
        if (threadIdx.x == 0) {
            k6_mark(mask, first & 0xffff, (unsigned int)b);
            if ((first >> 16) != (first & 0xffff)) k6_mark(mask, first >> 16, (unsigned int)b);
        }
    } else if (want) {
        k6_mark(mask, p.rows & 0xffff, p.bits);
        if ((p.rows >> 16) != (p.rows & 0xffff)) k6_mark(mask, p.rows >> 16, p.bits);
    }
}
// name the four texels of a footprint (`live`: this lane loads it)
RFX_DEV void k6_name(unsigned int *mask, K6Pending &p, const K6Foot &f, int W, bool live) {
    const unsigned int bits = (1u << rfx_block_of_col(f.x0, W)) | (1u << rfx_block_of_col(f.x1, W));
    const int rows = f.y0 | (f.y1 << 16);  // rows are < 2^15 (rfx_create)
    k6_flush_wave(mask, p, live && p.rows >= 0 && p.rows != rows);
    if (live) {
        p.bits = p.rows == rows ? (p.bits | bits) : bits;
        p.rows = rows;
    }
}

__global__ __launch_bounds__(256) void k6_motion_blur_reach(K6Args A) {
#pragma clang fp contract(off)
    FrameDims d = A.dims;
    d.viol = 0;
    const int x = blockIdx.x * 64 + threadIdx.x, y = A.y0 + blockIdx.y * 4 + threadIdx.y;
    if (y >= A.y1) return;  // (wave-uniform: threadIdx.y is the wavefront)
    const bool in_frame = x < d.W;
    const int xc = min(x, d.W - 1);  // lanes past the right edge stay for the wave operations and name nothing
    const float u = rfx_frag_u(d.uv, xc, y), v = rfx_frag_v(d.uv, y);
    K6Pending pend;
    pend.rows = -1; pend.bits = 0u;
    if (A.center_is_source) k6_name(A.reach_mask, pend, k6_footprint(d, u, v), d.W, in_frame);  // inputColor = texture2D(inputBuffer, vUv)
    const float4 vel = rfx_gather<float4>(A.velocity, (unsigned int)__mul24(rfx_local_row(d, A.vel_row0, A.vel_rows, y), d.W) + (unsigned int)xc);
    const bool moved = in_frame && k6_moved(vel.x, vel.y);
    if (__ballot(moved) != 0) {  // (wave-uniform)
        const K6Streak s = k6_streak(A, u, v, vel.x, vel.y);
        for (int i = 0; i <= A.samples; i++) {
            const float2 tuv = k6_tap_uv(A, s, i);
            k6_name(A.reach_mask, pend, k6_footprint(d, tuv.x, tuv.y), d.W, moved);
        }
    }
    k6_flush_wave(A.reach_mask, pend, pend.rows >= 0);
    rfx_flush_violations(d);  // (a velocity row outside the held band: counted, as the draw counts it)
}

}  // namespace

hipError_t rfx_launch_k6(const K6Args &A, hipStream_t stream) {
    dim3 block(16, 16), grid((A.dims.W + 15) / 16, (A.y1 - A.y0 + 15) / 16);
    if (A.tiled) hipLaunchKernelGGL(k6_motion_blur_tiled, grid, block, 0, stream, A);
    else hipLaunchKernelGGL(k6_motion_blur, grid, block, 0, stream, A);
    return hipGetLastError();
}

hipError_t rfx_launch_k6_reach(const K6Args &A, hipStream_t stream) {
    dim3 block(64, 4), grid((A.dims.W + 63) / 64, (A.y1 - A.y0 + 3) / 4);
    hipLaunchKernelGGL(k6_motion_blur_reach, grid, block, 0, stream, A);
    return hipGetLastError();
}
