// K0 — importer: engine-side attribute planes (AOVs) -> the reference's packed render targets, on the device.
// Replaces the fragment epilogues of the two raster passes for an importer of engine dumps:
//   GBufferMaterial.js:84-89            gl_FragColor = packGBuffer(diffuseColor, worldNormal, roughnessFactor, metalnessFactor, totalEmissiveRadiance)
//   VelocityDepthNormalMaterial.js:76-83,186-188   gl_FragColor = vec4(vel.x, vel.y, packNormal(worldNormal), fragCoordZ)
// with the encode side of src/gbuffer/shader/gbuffer_packing.glsl (vec4ToFloat :143-149, packNormal / encodeOctWrap :44-61,
// color2float :17-22, encodeRGBE8 :127-134, packGBuffer :166-178).  Texels the rasteriser would not cover (depth == 1) keep the
// passes' clear colour, `scene.background = Color(0)` with alpha 1 (GBufferPass.js:103-105, VelocityDepthNormalPass.js:177-179).
// Streaming: 13 floats in, 16 B out per pixel (G-buffer); 6 floats in, 16 B out (velocity).
#include "rfx_device.h"
#include "rfx_kernels.h"
#include "rfx_launch.h"

namespace {

RFX_DEV uint32_t k0_vec4_to_float(float x, float y, float z, float w) {  // vec4ToFloat
    const float o = 0.0001f, one_safe = 0.999999f;
    // min() as the GLSL evaluates it: NaN (the 0/0 of encodeRGBE8 on a black emissive, Appendix D-9) does not propagate
    const uint32_t r = (uint32_t)(fminf(x + o, one_safe) * 255.0f), g = (uint32_t)(fminf(y + o, one_safe) * 255.0f);
    const uint32_t b = (uint32_t)(fminf(z + o, one_safe) * 255.0f), a = (uint32_t)(fminf(w + o, one_safe) * 255.0f);
    return (a << 24) | (b << 16) | (g << 8) | r;
}
RFX_DEV uint32_t k0_pack_normal(float3 n) {  // packNormal(encodeOctWrap(n))
    const float s = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);
    n.x /= s; n.y /= s; n.z /= s;
    float wx = 1.0f - fabsf(n.y), wy = 1.0f - fabsf(n.x);  // OctWrap
    if (n.x < 0.0f) wx = -wx;
    if (n.y < 0.0f) wy = -wy;
    const float ox = n.z > 0.0f ? n.x : wx, oy = n.z > 0.0f ? n.y : wy;
    return rfx_pack_half2(ox * 0.5f + 0.5f, oy * 0.5f + 0.5f);
}
RFX_DEV float k0_color2float(float r, float g, float b) {  // color2float
    const float o = 0.0001f, one_safe = 0.999999f, P = 256.0f, P1 = 257.0f;
    r = fminf(r + o, one_safe); g = fminf(g + o, one_safe); b = fminf(b + o, one_safe);
    return floorf(r * P + 0.5f) + floorf(b * P + 0.5f) * P1 + floorf(g * P + 0.5f) * P1 * P1;
}
RFX_DEV uint32_t k0_rgbe8(float3 c) {  // vec4ToFloat(encodeRGBE8(rgb))
    const float mx = fmaxf(fmaxf(c.x, c.y), c.z);
    const float fexp = ceilf(rfx_log2(mx));
    const float sc = rfx_exp2(fexp);
    return k0_vec4_to_float(c.x / sc, c.y / sc, c.z / sc, (fexp + 128.0f) / 255.0f);
}

struct K0GBuffer {
    int W, rows;
    const float *diffuse, *normal, *roughness, *metalness, *emissive, *depth;  // device staging planes of `rows` rows
    uint4 *out;                                                                // first output row
};
__global__ __launch_bounds__(256) void k0_pack_gbuffer(K0GBuffer A) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.W || y >= A.rows) return;
    const size_t i = (size_t)y * A.W + x;
    uint4 o;
    if (A.depth && A.depth[i] == 1.0f) {
        o = make_uint4(0u, 0u, 0u, 0x3f800000u);  // the clear colour (0, 0, 0, 1)
    } else {
        o.x = k0_vec4_to_float(A.diffuse[4 * i], A.diffuse[4 * i + 1], A.diffuse[4 * i + 2], A.diffuse[4 * i + 3]);
        o.y = k0_pack_normal(make_float3(A.normal[3 * i], A.normal[3 * i + 1], A.normal[3 * i + 2]));
        o.z = __float_as_uint(k0_color2float(A.roughness[i], A.metalness[i], 0.0f));
        o.w = k0_rgbe8(make_float3(A.emissive[3 * i], A.emissive[3 * i + 1], A.emissive[3 * i + 2]));
    }
    A.out[i] = o;
}

struct K0Velocity {
    int W, rows;
    const float *velocity, *normal, *depth;
    uint4 *out;
};
__global__ __launch_bounds__(256) void k0_pack_velocity(K0Velocity A) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.W || y >= A.rows) return;
    const size_t i = (size_t)y * A.W + x;
    const float d = A.depth[i];
    uint4 o;
    if (d == 1.0f) o = make_uint4(0u, 0u, 0u, 0x3f800000u);
    else
        o = make_uint4(__float_as_uint(A.velocity[2 * i]), __float_as_uint(A.velocity[2 * i + 1]),
                       k0_pack_normal(make_float3(A.normal[3 * i], A.normal[3 * i + 1], A.normal[3 * i + 2])), __float_as_uint(d));
    A.out[i] = o;
}

// ---------------------------------------------------------------- K0 AOV pack: the two packers above, fused, for rfx_stage_aov (include/rfx.h "streamed AOV frames")
// One pass over the flat pixel run of a segment (rfx_launch.h rfx_aov_plan_for): 44 .. 76 B in per pixel (84 with a float position plane), 52 B out.  Lane t owns the four
// consecutive pixels [4 t, 4 t + 4), as K7's does: a float plane of C channels is C 16-byte loads, a half plane C 8-byte loads (C / 2 16-byte
// loads for an even C), and every slot leaves as 16-byte stores — four G-buffer, four velocity and four direct-light texels and the four depth
// values.  Normal and depth are read once for both packed texels.  The pixels mod 4 left over go to the lane after the last group, element by
// element.  Which planes hold halves is uniform over a launch: SET 0 = none, SET 1 = every plane but velocity and depth (the 44 B/px frame of a
// renderer that writes HALF colour AOVs), SET 2 = whatever half_mask says, decided by branches on the argument block.  Nothing is decided per
// pixel but coverage.  The arithmetic is k0_pack_gbuffer's and k0_pack_velocity's own device functions on the widened values, and this file is
// built uncontracted: the texels are theirs bit for bit.
template <int SET>
RFX_DEV bool k0_aov_half(const K0AovArgs &A, int i) {
    if (SET == 0) return false;
    if (SET == 1) return i != RFX_AOV_VELOCITY && i != RFX_AOV_DEPTH;
    return ((A.half_mask >> i) & 1u) != 0u;
}
RFX_DEV void k0_aov_widen2(uint32_t w, float *v) { v[0] = rfx_h2f((unsigned short)(w & 0xffffu)); v[1] = rfx_h2f((unsigned short)(w >> 16)); }
// the 4 * C elements of lane t's four pixels, widened
template <int C>
RFX_DEV void k0_aov_load4(const void *base, bool half, size_t t, float *v) {
    if (!half) {
        const uint4 *p = (const uint4 *)base + t * C;
#pragma unroll
        for (int i = 0; i < C; i++) {
            const uint4 w = p[i];
            v[4 * i] = __uint_as_float(w.x); v[4 * i + 1] = __uint_as_float(w.y); v[4 * i + 2] = __uint_as_float(w.z); v[4 * i + 3] = __uint_as_float(w.w);
        }
    } else if (C % 2 == 0) {
        const uint4 *p = (const uint4 *)base + t * (C / 2);
#pragma unroll
        for (int i = 0; i < C / 2; i++) {
            const uint4 w = p[i];
            k0_aov_widen2(w.x, v + 8 * i); k0_aov_widen2(w.y, v + 8 * i + 2); k0_aov_widen2(w.z, v + 8 * i + 4); k0_aov_widen2(w.w, v + 8 * i + 6);
        }
    } else {
        const uint2 *p = (const uint2 *)base + t * C;
#pragma unroll
        for (int i = 0; i < C; i++) {
            const uint2 w = p[i];
            k0_aov_widen2(w.x, v + 4 * i); k0_aov_widen2(w.y, v + 4 * i + 2);
        }
    }
}
// ... of an rgb(a) plane: always four channels out, alpha 1 where the plane has three
RFX_DEV void k0_aov_load4_rgba(const void *base, bool half, int channels, size_t t, float *v) {
    if (channels == 4) {
        k0_aov_load4<4>(base, half, t, v);
    } else {
        float c[12];
        k0_aov_load4<3>(base, half, t, c);
#pragma unroll
        for (int k = 0; k < 4; k++) { v[4 * k] = c[3 * k]; v[4 * k + 1] = c[3 * k + 1]; v[4 * k + 2] = c[3 * k + 2]; v[4 * k + 3] = 1.0f; }
    }
}
RFX_DEV float k0_aov_elem(const void *base, bool half, size_t i) { return half ? rfx_h2f(((const unsigned short *)base)[i]) : ((const float *)base)[i]; }
RFX_DEV uint4 k0_aov_gbuffer_texel(float depth, const float *rgba, uint32_t normal, float roughness, float metalness, const float *emissive) {
    if (depth == 1.0f) return make_uint4(0u, 0u, 0u, 0x3f800000u);  // the clear colour (0, 0, 0, 1)
    return make_uint4(k0_vec4_to_float(rgba[0], rgba[1], rgba[2], rgba[3]), normal, __float_as_uint(k0_color2float(roughness, metalness, 0.0f)),
                      k0_rgbe8(make_float3(emissive[0], emissive[1], emissive[2])));
}
RFX_DEV uint4 k0_aov_velocity_texel(float depth, float vx, float vy, uint32_t normal) {
    if (depth == 1.0f) return make_uint4(0u, 0u, 0u, 0x3f800000u);
    return make_uint4(__float_as_uint(vx), __float_as_uint(vy), normal, __float_as_uint(depth));
}
// ---- conventions in use (include/rfx.h "AOV conventions"): the planes as an engine writes them -> the depth and velocity the packers above take.
// Everything here is decided by wave-uniform branches on K0AovConv; the arithmetic is the header's, operation for operation (this file is built
// uncontracted), restated by tests/aov_convention_ref.py.
RFX_DEV bool k0_finite(float a) { return (__float_as_uint(a) & 0x7f800000u) != 0x7f800000u; }
RFX_DEV void k0_conv_mul(const float *M, float x, float y, float z, float *r) {  // mul(M, p)
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = ((M[i] * x + M[4 + i] * y) + M[8 + i] * z) + M[12 + i];
}
RFX_DEV float k0_conv_frag_z(float cz, float cw) { return ((0.5f * cz) / cw) + 0.5f; }  // VelocityDepthNormalMaterial.js:81
// One texel.  dp: the depth plane's widened texel (three values under POSITION, else one); (x, y): its frame coordinates, read only where the
// world point is rebuilt from uv and view Z; vel: in, the velocity plane's texel (UV, SCALED); out, the uv-space velocity.  -> gl_FragCoord.z,
// 1.0 where the texel is not covered.
RFX_DEV float k0_conv_pixel(const K0AovConv &v, const float *dp, int x, int y, bool want_velocity, float *vel) {
    float depth = dp[0], viewZ = 0.0f;
    if (v.depth_kind == RFX_AOV_DEPTH_POSITION) {
        float n[4];
        k0_conv_mul(v.VM, dp[0], dp[1], dp[2], n);
        const float fz = k0_conv_frag_z(n[2], n[3]);
        const bool background = v.has_background && dp[0] == v.background[0] && dp[1] == v.background[1] && dp[2] == v.background[2];
        const bool covered = k0_finite(dp[0]) && k0_finite(dp[1]) && k0_finite(dp[2]) && !background && n[3] > 0.0f && fz >= 0.0f && fz < 1.0f;
        depth = covered ? fz : 1.0f;
    } else if (v.depth_kind == RFX_AOV_DEPTH_VIEW_Z) {
        viewZ = -dp[0];
        const float fz = k0_conv_frag_z(v.P[10] * viewZ + v.P[14], v.P[11] * viewZ + v.P[15]);
        const bool covered = k0_finite(dp[0]) && dp[0] > 0.0f && fz >= 0.0f && fz < 1.0f;
        depth = covered ? fz : 1.0f;
    }
    if (!want_velocity) return depth;
    if (v.velocity_kind == RFX_AOV_VELOCITY_SCALED) {
        vel[0] = vel[0] * v.scale[0];
        vel[1] = vel[1] * v.scale[1];
    } else if (v.velocity_kind == RFX_AOV_VELOCITY_CAMERAS) {
        float w[4] = {dp[0], dp[1], dp[2], 1.0f};
        if (v.depth_kind != RFX_AOV_DEPTH_POSITION) {
            if (v.depth_kind == RFX_AOV_DEPTH_FRAGCOORD) viewZ = rfx_depth_to_view_z(dp[0], v.near_, v.far_, v.perspective != 0);
            const float u = ((float)x + 0.5f) / (float)v.W, uv_v = ((float)y + 0.5f) / (float)v.H;
            // getViewPosition ssgi_utils.frag:17-24, as K1 evaluates it
            const float clipW = v.P[11] * viewZ + v.P[15];
            const float4 pp = rfx_mat_mul(v.Pi, ((u - 0.5f) * 2.0f) * clipW, ((uv_v - 0.5f) * 2.0f) * clipW, ((viewZ - 0.5f) * 2.0f) * clipW, 1.0f * clipW);
            k0_conv_mul(v.C, pp.x, pp.y, viewZ, w);
        }
        float n[4], p[4];
        k0_conv_mul(v.VM, w[0], w[1], w[2], n);
        k0_conv_mul(v.PVM, w[0], w[1], w[2], p);
        // VelocityDepthNormalMaterial.js:76-79
        const float pos0x = (p[0] / p[3]) * 0.5f + 0.5f, pos0y = (p[1] / p[3]) * 0.5f + 0.5f;
        const float pos1x = (n[0] / n[3]) * 0.5f + 0.5f, pos1y = (n[1] / n[3]) * 0.5f + 0.5f;
        vel[0] = pos1x - pos0x;
        vel[1] = pos1y - pos0y;
    }
    return depth;
}
RFX_DEV float3 k0_conv_normal(const K0AovConv &v, float3 n) {  // camera space -> world space
    if (v.normal_space != RFX_AOV_NORMAL_VIEW) return n;
    const float *C = v.C;
    return make_float3((C[0] * n.x + C[4] * n.y) + C[8] * n.z, (C[1] * n.x + C[5] * n.y) + C[9] * n.z, (C[2] * n.x + C[6] * n.y) + C[10] * n.z);
}
// the frame coordinates of the segment's pixel i: one integer divide per lane, the lane's other pixels step with a row wrap
RFX_DEV bool k0_conv_needs_xy(const K0AovConv &v, bool want_velocity) {
    return want_velocity && v.velocity_kind == RFX_AOV_VELOCITY_CAMERAS && v.depth_kind != RFX_AOV_DEPTH_POSITION;
}
RFX_DEV void k0_conv_xy(const K0AovConv &v, int i, int &x, int &y) {
    const int r = i / v.W;
    x = i - r * v.W;
    y = v.row0 + r;
}
RFX_DEV void k0_conv_step(const K0AovConv &v, int &x, int &y) {
    if (++x == v.W) { x = 0; y++; }
}
// lane g's four pixels: depth plane (and velocity plane, where the kind has one) -> d[4], vel[8]
template <int SET>
RFX_DEV void k0_conv_group(const K0AovConvArgs &A, size_t g, float *d, float *vel) {
    const K0AovConv &v = A.v;
    const bool want = A.velocity != nullptr, hd = k0_aov_half<SET>(A, RFX_AOV_DEPTH);
    float dp[12];
    if (v.depth_kind == RFX_AOV_DEPTH_POSITION) {
        k0_aov_load4<3>(A.plane[RFX_AOV_DEPTH], hd, g, dp);
    } else {
        float z[4];
        k0_aov_load4<1>(A.plane[RFX_AOV_DEPTH], hd, g, z);
#pragma unroll
        for (int k = 0; k < 4; k++) { dp[3 * k] = z[k]; dp[3 * k + 1] = 0.0f; dp[3 * k + 2] = 0.0f; }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) vel[k] = 0.0f;
    if (want && v.velocity_kind != RFX_AOV_VELOCITY_CAMERAS) k0_aov_load4<2>(A.plane[RFX_AOV_VELOCITY], k0_aov_half<SET>(A, RFX_AOV_VELOCITY), g, vel);
    int x = 0, y = 0;
    if (k0_conv_needs_xy(v, want)) k0_conv_xy(v, 4 * (int)g, x, y);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        d[k] = k0_conv_pixel(v, dp + 3 * k, x, y, want, vel + 2 * k);
        k0_conv_step(v, x, y);
    }
}
template <bool CONV>
struct K0AovBlock { typedef K0AovArgs type; };
template <>
struct K0AovBlock<true> { typedef K0AovConvArgs type; };
// CONV false: the default, on K0AovArgs alone — its source path is the one this kernel had before the conventions
template <int SET, bool CONV>
__global__ __launch_bounds__(RFX_K0_AOV_BLOCK) void k0_aov_pack(typename K0AovBlock<CONV>::type A) {
    const int t = blockIdx.x * RFX_K0_AOV_BLOCK + threadIdx.x;
    const bool packs = A.gbuffer || A.velocity;
    if (t < A.groups) {
        const size_t g = (size_t)t;
        float d[4], cv[8];
        if constexpr (CONV) k0_conv_group<SET>(A, g, d, cv);
        else k0_aov_load4<1>(A.plane[RFX_AOV_DEPTH], k0_aov_half<SET>(A, RFX_AOV_DEPTH), g, d);
        float *od = A.depth + g * 4;  // (dword-aligned only when the segment's first texel is not a multiple of four: four dwords, one store where the target allows)
        od[0] = d[0]; od[1] = d[1]; od[2] = d[2]; od[3] = d[3];
        uint32_t nrm[4] = {0u, 0u, 0u, 0u};
        if (packs) {
            float n[12];
            k0_aov_load4<3>(A.plane[RFX_AOV_NORMAL], k0_aov_half<SET>(A, RFX_AOV_NORMAL), g, n);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if constexpr (CONV) nrm[k] = k0_pack_normal(k0_conv_normal(A.v, make_float3(n[3 * k], n[3 * k + 1], n[3 * k + 2])));
                else nrm[k] = k0_pack_normal(make_float3(n[3 * k], n[3 * k + 1], n[3 * k + 2]));
            }
        }
        if (A.gbuffer) {
            float c[16], r[4], m[4], e[12];
            k0_aov_load4_rgba(A.plane[RFX_AOV_DIFFUSE], k0_aov_half<SET>(A, RFX_AOV_DIFFUSE), A.diffuse_ch, g, c);
            k0_aov_load4<1>(A.plane[RFX_AOV_ROUGHNESS], k0_aov_half<SET>(A, RFX_AOV_ROUGHNESS), g, r);
            k0_aov_load4<1>(A.plane[RFX_AOV_METALNESS], k0_aov_half<SET>(A, RFX_AOV_METALNESS), g, m);
            k0_aov_load4<3>(A.plane[RFX_AOV_EMISSIVE], k0_aov_half<SET>(A, RFX_AOV_EMISSIVE), g, e);
            uint4 *o = A.gbuffer + g * 4;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = k0_aov_gbuffer_texel(d[k], c + 4 * k, nrm[k], r[k], m[k], e + 3 * k);
        }
        if (A.velocity) {
            float v[8];
            if constexpr (CONV) {
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = cv[k];
            } else k0_aov_load4<2>(A.plane[RFX_AOV_VELOCITY], k0_aov_half<SET>(A, RFX_AOV_VELOCITY), g, v);
            uint4 *o = A.velocity + g * 4;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = k0_aov_velocity_texel(d[k], v[2 * k], v[2 * k + 1], nrm[k]);
        }
        if (A.direct) {
            float q[16];
            k0_aov_load4_rgba(A.plane[RFX_AOV_DIRECT], k0_aov_half<SET>(A, RFX_AOV_DIRECT), A.direct_ch, g, q);
            uint4 *o = A.direct + g * 4;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = make_uint4(__float_as_uint(q[4 * k]), __float_as_uint(q[4 * k + 1]), __float_as_uint(q[4 * k + 2]), __float_as_uint(q[4 * k + 3]));
        }
    } else if (t == A.groups) {
        int cx = 0, cy = 0;
        if constexpr (CONV) {
            if (k0_conv_needs_xy(A.v, A.velocity != nullptr)) k0_conv_xy(A.v, A.tail_start, cx, cy);
        }
        for (int k = 0; k < A.tail_pixels; k++) {
            const size_t px = (size_t)A.tail_start + k;
            float d, cv[2] = {0.0f, 0.0f};
            if constexpr (CONV) {
                const bool hd = k0_aov_half<SET>(A, RFX_AOV_DEPTH), want = A.velocity != nullptr;
                const void *pd = A.plane[RFX_AOV_DEPTH];
                float dp[3] = {0.0f, 0.0f, 0.0f};
                if (A.v.depth_kind == RFX_AOV_DEPTH_POSITION) { dp[0] = k0_aov_elem(pd, hd, 3 * px); dp[1] = k0_aov_elem(pd, hd, 3 * px + 1); dp[2] = k0_aov_elem(pd, hd, 3 * px + 2); }
                else dp[0] = k0_aov_elem(pd, hd, px);
                if (want && A.v.velocity_kind != RFX_AOV_VELOCITY_CAMERAS) {
                    const bool h = k0_aov_half<SET>(A, RFX_AOV_VELOCITY);
                    cv[0] = k0_aov_elem(A.plane[RFX_AOV_VELOCITY], h, 2 * px);
                    cv[1] = k0_aov_elem(A.plane[RFX_AOV_VELOCITY], h, 2 * px + 1);
                }
                d = k0_conv_pixel(A.v, dp, cx, cy, want, cv);
                k0_conv_step(A.v, cx, cy);
            } else d = k0_aov_elem(A.plane[RFX_AOV_DEPTH], k0_aov_half<SET>(A, RFX_AOV_DEPTH), px);
            A.depth[px] = d;
            uint32_t nrm = 0u;
            if (packs) {
                const bool h = k0_aov_half<SET>(A, RFX_AOV_NORMAL);
                const void *p = A.plane[RFX_AOV_NORMAL];
                const float3 n = make_float3(k0_aov_elem(p, h, 3 * px), k0_aov_elem(p, h, 3 * px + 1), k0_aov_elem(p, h, 3 * px + 2));
                if constexpr (CONV) nrm = k0_pack_normal(k0_conv_normal(A.v, n));
                else nrm = k0_pack_normal(n);
            }
            if (A.gbuffer) {
                const bool hc = k0_aov_half<SET>(A, RFX_AOV_DIFFUSE), he = k0_aov_half<SET>(A, RFX_AOV_EMISSIVE);
                const void *pc = A.plane[RFX_AOV_DIFFUSE], *pe = A.plane[RFX_AOV_EMISSIVE];
                const size_t ci = px * A.diffuse_ch;
                const float c[4] = {k0_aov_elem(pc, hc, ci), k0_aov_elem(pc, hc, ci + 1), k0_aov_elem(pc, hc, ci + 2), A.diffuse_ch == 4 ? k0_aov_elem(pc, hc, ci + 3) : 1.0f};
                const float e[3] = {k0_aov_elem(pe, he, 3 * px), k0_aov_elem(pe, he, 3 * px + 1), k0_aov_elem(pe, he, 3 * px + 2)};
                A.gbuffer[px] = k0_aov_gbuffer_texel(d, c, nrm, k0_aov_elem(A.plane[RFX_AOV_ROUGHNESS], k0_aov_half<SET>(A, RFX_AOV_ROUGHNESS), px),
                                                     k0_aov_elem(A.plane[RFX_AOV_METALNESS], k0_aov_half<SET>(A, RFX_AOV_METALNESS), px), e);
            }
            if (A.velocity) {
                if constexpr (CONV) {
                    A.velocity[px] = k0_aov_velocity_texel(d, cv[0], cv[1], nrm);
                } else {
                    const bool h = k0_aov_half<SET>(A, RFX_AOV_VELOCITY);
                    const void *p = A.plane[RFX_AOV_VELOCITY];
                    A.velocity[px] = k0_aov_velocity_texel(d, k0_aov_elem(p, h, 2 * px), k0_aov_elem(p, h, 2 * px + 1), nrm);
                }
            }
            if (A.direct) {
                const bool h = k0_aov_half<SET>(A, RFX_AOV_DIRECT);
                const void *p = A.plane[RFX_AOV_DIRECT];
                const size_t qi = px * A.direct_ch;
                A.direct[px] = make_uint4(__float_as_uint(k0_aov_elem(p, h, qi)), __float_as_uint(k0_aov_elem(p, h, qi + 1)), __float_as_uint(k0_aov_elem(p, h, qi + 2)),
                                          __float_as_uint(A.direct_ch == 4 ? k0_aov_elem(p, h, qi + 3) : 1.0f));
            }
        }
    }
}

// ---------------------------------------------------------------- K0 AOV pack over device planes, for rfx_stage_aov_device (include/rfx.h "device planes")
// k0_aov_pack's work on planes that lie where their producer left them: the element of column x, segment row y, channel ch of a plane sits
// sx x + sy y + sc ch elements from its base, strides of any sign or 0.  Rows have pitch, so the decomposition is two-dimensional: a workgroup is
// RFX_K0_DEV_BX lanes along a row by RFX_K0_DEV_BY rows, lane l < groups_x of a row owns its pixels [4 l, 4 l + 4), lane groups_x the W mod 4
// pixels from tail_x on, element by element; no group straddles rows and the frame's (x, y) are at hand for the conventions (no k0_conv_xy).
// Each plane's layout class is uniform over the launch (rfx_launch.h rfx_aov_device_plan_for decides it, with the alignment it needs) and
// branched on per wave, as SET 2 does with half_mask:
//   INTERLEAVED  the lane's 4 C elements are one run: C 16-byte loads (halves: C 8-byte loads), lane to lane 16 C bytes on — k0_aov_load4's access;
//   PLANAR       per channel the lane's four elements are one run: one 16-byte (8-byte) load, lane to lane 16 (8) bytes on — a wave reads
//                1 KiB (512 B) of consecutive bytes per instruction;
//   ELEMENT      one element per load.
// The slots leave as in k0_aov_pack: four 16-byte stores per lane and slot, the four depth values.  The arithmetic is the same device functions
// on the same widened values: the texels are k0_aov_pack's bit for bit.
RFX_DEV float k0s_elem(const K0AovStridedPlane &p, bool half, long long i) {
    return half ? rfx_h2f(((const unsigned short *)p.base)[i]) : ((const float *)p.base)[i];
}
// N pixels from column x0 of row y, pixel-major: v[C k + ch].  N 4: by the plane's layout; N 1 (the tail): the element form
template <int C, int N>
RFX_DEV void k0s_load(const K0AovStridedPlane &p, int layout, bool half, int x0, int y, float *v) {
    const long long row = (long long)y * p.sy;
    if (N == 4 && layout == RFX_AOV_LAYOUT_INTERLEAVED) {
        const long long at = row + (long long)x0 * C;
        if (!half) {
            const uint4 *q = (const uint4 *)((const float *)p.base + at);
#pragma unroll
            for (int i = 0; i < C; i++) {
                const uint4 w = q[i];
                v[4 * i] = __uint_as_float(w.x); v[4 * i + 1] = __uint_as_float(w.y); v[4 * i + 2] = __uint_as_float(w.z); v[4 * i + 3] = __uint_as_float(w.w);
            }
        } else {
            const uint2 *q = (const uint2 *)((const unsigned short *)p.base + at);
#pragma unroll
            for (int i = 0; i < C; i++) {
                const uint2 w = q[i];
                k0_aov_widen2(w.x, v + 4 * i); k0_aov_widen2(w.y, v + 4 * i + 2);
            }
        }
    } else if (N == 4 && layout == RFX_AOV_LAYOUT_PLANAR) {
#pragma unroll
        for (int ch = 0; ch < C; ch++) {
            const long long at = row + (long long)ch * p.sc + x0;
            float f[4];
            if (!half) {
                const uint4 w = *(const uint4 *)((const float *)p.base + at);
                f[0] = __uint_as_float(w.x); f[1] = __uint_as_float(w.y); f[2] = __uint_as_float(w.z); f[3] = __uint_as_float(w.w);
            } else {
                const uint2 w = *(const uint2 *)((const unsigned short *)p.base + at);
                k0_aov_widen2(w.x, f); k0_aov_widen2(w.y, f + 2);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) v[C * k + ch] = f[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; k++)
#pragma unroll
            for (int ch = 0; ch < C; ch++) v[C * k + ch] = k0s_elem(p, half, row + (long long)(x0 + k) * p.sx + (long long)ch * p.sc);
    }
}
// ... of an rgb(a) plane: always four channels out, alpha 1 where the plane has three
template <int N>
RFX_DEV void k0s_load_rgba(const K0AovStridedPlane &p, int layout, bool half, int channels, int x0, int y, float *v) {
    if (channels == 4) {
        k0s_load<4, N>(p, layout, half, x0, y, v);
    } else {
        float c[3 * N];
        k0s_load<3, N>(p, layout, half, x0, y, c);
#pragma unroll
        for (int k = 0; k < N; k++) { v[4 * k] = c[3 * k]; v[4 * k + 1] = c[3 * k + 1]; v[4 * k + 2] = c[3 * k + 2]; v[4 * k + 3] = 1.0f; }
    }
}
// the N pixels from column x0 of segment row y
template <bool CONV, int N, class Block>
RFX_DEV void k0s_pixels(const Block &A, int x0, int y) {
    const auto lay = [&](int i) { return (int)((A.layouts >> (2 * i)) & 3u); };
    const auto half = [&](int i) { return ((A.half_mask >> i) & 1u) != 0u; };
    const size_t first = (size_t)y * (size_t)A.W + (size_t)x0;
    float d[N], cv[2 * N];
    if constexpr (CONV) {
        const K0AovConv &v = A.v;
        const bool want = A.velocity != nullptr;
        float dp[3 * N];
        if (v.depth_kind == RFX_AOV_DEPTH_POSITION) {
            k0s_load<3, N>(A.plane[RFX_AOV_DEPTH], lay(RFX_AOV_DEPTH), half(RFX_AOV_DEPTH), x0, y, dp);
        } else {
            float z[N];
            k0s_load<1, N>(A.plane[RFX_AOV_DEPTH], lay(RFX_AOV_DEPTH), half(RFX_AOV_DEPTH), x0, y, z);
#pragma unroll
            for (int k = 0; k < N; k++) { dp[3 * k] = z[k]; dp[3 * k + 1] = 0.0f; dp[3 * k + 2] = 0.0f; }
        }
#pragma unroll
        for (int k = 0; k < 2 * N; k++) cv[k] = 0.0f;
        if (want && v.velocity_kind != RFX_AOV_VELOCITY_CAMERAS)
            k0s_load<2, N>(A.plane[RFX_AOV_VELOCITY], lay(RFX_AOV_VELOCITY), half(RFX_AOV_VELOCITY), x0, y, cv);
#pragma unroll
        for (int k = 0; k < N; k++) d[k] = k0_conv_pixel(v, dp + 3 * k, x0 + k, v.row0 + y, want, cv + 2 * k);
    } else k0s_load<1, N>(A.plane[RFX_AOV_DEPTH], lay(RFX_AOV_DEPTH), half(RFX_AOV_DEPTH), x0, y, d);
    float *od = A.depth + first;
#pragma unroll
    for (int k = 0; k < N; k++) od[k] = d[k];
    uint32_t nrm[N];
#pragma unroll
    for (int k = 0; k < N; k++) nrm[k] = 0u;
    if (A.gbuffer || A.velocity) {
        float n[3 * N];
        k0s_load<3, N>(A.plane[RFX_AOV_NORMAL], lay(RFX_AOV_NORMAL), half(RFX_AOV_NORMAL), x0, y, n);
#pragma unroll
        for (int k = 0; k < N; k++) {
            if constexpr (CONV) nrm[k] = k0_pack_normal(k0_conv_normal(A.v, make_float3(n[3 * k], n[3 * k + 1], n[3 * k + 2])));
            else nrm[k] = k0_pack_normal(make_float3(n[3 * k], n[3 * k + 1], n[3 * k + 2]));
        }
    }
    if (A.gbuffer) {
        float c[4 * N], r[N], m[N], e[3 * N];
        k0s_load_rgba<N>(A.plane[RFX_AOV_DIFFUSE], lay(RFX_AOV_DIFFUSE), half(RFX_AOV_DIFFUSE), A.diffuse_ch, x0, y, c);
        k0s_load<1, N>(A.plane[RFX_AOV_ROUGHNESS], lay(RFX_AOV_ROUGHNESS), half(RFX_AOV_ROUGHNESS), x0, y, r);
        k0s_load<1, N>(A.plane[RFX_AOV_METALNESS], lay(RFX_AOV_METALNESS), half(RFX_AOV_METALNESS), x0, y, m);
        k0s_load<3, N>(A.plane[RFX_AOV_EMISSIVE], lay(RFX_AOV_EMISSIVE), half(RFX_AOV_EMISSIVE), x0, y, e);
        uint4 *o = A.gbuffer + first;
#pragma unroll
        for (int k = 0; k < N; k++) o[k] = k0_aov_gbuffer_texel(d[k], c + 4 * k, nrm[k], r[k], m[k], e + 3 * k);
    }
    if (A.velocity) {
        float v[2 * N];
        if constexpr (CONV) {
#pragma unroll
            for (int k = 0; k < 2 * N; k++) v[k] = cv[k];
        } else k0s_load<2, N>(A.plane[RFX_AOV_VELOCITY], lay(RFX_AOV_VELOCITY), half(RFX_AOV_VELOCITY), x0, y, v);
        uint4 *o = A.velocity + first;
#pragma unroll
        for (int k = 0; k < N; k++) o[k] = k0_aov_velocity_texel(d[k], v[2 * k], v[2 * k + 1], nrm[k]);
    }
    if (A.direct) {
        float q[4 * N];
        k0s_load_rgba<N>(A.plane[RFX_AOV_DIRECT], lay(RFX_AOV_DIRECT), half(RFX_AOV_DIRECT), A.direct_ch, x0, y, q);
        uint4 *o = A.direct + first;
#pragma unroll
        for (int k = 0; k < N; k++) o[k] = make_uint4(__float_as_uint(q[4 * k]), __float_as_uint(q[4 * k + 1]), __float_as_uint(q[4 * k + 2]), __float_as_uint(q[4 * k + 3]));
    }
}
template <bool CONV>
struct K0AovStridedBlock { typedef K0AovStridedArgs type; };
template <>
struct K0AovStridedBlock<true> { typedef K0AovStridedConvArgs type; };
template <bool CONV>
__global__ __launch_bounds__(RFX_K0_DEV_BX * RFX_K0_DEV_BY) void k0_aov_pack_strided(typename K0AovStridedBlock<CONV>::type A) {
    const int lane = blockIdx.x * RFX_K0_DEV_BX + threadIdx.x, y = blockIdx.y * RFX_K0_DEV_BY + threadIdx.y;
    if (lane >= A.lanes_x || y >= A.rows) return;
    if (lane < A.groups_x) {
        k0s_pixels<CONV, 4>(A, 4 * lane, y);
    } else {
        for (int k = 0; k < A.tail_pixels; k++) k0s_pixels<CONV, 1>(A, A.tail_x + k, y);
    }
}

}  // namespace

hipError_t rfx_launch_pack_gbuffer(int W, int rows, const float *diffuse, const float *normal, const float *roughness, const float *metalness,
                                   const float *emissive, const float *depth, void *out, hipStream_t stream) {
    K0GBuffer A = {W, rows, diffuse, normal, roughness, metalness, emissive, depth, (uint4 *)out};
    dim3 block(64, 4), grid((W + 63) / 64, (rows + 3) / 4);
    hipLaunchKernelGGL(k0_pack_gbuffer, grid, block, 0, stream, A);
    return hipGetLastError();
}
// the three specialisations: no half plane, the typed set (every plane the segment reads but velocity and depth), any other mix; each of them
// once more with conventions in use
template <bool CONV, class Block>
static void k0_aov_launch(int set, const Block &B, int blocks, hipStream_t stream) {
    if (set == 0) hipLaunchKernelGGL((k0_aov_pack<0, CONV>), dim3(blocks), dim3(RFX_K0_AOV_BLOCK), 0, stream, B);
    else if (set == 1) hipLaunchKernelGGL((k0_aov_pack<1, CONV>), dim3(blocks), dim3(RFX_K0_AOV_BLOCK), 0, stream, B);
    else hipLaunchKernelGGL((k0_aov_pack<2, CONV>), dim3(blocks), dim3(RFX_K0_AOV_BLOCK), 0, stream, B);
}
hipError_t rfx_launch_k0_aov(const K0AovArgs &A, int blocks, hipStream_t stream, const K0AovConv *conv) {
    if (!A.plane[RFX_AOV_DEPTH] || !A.depth || blocks <= 0) return hipErrorInvalidValue;
    unsigned int given = 0;
    for (int i = 0; i < RFX_AOV_PLANES; i++) given |= A.plane[i] ? 1u << i : 0u;
    const unsigned int halves = A.half_mask & given, typed = given & ~((1u << RFX_AOV_VELOCITY) | (1u << RFX_AOV_DEPTH));
    const int set = halves == 0u ? 0 : halves == typed ? 1 : 2;
    if (conv) {
        if (conv->W <= 0 || conv->H <= 0) return hipErrorInvalidValue;
        if (A.velocity && conv->velocity_kind != RFX_AOV_VELOCITY_CAMERAS && !A.plane[RFX_AOV_VELOCITY]) return hipErrorInvalidValue;
        K0AovConvArgs B;
        static_cast<K0AovArgs &>(B) = A;
        B.v = *conv;
        k0_aov_launch<true>(set, B, blocks, stream);
    } else k0_aov_launch<false>(set, A, blocks, stream);
    return hipGetLastError();
}
hipError_t rfx_launch_k0_aov_strided(const K0AovStridedArgs &A, int grid_x, int grid_y, hipStream_t stream, const K0AovConv *conv) {
    if (!A.plane[RFX_AOV_DEPTH].base || !A.depth || grid_x <= 0 || grid_y <= 0 || A.W <= 0 || A.rows <= 0) return hipErrorInvalidValue;
    if (A.groups_x != A.W / 4 || A.tail_x != 4 * A.groups_x || A.tail_pixels != A.W - A.tail_x || A.lanes_x != A.groups_x + (A.tail_pixels ? 1 : 0))
        return hipErrorInvalidValue;
    const dim3 grid(grid_x, grid_y), block(RFX_K0_DEV_BX, RFX_K0_DEV_BY);
    if (conv) {
        if (conv->W <= 0 || conv->H <= 0) return hipErrorInvalidValue;
        if (A.velocity && conv->velocity_kind != RFX_AOV_VELOCITY_CAMERAS && !A.plane[RFX_AOV_VELOCITY].base) return hipErrorInvalidValue;
        K0AovStridedConvArgs B;
        static_cast<K0AovStridedArgs &>(B) = A;
        B.v = *conv;
        hipLaunchKernelGGL((k0_aov_pack_strided<true>), grid, block, 0, stream, B);
    } else hipLaunchKernelGGL((k0_aov_pack_strided<false>), grid, block, 0, stream, A);
    return hipGetLastError();
}
hipError_t rfx_launch_pack_velocity(int W, int rows, const float *velocity, const float *normal, const float *depth, void *out, hipStream_t stream) {
    K0Velocity A = {W, rows, velocity, normal, depth, (uint4 *)out};
    dim3 block(64, 4), grid((W + 63) / 64, (rows + 3) / 4);
    hipLaunchKernelGGL(k0_pack_velocity, grid, block, 0, stream, A);
    return hipGetLastError();
}
