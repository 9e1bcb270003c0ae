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
// One pass over the flat pixel run of a segment (rfx_launch.h rfx_aov_plan_for): 44 .. 76 B in per pixel, 52 B out.  Lane t owns the four
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
template <int SET>
__global__ __launch_bounds__(RFX_K0_AOV_BLOCK) void k0_aov_pack(K0AovArgs A) {
    const int t = blockIdx.x * RFX_K0_AOV_BLOCK + threadIdx.x;
    const bool packs = A.gbuffer || A.velocity;
    if (t < A.groups) {
        const size_t g = (size_t)t;
        float d[4];
        k0_aov_load4<1>(A.plane[RFX_AOV_DEPTH], k0_aov_half<SET>(A, RFX_AOV_DEPTH), g, d);
        float *od = A.depth + g * 4;  // (dword-aligned only when the segment's first texel is not a multiple of four: four dwords, one store where the target allows)
        od[0] = d[0]; od[1] = d[1]; od[2] = d[2]; od[3] = d[3];
        uint32_t nrm[4] = {0u, 0u, 0u, 0u};
        if (packs) {
            float n[12];
            k0_aov_load4<3>(A.plane[RFX_AOV_NORMAL], k0_aov_half<SET>(A, RFX_AOV_NORMAL), g, n);
#pragma unroll
            for (int k = 0; k < 4; k++) nrm[k] = k0_pack_normal(make_float3(n[3 * k], n[3 * k + 1], n[3 * k + 2]));
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
            k0_aov_load4<2>(A.plane[RFX_AOV_VELOCITY], k0_aov_half<SET>(A, RFX_AOV_VELOCITY), g, v);
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
        for (int k = 0; k < A.tail_pixels; k++) {
            const size_t px = (size_t)A.tail_start + k;
            const float d = k0_aov_elem(A.plane[RFX_AOV_DEPTH], k0_aov_half<SET>(A, RFX_AOV_DEPTH), px);
            A.depth[px] = d;
            uint32_t nrm = 0u;
            if (packs) {
                const bool h = k0_aov_half<SET>(A, RFX_AOV_NORMAL);
                const void *p = A.plane[RFX_AOV_NORMAL];
                nrm = k0_pack_normal(make_float3(k0_aov_elem(p, h, 3 * px), k0_aov_elem(p, h, 3 * px + 1), k0_aov_elem(p, h, 3 * px + 2)));
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
                const bool h = k0_aov_half<SET>(A, RFX_AOV_VELOCITY);
                const void *p = A.plane[RFX_AOV_VELOCITY];
                A.velocity[px] = k0_aov_velocity_texel(d, k0_aov_elem(p, h, 2 * px), k0_aov_elem(p, h, 2 * px + 1), nrm);
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

// ---------------------------------------------------------------- CubeToEquirectEnvPass (src/ssgi/pass/CubeToEquirectEnvPass.js:21-42)
// One `textureCube(cubeMap, dir)` per texel of the equirectangular render target, with the lookup rules of the oracle's GL (measured
// bit-exact on every interior lookup, oracle/glref/probes/probe_cube.py): major axis by >= in x, y, z order,
// (s, t) = (sc * (1 / ma)) * 0.5 + 0.5, seamless edges (a footprint texel beyond the face edge is the neighbouring face's texel the
// extended position projects to; beyond a corner: the average of the other three), blend = fused lerp in x, then in y.
struct K0Cube {
    const float4 *chain;  // level l at chain + off[l]: six faces +X -X +Y -Y +Z -Z, each (S >> l) x (S >> l), row j = t
    unsigned int off[14];
    int S, levels;        // levels = 1: the cube has no mip chain (minFilter LinearFilter)
    float4 *out;
    int W, H;
    UvPlanes uv;
};
struct CubeLevel { const float4 *faces; int S; };
struct CubeFace { int face; float s, t; };
RFX_DEV CubeFace k0_cube_face(float x, float y, float z) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    CubeFace r;
    float sc, tc, ma;
    if (ax >= ay && ax >= az) { r.face = x >= 0.0f ? 0 : 1; sc = x >= 0.0f ? -z : z; tc = -y; ma = ax; }
    else if (ay >= az) { r.face = y >= 0.0f ? 2 : 3; sc = x; tc = y >= 0.0f ? z : -z; ma = ay; }
    else { r.face = z >= 0.0f ? 4 : 5; sc = z >= 0.0f ? x : -x; tc = -y; ma = az; }
    const float ima = 1.0f / ma;  // IEEE division, as the GL's
    r.s = (sc * ima) * 0.5f + 0.5f;
    r.t = (tc * ima) * 0.5f + 0.5f;
    return r;
}
// texel (i, j) of the footprint on `face`; false for the texel beyond a corner
RFX_DEV bool k0_cube_texel(const CubeLevel &A, int face, int i, int j, float4 &out) {
    const int S = A.S;
    const bool oi = i < 0 || i >= S, oj = j < 0 || j >= S;
    if (oi && oj) return false;
    if (oi || oj) {  // the centre of the would-be texel, projected onto the neighbouring face
        const float a = (((float)i + 0.5f) / (float)S) * 2.0f - 1.0f, b = (((float)j + 0.5f) / (float)S) * 2.0f - 1.0f;
        float x, y, z;
        switch (face) {
        case 0: x = 1.0f; y = -b; z = -a; break;
        case 1: x = -1.0f; y = -b; z = a; break;
        case 2: x = a; y = 1.0f; z = b; break;
        case 3: x = a; y = -1.0f; z = -b; break;
        case 4: x = a; y = -b; z = 1.0f; break;
        default: x = -a; y = -b; z = -1.0f; break;
        }
        const CubeFace n = k0_cube_face(x, y, z);
        face = n.face;
        i = min(max((int)floorf(n.s * (float)S), 0), S - 1);
        j = min(max((int)floorf(n.t * (float)S), 0), S - 1);
    }
    out = A.faces[((size_t)face * S + j) * S + i];
    return true;
}
// seamless bilinear lookup of one level
RFX_DEV float4 k0_cube_linear(const CubeLevel &L, float dx, float dy, float dz) {
    const CubeFace f = k0_cube_face(dx, dy, dz);
    const float cu = f.s * (float)L.S - 0.5f, cv = f.t * (float)L.S - 0.5f;
    const float fi = floorf(cu), fj = floorf(cv), fu = cu - fi, fv = cv - fj;
    const int i0 = (int)fi, j0 = (int)fj;
    float4 q[4];
    bool have[4];
    have[0] = k0_cube_texel(L, f.face, i0, j0, q[0]);
    have[1] = k0_cube_texel(L, f.face, i0 + 1, j0, q[1]);
    have[2] = k0_cube_texel(L, f.face, i0, j0 + 1, q[2]);
    have[3] = k0_cube_texel(L, f.face, i0 + 1, j0 + 1, q[3]);
    int missing = -1;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (!have[k]) missing = k;
    if (missing >= 0) {  // beyond the corner: the average of the three texels that exist (summed in footprint order)
        float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k != missing) { sum.x += q[k].x; sum.y += q[k].y; sum.z += q[k].z; sum.w += q[k].w; }
        const float4 avg = make_float4(sum.x / 3.0f, sum.y / 3.0f, sum.z / 3.0f, sum.w / 3.0f);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k == missing) q[k] = avg;
    }
    float4 o;
    float top, bot;
    top = __fmaf_rn(fu, q[1].x - q[0].x, q[0].x); bot = __fmaf_rn(fu, q[3].x - q[2].x, q[2].x); o.x = __fmaf_rn(fv, bot - top, top);
    top = __fmaf_rn(fu, q[1].y - q[0].y, q[0].y); bot = __fmaf_rn(fu, q[3].y - q[2].y, q[2].y); o.y = __fmaf_rn(fv, bot - top, top);
    top = __fmaf_rn(fu, q[1].z - q[0].z, q[0].z); bot = __fmaf_rn(fu, q[3].z - q[2].z, q[2].z); o.z = __fmaf_rn(fv, bot - top, top);
    top = __fmaf_rn(fu, q[1].w - q[0].w, q[0].w); bot = __fmaf_rn(fu, q[3].w - q[2].w, q[2].w); o.w = __fmaf_rn(fv, bot - top, top);
    return o;
}
// the pass's direction at fragment (x, y).  A one-off set-up pass whose direction error is multiplied by the face size in texels and the
// cube's local contrast: the library sin / cos (<= 1-2 ulp), not the hardware approximations the per-frame kernels use
RFX_DEV float3 k0_cube_direction(const UvPlanes &uv, int x, int y) {
    const float PI = 3.1415926535897932384626433832795f;
    const float u = rfx_frag_u(uv, x, y), v = rfx_frag_v(uv, y);
    const float longitude = ((u * 2.0f) * PI - PI) + PI / 2.0f, latitude = v * PI;
    const float sLat = sinf(latitude);
    return make_float3(-sinf(longitude) * sLat, -cosf(latitude), -cosf(longitude) * sLat);  // dir.y = -dir.y
}
RFX_DEV void k0_cube_components(int face, float3 p, float &sc, float &tc, float &ma) {
    switch (face) {
    case 0: sc = -p.z; tc = -p.y; ma = p.x; break;
    case 1: sc = p.z; tc = -p.y; ma = -p.x; break;
    case 2: sc = p.x; tc = p.z; ma = p.y; break;
    case 3: sc = p.x; tc = -p.z; ma = -p.y; break;
    case 4: sc = p.x; tc = -p.y; ma = p.z; break;
    default: sc = -p.x; tc = -p.y; ma = -p.z; break;
    }
}
// textureCube's implicit level of detail as the oracle's GL derives it: per pixel, from the direction differences within the pixel's own
// row and own column of its 2x2 quad, through the quotient rule on the pixel's own face; linear-mantissa log2
RFX_DEV float k0_cube_lod(float3 p, float3 ddx, float3 ddy, int S) {
    const CubeFace f = k0_cube_face(p.x, p.y, p.z);
    float sc, tc, ma, xsc, xtc, xma, ysc, ytc, yma;
    k0_cube_components(f.face, p, sc, tc, ma);
    k0_cube_components(f.face, ddx, xsc, xtc, xma);
    k0_cube_components(f.face, ddy, ysc, ytc, yma);
    const float ima = 1.0f / ma, k = (ima * ima) * 0.5f;
    const float dsx = (xsc * ma - sc * xma) * k, dtx = (xtc * ma - tc * xma) * k;
    const float dsy = (ysc * ma - sc * yma) * k, dty = (ytc * ma - tc * yma) * k;
    const float rho2 = fmaxf(dsx * dsx + dtx * dtx, dsy * dsy + dty * dty) * ((float)S * (float)S);
    const uint32_t bits = __float_as_uint(rho2);
    const float mant = __uint_as_float((bits & 0x7fffffu) | 0x3f800000u);
    return 0.5f * ((float)((int)((bits >> 23) & 0xffu) - 127) + (mant - 1.0f));
}
__global__ __launch_bounds__(256) void k0_cube_to_equirect(K0Cube A) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.W || y >= A.H) return;
    const float3 p = k0_cube_direction(A.uv, x, y);
    const CubeLevel base = {A.chain, A.S};
    float4 o;
    if (A.levels == 1) {
        o = k0_cube_linear(base, p.x, p.y, p.z);
    } else {
        const float3 pr = k0_cube_direction(A.uv, x ^ 1, y), pc = k0_cube_direction(A.uv, x, y ^ 1);
        const float3 ddx = (x & 1) ? make_float3(p.x - pr.x, p.y - pr.y, p.z - pr.z) : make_float3(pr.x - p.x, pr.y - p.y, pr.z - p.z);
        const float3 ddy = (y & 1) ? make_float3(p.x - pc.x, p.y - pc.y, p.z - pc.z) : make_float3(pc.x - p.x, pc.y - p.y, pc.z - p.z);
        float lod = k0_cube_lod(p, ddx, ddy, A.S);
        lod = fminf(fmaxf(lod, 0.0f), (float)(A.levels - 1));
        const float fl = floorf(lod), f = lod - fl;
        const int l0 = (int)fl, l1 = min(l0 + 1, A.levels - 1);
        const CubeLevel L0 = {A.chain + A.off[l0], max(A.S >> l0, 1)}, L1 = {A.chain + A.off[l1], max(A.S >> l1, 1)};
        const float4 c0 = k0_cube_linear(L0, p.x, p.y, p.z), c1 = k0_cube_linear(L1, p.x, p.y, p.z);
        o = make_float4(__fmaf_rn(f, c1.x - c0.x, c0.x), __fmaf_rn(f, c1.y - c0.y, c0.y), __fmaf_rn(f, c1.z - c0.z, c0.z), __fmaf_rn(f, c1.w - c0.w, c0.w));
    }
    A.out[(size_t)y * A.W + x] = o;
}
// one level of the cube's chain from the one above, per face (glGenerateMipmap on the oracle's GL: the 2x2 bilinear centre)
__global__ __launch_bounds__(256) void k0_cube_mip(const float4 *src, float4 *dst, int s0, int s1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 6 * s1 * s1) return;
    const int f = i / (s1 * s1), r = i - f * s1 * s1, y = r / s1, x = r - y * s1;
    const float4 *q = src + (size_t)f * s0 * s0;
    if (s0 & 1) {  // a level of odd size (a face that is not a power of two): the GL's LINEAR blit of the face at the target texel's centre, CLAMP_TO_EDGE
        int x0, x1, y0, y1;
        float wx, wy;
        rfx_linear_coord(((float)x + 0.5f) / (float)s1, (float)s0, s0, x0, x1, wx);
        rfx_linear_coord(((float)y + 0.5f) / (float)s1, (float)s0, s0, y0, y1, wy);
        const float4 t00 = q[(size_t)y0 * s0 + x0], t10 = q[(size_t)y0 * s0 + x1], t01 = q[(size_t)y1 * s0 + x0], t11 = q[(size_t)y1 * s0 + x1];
        dst[i] = make_float4(rfx_lerp(wy, rfx_lerp(wx, t00.x, t10.x), rfx_lerp(wx, t01.x, t11.x)), rfx_lerp(wy, rfx_lerp(wx, t00.y, t10.y), rfx_lerp(wx, t01.y, t11.y)),
                             rfx_lerp(wy, rfx_lerp(wx, t00.z, t10.z), rfx_lerp(wx, t01.z, t11.z)), rfx_lerp(wy, rfx_lerp(wx, t00.w, t10.w), rfx_lerp(wx, t01.w, t11.w)));
        return;
    }
    const float4 a = q[(size_t)(2 * y) * s0 + 2 * x], b = q[(size_t)(2 * y) * s0 + 2 * x + 1];
    const float4 c = q[(size_t)(2 * y + 1) * s0 + 2 * x], e = q[(size_t)(2 * y + 1) * s0 + 2 * x + 1];
    float4 o;
    o.x = rfx_lerp(0.5f, rfx_lerp(0.5f, a.x, b.x), rfx_lerp(0.5f, c.x, e.x));
    o.y = rfx_lerp(0.5f, rfx_lerp(0.5f, a.y, b.y), rfx_lerp(0.5f, c.y, e.y));
    o.z = rfx_lerp(0.5f, rfx_lerp(0.5f, a.z, b.z), rfx_lerp(0.5f, c.z, e.z));
    o.w = rfx_lerp(0.5f, rfx_lerp(0.5f, a.w, b.w), rfx_lerp(0.5f, c.w, e.w));
    dst[i] = o;
}

// ---------------------------------------------------------------- K7: export — the importer run in reverse (include/rfx.h rfx_export_params)
// A pure stream: 16 B in per pixel, 3 to 16 B out.  Lane t owns the four consecutive pixels [4 t, 4 t + 4) of the flat run (rfx_launch.h
// rfx_export_plan_for): four 16-byte loads, one run of whole dwords out (12 .. 64 bytes at t * group_bytes), never a byte or short store.  The
// pixels mod 4 left over are written by the lane after the last group with element-wide stores.  Format, channel count and operator are template
// arguments: nothing is decided per pixel.  This file is built uncontracted, so the fp32 chain keeps the operation order of imageio.tonemap.
RFX_DEV uint32_t k7_byte(float s) { return (uint32_t)(s * 255.0f + 0.5f); }  // s in [0, 1]: at most 255
// NaN -> 0, +inf -> 65504, -inf -> 0, clip to [0, 65504], times exposure
RFX_DEV float k7_linear_in(float x, float exposure) {
    x = x == x ? x : 0.0f;
    return fminf(fmaxf(x, 0.0f), 65504.0f) * exposure;
}
// NaN -> 0, inf -> 1, clip to [0, 1]; the sRGB transfer function; the byte
RFX_DEV uint32_t k7_srgb_byte(float c) {
    c = c == c ? c : 0.0f;
    c = fminf(fmaxf(c, 0.0f), 1.0f);
    const float s = c <= 0.0031308f ? c * 12.92f : 1.055f * rfx_pow(c, 1.0f / 2.4f) - 0.055f;
    return k7_byte(s);
}
RFX_DEV float k7_aces_fit(float c) { return (c * (c + 0.0245786f) - 0.000090537f) / (c * (0.983729f * c + 0.4329510f) + 0.238081f); }
template <int TM>
RFX_DEV void k7_display_rgb(float r, float g, float b, float exposure, uint32_t &R, uint32_t &G, uint32_t &B) {
    r = k7_linear_in(r, exposure); g = k7_linear_in(g, exposure); b = k7_linear_in(b, exposure);
    if (TM == 1) {  // three's ACESFilmicToneMapping: exposure / 0.6, RRT + ODT fit (Stephen Hill)
        r = r / 0.6f; g = g / 0.6f; b = b / 0.6f;
        const float x = k7_aces_fit(0.59719f * r + 0.35458f * g + 0.04823f * b);
        const float y = k7_aces_fit(0.07600f * r + 0.90834f * g + 0.01566f * b);
        const float z = k7_aces_fit(0.02840f * r + 0.13383f * g + 0.83777f * b);
        r = 1.60475f * x + -0.53108f * y + -0.07367f * z;
        g = -0.10208f * x + 1.10813f * y + -0.00605f * z;
        b = -0.00327f * x + -0.07276f * y + 1.07602f * z;
    }
    R = k7_srgb_byte(r); G = k7_srgb_byte(g); B = k7_srgb_byte(b);
}
RFX_DEV uint32_t k7_alpha_byte(float a) {
    a = a == a ? a : 0.0f;
    return k7_byte(fminf(fmaxf(a, 0.0f), 1.0f));
}
// the CH elements of one pixel, each in the low bits of a word: the float's bits, the half's bits, the byte
template <int FMT, int CH, int TM>
RFX_DEV void k7_encode(uint4 p, float exposure, uint32_t *e) {
    if (FMT == RFX_EXPORT_F32) {
        e[0] = p.x; e[1] = p.y; e[2] = p.z;
        if (CH == 4) e[3] = p.w;
    } else if (FMT == RFX_EXPORT_F16) {
        e[0] = rfx_f2h_rne(__uint_as_float(p.x)); e[1] = rfx_f2h_rne(__uint_as_float(p.y)); e[2] = rfx_f2h_rne(__uint_as_float(p.z));
        if (CH == 4) e[3] = rfx_f2h_rne(__uint_as_float(p.w));
    } else {
        k7_display_rgb<TM>(__uint_as_float(p.x), __uint_as_float(p.y), __uint_as_float(p.z), exposure, e[0], e[1], e[2]);
        if (CH == 4) e[3] = k7_alpha_byte(__uint_as_float(p.w));
    }
}
template <int FMT, int CH, int TM>
__global__ __launch_bounds__(RFX_K7_BLOCK) void k7_export(K7Args A) {
    constexpr int PER = FMT == RFX_EXPORT_F32 ? 1 : FMT == RFX_EXPORT_F16 ? 2 : 4;  // elements per dword
    constexpr int BITS = 32 / PER;
    constexpr int NW = 4 * CH / PER;  // dwords per group: 12 16 | 6 8 | 3 4
    const int t = blockIdx.x * RFX_K7_BLOCK + threadIdx.x;
    if (t < A.groups) {
        const uint4 *s = A.src + (size_t)t * 4;
        const uint4 p0 = s[0], p1 = s[1], p2 = s[2], p3 = s[3];
        uint32_t e[4 * CH];
        k7_encode<FMT, CH, TM>(p0, A.exposure, e);
        k7_encode<FMT, CH, TM>(p1, A.exposure, e + CH);
        k7_encode<FMT, CH, TM>(p2, A.exposure, e + 2 * CH);
        k7_encode<FMT, CH, TM>(p3, A.exposure, e + 3 * CH);
        uint32_t w[NW];
#pragma unroll
        for (int i = 0; i < NW; i++) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < PER; k++) v |= e[i * PER + k] << (k * BITS);
            w[i] = v;
        }
        uint32_t *d = (uint32_t *)A.dst + (size_t)t * NW;
#pragma unroll
        for (int i = 0; i < NW; i++) d[i] = w[i];
    } else if (t == A.groups) {
        for (int k = 0; k < A.tail_pixels; k++) {
            const size_t px = (size_t)A.tail_start + k;
            uint32_t e[CH];
            k7_encode<FMT, CH, TM>(A.src[px], A.exposure, e);
#pragma unroll
            for (int c = 0; c < CH; c++) {
                if (FMT == RFX_EXPORT_F32) ((uint32_t *)A.dst)[px * CH + c] = e[c];
                else if (FMT == RFX_EXPORT_F16) ((unsigned short *)A.dst)[px * CH + c] = (unsigned short)e[c];
                else ((unsigned char *)A.dst)[px * CH + c] = (unsigned char)e[c];
            }
        }
    }
}

}  // namespace

#include "k8_png.h"  // K8: the PNG fragment of K7's U8 stream
#include "k8_exr.h"  // ... and the EXR fragment of its F16 stream: the same coder behind another pre-transform
#include "k8_match.h"  // ... and both with run-length matches, as second scanline kernels

template <int FMT, int CH, int TM>
static void k7_launch(const K7Args &A, int blocks, hipStream_t stream) {
    hipLaunchKernelGGL((k7_export<FMT, CH, TM>), dim3(blocks), dim3(RFX_K7_BLOCK), 0, stream, A);
}
// the eight specialisations: F32 and F16 x {3, 4} channels, U8_SRGB x {3, 4} x {linear, ACES}
hipError_t rfx_launch_k7(const K7Args &A, int blocks, int format, int channels, int tonemap, hipStream_t stream) {
    if ((channels != 3 && channels != 4) || tonemap < 0 || tonemap > 1 || (tonemap && format != RFX_EXPORT_U8_SRGB)) return hipErrorInvalidValue;
    const bool rgba = channels == 4;
    switch (format) {
    case RFX_EXPORT_F32: rgba ? k7_launch<RFX_EXPORT_F32, 4, 0>(A, blocks, stream) : k7_launch<RFX_EXPORT_F32, 3, 0>(A, blocks, stream); break;
    case RFX_EXPORT_F16: rgba ? k7_launch<RFX_EXPORT_F16, 4, 0>(A, blocks, stream) : k7_launch<RFX_EXPORT_F16, 3, 0>(A, blocks, stream); break;
    case RFX_EXPORT_U8_SRGB:
        if (tonemap) rgba ? k7_launch<RFX_EXPORT_U8_SRGB, 4, 1>(A, blocks, stream) : k7_launch<RFX_EXPORT_U8_SRGB, 3, 1>(A, blocks, stream);
        else rgba ? k7_launch<RFX_EXPORT_U8_SRGB, 4, 0>(A, blocks, stream) : k7_launch<RFX_EXPORT_U8_SRGB, 3, 0>(A, blocks, stream);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// `chain` holds level 0 (6 * size * size texels) and room for the further levels (size >> l, at least 1), built here
hipError_t rfx_launch_cube_to_equirect(float4 *chain, int size, int levels, float4 *out, int W, int H, const UvPlanes &uv, hipStream_t stream) {
    K0Cube A;
    A.chain = chain; A.S = size; A.levels = levels; A.out = out; A.W = W; A.H = H; A.uv = uv;
    unsigned int off = 0;
    for (int l = 0; l < 14; l++) {
        A.off[l] = off;
        const int s = (size >> l) > 0 ? size >> l : 1;
        off += 6u * (unsigned int)s * (unsigned int)s;
    }
    for (int l = 1; l < levels; l++) {
        const int s0 = size >> (l - 1), s1 = size >> l;
        hipLaunchKernelGGL(k0_cube_mip, dim3((6 * s1 * s1 + 255) / 256), dim3(256), 0, stream, (const float4 *)chain + A.off[l - 1], chain + A.off[l], s0, s1);
    }
    dim3 block(64, 4), grid((W + 63) / 64, (H + 3) / 4);
    hipLaunchKernelGGL(k0_cube_to_equirect, grid, block, 0, stream, A);
    return hipGetLastError();
}

hipError_t rfx_launch_pack_gbuffer(int W, int rows, const float *diffuse, const float *normal, const float *roughness, const float *metalness,
                                   const float *emissive, const float *depth, void *out, hipStream_t stream) {
    K0GBuffer A = {W, rows, diffuse, normal, roughness, metalness, emissive, depth, (uint4 *)out};
    dim3 block(64, 4), grid((W + 63) / 64, (rows + 3) / 4);
    hipLaunchKernelGGL(k0_pack_gbuffer, grid, block, 0, stream, A);
    return hipGetLastError();
}
// the three specialisations: no half plane, the typed set (every plane the segment reads but velocity and depth), any other mix
hipError_t rfx_launch_k0_aov(const K0AovArgs &A, int blocks, hipStream_t stream) {
    if (!A.plane[RFX_AOV_DEPTH] || !A.depth || blocks <= 0) return hipErrorInvalidValue;
    unsigned int given = 0;
    for (int i = 0; i < RFX_AOV_PLANES; i++) given |= A.plane[i] ? 1u << i : 0u;
    const unsigned int halves = A.half_mask & given, typed = given & ~((1u << RFX_AOV_VELOCITY) | (1u << RFX_AOV_DEPTH));
    if (halves == 0u) hipLaunchKernelGGL(k0_aov_pack<0>, dim3(blocks), dim3(RFX_K0_AOV_BLOCK), 0, stream, A);
    else if (halves == typed) hipLaunchKernelGGL(k0_aov_pack<1>, dim3(blocks), dim3(RFX_K0_AOV_BLOCK), 0, stream, A);
    else hipLaunchKernelGGL(k0_aov_pack<2>, dim3(blocks), dim3(RFX_K0_AOV_BLOCK), 0, stream, A);
    return hipGetLastError();
}
hipError_t rfx_launch_pack_velocity(int W, int rows, const float *velocity, const float *normal, const float *depth, void *out, hipStream_t stream) {
    K0Velocity A = {W, rows, velocity, normal, depth, (uint4 *)out};
    dim3 block(64, 4), grid((W + 63) / 64, (rows + 3) / 4);
    hipLaunchKernelGGL(k0_pack_velocity, grid, block, 0, stream, A);
    return hipGetLastError();
}
