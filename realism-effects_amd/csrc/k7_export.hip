// K7 — export: the importer run in reverse (include/rfx.h rfx_export_params), and K8, the encoders of its stream (k8_coder.h, k8_png.h, k8_exr.h).
// A pure stream: 16 B in per pixel, 3 to 16 B out.  Lane t owns the four consecutive pixels [4 t, 4 t + 4) of the flat run (rfx_launch.h
// rfx_export_plan_for): four 16-byte loads, one run of whole dwords out (12 .. 64 bytes at t * group_bytes), never a byte or short store.  The
// pixels mod 4 left over are written by the lane after the last group with element-wide stores.  Format, channel count and operator are template
// arguments: nothing is decided per pixel.  This file is built uncontracted, so the fp32 chain keeps the operation order of imageio.tonemap.
// k7_export_strided (below k7_export) is the same encode into an image in device memory that its owner addresses by strides.
#include "rfx_device.h"
#include "rfx_kernels.h"
#include "rfx_launch.h"

namespace {

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

// ---------------------------------------------------------------- K7 into a device image, for rfx_export_device (include/rfx.h "device images")
// k7_export's work with a destination that lies where its owner keeps it: the element of column x, row y, channel ch goes sx x + sy y + sc ch
// elements from dst, strides of any sign.  Rows have pitch, so the decomposition is two-dimensional, k0_aov_pack_strided's: a workgroup is
// RFX_K7_DEV_BX lanes along a row by RFX_K7_DEV_BY rows, lane l < groups_x of a row owns its pixels [4 l, 4 l + 4) — four 16-byte loads, as in
// k7_export —, lane groups_x the W mod 4 pixels from tail_x on, element by element.  The store form is uniform over the launch (rfx_launch.h
// rfx_export_device_plan_for decides it, with the alignment it needs) and branched on per wave; nothing but the encode is decided per pixel:
//   INTERLEAVED  the lane's 4 CH elements are one run of NW whole dwords (k7_export's words, at the row's base + 16 CH element bytes x lane);
//   PLANAR       per channel the lane's four elements are one aligned store: 16 bytes (F32), 8 (F16), 4 (U8) — a wave writes 1 KiB / 512 B /
//                256 B of consecutive bytes per instruction;
//   ELEMENT      one element per store.
// The elements come from the same k7_encode on the same texels: they are k7_export's bit for bit.
template <int FMT>
RFX_DEV void k7_store_elem(void *dst, long long i, uint32_t e) {
    if (FMT == RFX_EXPORT_F32) ((uint32_t *)dst)[i] = e;
    else if (FMT == RFX_EXPORT_F16) ((unsigned short *)dst)[i] = (unsigned short)e;
    else ((unsigned char *)dst)[i] = (unsigned char)e;
}
template <int FMT, int CH, int TM>
__global__ __launch_bounds__(RFX_K7_DEV_BX * RFX_K7_DEV_BY) void k7_export_strided(K7StridedArgs A) {
    constexpr int PER = FMT == RFX_EXPORT_F32 ? 1 : FMT == RFX_EXPORT_F16 ? 2 : 4;  // elements per dword
    constexpr int BITS = 32 / PER;
    constexpr int NW = 4 * CH / PER;  // dwords per group: 12 16 | 6 8 | 3 4
    constexpr int ELEM = 4 / PER;     // bytes per element
    const int lane = blockIdx.x * RFX_K7_DEV_BX + threadIdx.x, y = blockIdx.y * RFX_K7_DEV_BY + threadIdx.y;
    if (lane >= A.lanes_x || y >= A.rows) return;
    const uint4 *s = A.src + (size_t)y * (size_t)A.W;
    const long long row = (long long)y * A.sy;
    if (lane < A.groups_x) {
        const int x0 = 4 * lane;
        const uint4 p0 = s[x0], p1 = s[x0 + 1], p2 = s[x0 + 2], p3 = s[x0 + 3];
        uint32_t e[4 * CH];
        k7_encode<FMT, CH, TM>(p0, A.exposure, e);
        k7_encode<FMT, CH, TM>(p1, A.exposure, e + CH);
        k7_encode<FMT, CH, TM>(p2, A.exposure, e + 2 * CH);
        k7_encode<FMT, CH, TM>(p3, A.exposure, e + 3 * CH);
        if (A.form == RFX_EXPORT_FORM_INTERLEAVED) {
            uint32_t w[NW];
#pragma unroll
            for (int i = 0; i < NW; i++) {
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < PER; k++) v |= e[i * PER + k] << (k * BITS);
                w[i] = v;
            }
            uint32_t *d = (uint32_t *)((char *)A.dst + (row + (long long)x0 * CH) * ELEM);
#pragma unroll
            for (int i = 0; i < NW; i++) d[i] = w[i];
        } else if (A.form == RFX_EXPORT_FORM_PLANAR) {
#pragma unroll
            for (int c = 0; c < CH; c++) {
                char *d = (char *)A.dst + (row + (long long)c * A.sc + x0) * ELEM;
                const uint32_t a = e[c], b = e[CH + c], g = e[2 * CH + c], h = e[3 * CH + c];
                if (FMT == RFX_EXPORT_F32) *(uint4 *)d = make_uint4(a, b, g, h);
                else if (FMT == RFX_EXPORT_F16) *(uint2 *)d = make_uint2(a | (b << 16), g | (h << 16));
                else *(uint32_t *)d = a | (b << 8) | (g << 16) | (h << 24);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int c = 0; c < CH; c++) k7_store_elem<FMT>(A.dst, row + (long long)(x0 + k) * A.sx + (long long)c * A.sc, e[k * CH + c]);
        }
    } else {
        for (int k = 0; k < A.tail_pixels; k++) {
            const int x = A.tail_x + k;
            uint32_t e[CH];
            k7_encode<FMT, CH, TM>(s[x], A.exposure, e);
#pragma unroll
            for (int c = 0; c < CH; c++) k7_store_elem<FMT>(A.dst, row + (long long)x * A.sx + (long long)c * A.sc, e[c]);
        }
    }
}

}  // namespace

#include "k8_png.h"  // K8: the PNG fragment of K7's U8 stream (the deflate coder: k8_coder.h)
#include "k8_exr.h"  // ... and the EXR fragment of its F16 stream: the same coder behind another pre-transform

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

template <int FMT, int CH, int TM>
static void k7_launch_strided(const K7StridedArgs &A, int grid_x, int grid_y, hipStream_t stream) {
    hipLaunchKernelGGL((k7_export_strided<FMT, CH, TM>), dim3(grid_x, grid_y), dim3(RFX_K7_DEV_BX, RFX_K7_DEV_BY), 0, stream, A);
}
// ... and the same eight over a device image
hipError_t rfx_launch_k7_strided(const K7StridedArgs &A, int grid_x, int grid_y, int format, int channels, int tonemap, hipStream_t stream) {
    if ((channels != 3 && channels != 4) || tonemap < 0 || tonemap > 1 || (tonemap && format != RFX_EXPORT_U8_SRGB)) return hipErrorInvalidValue;
    if (!A.src || !A.dst || grid_x <= 0 || grid_y <= 0 || A.W <= 0 || A.rows <= 0) return hipErrorInvalidValue;
    if (A.groups_x != A.W / 4 || A.tail_x != 4 * A.groups_x || A.tail_pixels != A.W - A.tail_x || A.lanes_x != A.groups_x + (A.tail_pixels ? 1 : 0))
        return hipErrorInvalidValue;
    if (A.form != RFX_EXPORT_FORM_INTERLEAVED && A.form != RFX_EXPORT_FORM_PLANAR && A.form != RFX_EXPORT_FORM_ELEMENT) return hipErrorInvalidValue;
    const bool rgba = channels == 4;
    switch (format) {
    case RFX_EXPORT_F32:
        rgba ? k7_launch_strided<RFX_EXPORT_F32, 4, 0>(A, grid_x, grid_y, stream) : k7_launch_strided<RFX_EXPORT_F32, 3, 0>(A, grid_x, grid_y, stream);
        break;
    case RFX_EXPORT_F16:
        rgba ? k7_launch_strided<RFX_EXPORT_F16, 4, 0>(A, grid_x, grid_y, stream) : k7_launch_strided<RFX_EXPORT_F16, 3, 0>(A, grid_x, grid_y, stream);
        break;
    case RFX_EXPORT_U8_SRGB:
        if (tonemap) rgba ? k7_launch_strided<RFX_EXPORT_U8_SRGB, 4, 1>(A, grid_x, grid_y, stream) : k7_launch_strided<RFX_EXPORT_U8_SRGB, 3, 1>(A, grid_x, grid_y, stream);
        else rgba ? k7_launch_strided<RFX_EXPORT_U8_SRGB, 4, 0>(A, grid_x, grid_y, stream) : k7_launch_strided<RFX_EXPORT_U8_SRGB, 3, 0>(A, grid_x, grid_y, stream);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
