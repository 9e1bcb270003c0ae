// rfx_kernels.h — launch-argument blocks and launcher prototypes of the kernels, K0 .. K8, each block with its launchers under it.
#pragma once
#include <hip/hip_runtime.h>
#include "rfx_device.h"

// Rows [y0, y1) of the frame are produced by a launch (the context's tile, plus whatever extra
// rows the host asks for, e.g. K1's +-2 rows that K2's neighbourhood clamp reads).

// K0 importer (k0_import.hip): device staging planes of `rows` rows -> packed texels
hipError_t rfx_launch_pack_gbuffer(int W, int rows, const float *diffuse, const float *normal, const float *roughness, const float *metalness,
                                   const float *emissive, const float *depth, void *out, hipStream_t);
hipError_t rfx_launch_pack_velocity(int W, int rows, const float *velocity, const float *normal, const float *depth, void *out, hipStream_t);
// K0 AOV pack (k0_import.hip): one segment of rfx_stage_aov (rfx_launch.h rfx_aov_plan_for) — the staged planes of its flat pixel run -> the
// segment's first texel of every slot it writes.  Planes in rfx_aov_frame's order (RFX_AOV_*); a null output is not written.
struct K0AovArgs {
    const void *plane[8];      // 256-byte-aligned staging pieces; null: not read
    unsigned int half_mask;    // bit i: plane i holds IEEE halves
    int diffuse_ch, direct_ch; // 3 or 4
    uint4 *gbuffer, *velocity, *direct;
    float *depth;
    int groups, tail_start, tail_pixels;  // lanes [0, groups) own four pixels each; lane `groups` the tail
};
// ... with conventions in use (include/rfx.h "AOV conventions"): the setting as the kernel reads it, wave-uniform in the argument block behind
// K0AovArgs.  (W, H, row0): the frame and the segment's first frame row, for the texels' uv.
struct K0AovConv {
    int depth_kind, velocity_kind, normal_space, perspective;
    int W, H, row0;
    int has_background;
    float background[3];
    float scale[2];
    float near_, far_;
    float VM[16], PVM[16], P[16], Pi[16], C[16];  // velocityMatrix, prevVelocityMatrix, projectionMatrix, its inverse, cameraMatrixWorld
};
struct K0AovConvArgs : K0AovArgs { K0AovConv v; };
// conv null: the default kernels, on K0AovArgs alone
hipError_t rfx_launch_k0_aov(const K0AovArgs &, int blocks, hipStream_t, const K0AovConv *conv = nullptr);
// K0 AOV pack over device planes (k0_import.hip k0_aov_pack_strided): one segment of rfx_stage_aov_device that k0_aov_pack cannot serve
// (rfx_launch.h rfx_aov_device_plan_for) — the producer's planes, addressed by element strides, -> the segment's first texel of every slot it
// writes (row pitch W).  `base`: the element of column 0, the segment's first row, channel 0.
struct K0AovStridedPlane { const void *base; long long sx, sy, sc; };
struct K0AovStridedArgs {
    K0AovStridedPlane plane[8];  // base null: not read
    unsigned int half_mask;      // bit i: plane i holds IEEE halves
    unsigned int layouts;        // bits [2 i, 2 i + 2): plane i's RFX_AOV_LAYOUT_*
    int diffuse_ch, direct_ch;   // 3 or 4
    uint4 *gbuffer, *velocity, *direct;
    float *depth;
    int W, rows;                 // the segment: `rows` rows of W texels
    int groups_x, tail_x, tail_pixels, lanes_x;  // per row: lanes [0, groups_x) own four pixels each, lane groups_x the tail; lanes_x of them
};
struct K0AovStridedConvArgs : K0AovStridedArgs { K0AovConv v; };
// grid_x x grid_y workgroups of RFX_K0_DEV_BX x RFX_K0_DEV_BY lanes; conv null: the default kernel, on K0AovStridedArgs alone
hipError_t rfx_launch_k0_aov_strided(const K0AovStridedArgs &, int grid_x, int grid_y, hipStream_t, const K0AovConv *conv = nullptr);
// CubeToEquirectEnvPass (k0_cube.hip): six S x S RGBA32F faces -> a W x H RGBA32F equirectangular image
hipError_t rfx_launch_cube_to_equirect(float4 *chain, int size, int levels, float4 *out, int W, int H, const UvPlanes &uv, hipStream_t);

struct K1Args {
    FrameDims dims;
    int y0, y1;
    TexView depth, gbuffer, direct, history;  // history = K4 output of the previous frame (RGBA32F, nearest)
    const void *blue;
    int shift_x, shift_y;
    TexViewW out;  // RGBA32F holding 8 halfs
    rfx_ssgi_params p;
    float nearMulFar, farMinusNear, nearMinusFar;
    float *viewz;    // full-frame view-space Z (context scratch, filled by k1_prepare)
    float2 *coarse;  // exact (min, max) view Z per 16x16-texel base cell (k1_prepare)
    int coarse_w, coarse_h;
    unsigned int *cells;  // the march's table: two halfs per 2^cell_shift-texel cell, padded to whole uint4s (k1_pack_cells)
    int cells_w, cells_h, cell_shift, cells_vec4;
    int cells_pitch, cells_pitch_log2;  // cells per table row: cells_w, or (cells_pow2) the next power of two, at least 2^cell_shift — k1_tap_at
    int cells_pow2;                     // the table's rows are padded to a power of two (rfx_k1_table: when that fits at the same cell size)
    // scene.environment: all mip levels as float4 texels, level l (max(w>>l,1) x max(h>>l,1)) at env + env_off[l]
    const float4 *env;
    int env_w, env_h, env_levels;
    unsigned int env_off[16];
    float maxEnvMapMipLevel;
    const float *env_marginal, *env_conditional;  // EquirectHdrInfo.marginalWeights (env_h) / conditionalWeights (env_w x env_h), importanceSampling
    float totalSumWhole, totalSumDecimal;
    int out_w, out_h;  // the pass's render target = `resolution` (frame size unless resolutionScale != 1: [y0, y1) are then rows of THAT target, texel
                       // (x, y) is stored at y * out_w + x of `out.ptr` and `hits`, and a row tile — which holds the target rows [j0, j1) of rfx_launch.h
                       // rfx_scaled_rows from the start of its slot — passes both pointers rebased by -j0 rows; out.row0 / out.rows are not read)
    UvPlanes out_uv;   // that target's vUv
    float4 *hits;      // trace -> shade hand-over (2 texels per output pixel, indexed like `out`); null for the fused launch
    unsigned int *tile_counter;  // the persistent march kernel's work counter (context scratch; zero when the launch starts)
    int n_cu;                    // compute units of the device (sizes the persistent grid)
    unsigned char *fg_tiles;     // k1_prepare also writes K3's foreground map: one byte per 64 x 8-texel tile, rows of fg_w = ceil(W / 64) bytes
    int fg_w;
    const float *env_sums;       // tables built on the device (K10): totalSumWhole, totalSumDecimal are read here (device memory); null: the two fields above
};
int rfx_k1_base_cell();  // edge of k1_prepare's base cells in texels
hipError_t rfx_launch_k1_prepare(const K1Args &, hipStream_t);
hipError_t rfx_launch_k1(const K1Args &, int stage /* 0 fused, 1 trace, 2 shade */, hipStream_t);
// mask[row] |= 1 << column block (32 blocks across the frame) for every history texel the shade stage of the traced rays of rows [y0, y1) will read (H words, zeroed)
hipError_t rfx_launch_k1_hit_mask(const FrameDims &, int y0, int y1, TexView depth, TexViewW out, const float4 *hits, bool allow_missed, unsigned int *mask, hipStream_t);
// ... after a trace at resolutionScale != 1: the fragments are the out_w x [j0, j1) target rows (vUv planes out_uv), their hand-over texels sit at
// (y - j0) * out_w + x, their depth at the NEAREST frame texel of their vUv; rows and column blocks are named at full resolution, as k1_shade reads them
hipError_t rfx_launch_k1_hit_mask_scaled(const FrameDims &, const UvPlanes &out_uv, int out_w, int j0, int j1, TexView depth, const float4 *hits, bool allow_missed,
                                         unsigned int *mask, hipStream_t);
// one level of the environment's mip chain from the one above (glGenerateMipmap on the oracle's GL: 2x2 bilinear centre)
hipError_t rfx_launch_env_mip(const float4 *src, float4 *dst, int sw, int sh, int dw, int dh, bool to_half, bool rtz, hipStream_t);
// K10 (k10_env_tables.hip): the importance tables of a W x H environment (powers of two) from its level 0 — marginal (H floats), conditional (W x H),
// and in `scratch` (rfx_env_tables_scratch_bytes) a K10Sums first: the double total, then the two floats K1 reads (rfx_env_tables_sums)
hipError_t rfx_launch_env_tables(const float4 *env, int W, int H, int flipY, float *marginal, float *conditional, void *scratch, hipStream_t);
static inline size_t rfx_env_tables_scratch_bytes(int H) { return 24 + (size_t)H * sizeof(double); }  // K10Sums, the marginal's last sum, the row sums
static inline const float *rfx_env_tables_sums(const void *scratch) { return (const float *)((const char *)scratch + 8); }

struct K2Args {
    FrameDims dims;
    int y0, y1;
    TexView ssgi, velocity, hist0, hist1;  // hist* = K3 target B of the previous frame (RGBA16F, linear), or the pass's framebuffer copy
    int hist_f32;                          // history texels are RGBA32F (FloatType framebuffer copy) instead of RGBA16F
    int in_w, in_h;                        // size of the input texture (smaller than the frame when K1 ran with resolutionScale < 1)
    TexViewW out0, out1;
    rfx_temporal_params p;
    float invW, invH;        // invTexSize (TemporalReprojectPass.js:135)
    float rcpInvW, rcpInvH;  // RN(1 / invTexSize): the constant of the exact quotient P / invTexSize (RFX_DIV_CONST's form, k2_bicubic)
    float prevPV[16];  // prevProjectionMatrix * prevViewMatrix, multiplied in fp32 like the shader does per fragment
    // a smaller input texture on a row tile (appended, for in_w / in_h above: nothing in front of it moves): `ssgi` holds the target rows
    // [in_j0, in_j0 + in_rows) from the start of the slot, pitch in_w (rfx_launch.h rfx_scaled_rows); 0, in_h on a whole-frame context
    int in_j0, in_rows;
};
hipError_t rfx_launch_k2(const K2Args &, hipStream_t);
// rows [y0, y1) of an RGBA32F plane -> the same rows of an RGBA16F (to_half) or RGBA32F plane
hipError_t rfx_launch_copy_fb(const FrameDims &, int y0, int y1, TexView src, TexViewW dst, bool to_half, hipStream_t);

struct K3Args {
    FrameDims dims;
    int y0, y1;
    TexView depth, gbuffer, in0, in1;
    const void *blue;
    int shift_x, shift_y;
    TexViewW out0, out1;
    rfx_denoise_params p;
    struct { int Rx, Ry, LW, LH, skip; } tile;  // filled by the launcher (skip: texels shaved off each end of the staged rectangle, k3_tiled_body)
    float tap_ox[8], tap_oy[8];           // POISSON[k] / resolution, filled by the launcher
    // K1's foreground map of the depth plane (ceil(W / 64) bytes per row of frame-aligned 64 x 8-texel tiles; 4-byte aligned, padded to whole
    // words) or null: a workgroup whose tile's byte is 0 returns at once — every pixel of it would discard.  The caller passes it only while it
    // describes `depth` and y0 is a multiple of 8; the launcher drops it unless every view is the whole frame.
    const unsigned char *fg_tiles;
};
hipError_t rfx_launch_k3(const K3Args &, hipStream_t);

struct K4Args {
    FrameDims dims;
    int y0, y1;
    TexView depth, gbuffer, gi0, gi1;  // gi*: K3 target B (RGBA16F, linear) or, giSource 1, K2's targets (RGBA32F, nearest)
    TexView scene;  // the composer's input buffer (sceneTexture): read only by inputType "specular"
    TexViewW out;
    float *rgb_out;  // RFX_TEX_COMPOSE_RGB (whole frame, 3 floats per texel) or null
    rfx_compose_params p;
};
hipError_t rfx_launch_k4(const K4Args &, hipStream_t);

struct K5Args {
    FrameDims dims;
    int y0, y1;
    TexView depth, gi, scene;  // gi = K4 output (inputTexture), scene = the composer's input buffer (sceneTexture)
    TexViewW out;
    rfx_final_params p;
};
hipError_t rfx_launch_k5(const K5Args &, hipStream_t);

// K6 (k6_motion_blur.hip): MotionBlurEffect.  The whole-frame launch addresses every plane by frame row; the row-tiled launch (tiled != 0) reads
// velocity and an explicit centre, and writes the output, through their held bands (the *_row0 / *_rows pairs at the end of the block) while
// `src` is RFX_TEX_BLUR_SOURCE, held whole.
struct K6Args {
    FrameDims dims;
    int y0, y1;
    const float4 *velocity;  // RFX_TEX_VELOCITY: .xy = uv-space velocity (NEAREST at vUv = the pixel's own texel)
    const float4 *src;       // inputTexture (LINEAR taps)
    const float4 *center;    // where inputColor comes from
    float4 *out;             // RFX_TEX_MOTION_BLUR
    const uchar4 *blue;      // the 128 x 128 blue-noise table
    int shift_x, shift_y;    // blueNoise's per-frame toroidal shift (0 for frame 0: the texture path)
    int center_nearest, center_alpha_one, target_half, half_rtz;
    int samples;
    float samplesF, rcpSamplesF;  // samplesFloat and RN(1 / samplesFloat): i / samplesFloat as rfx_div_const_impl
    float div2;                   // samplesFloat + 2
    float intensity, jitter, frameSpeed;  // frameSpeed = RN(0.01 / deltaTime), a uniform expression: the same for every fragment
    float resX, resY;
    // row-tiled launches and the reach reduction (appended: the whole-frame kernel reads nothing past resY)
    int tiled;                 // select the band-view kernel
    int vel_row0, vel_rows, center_row0, center_rows, out_row0, out_rows;  // held bands of velocity / center / out
    int center_is_source;      // center == -1: inputColor is the LINEAR fetch of `src` at vUv (the reach mask then names its footprint)
    unsigned int *reach_mask;  // k6_motion_blur_reach: H words, zeroed (one per frame row, a bit per column block)
};
hipError_t rfx_launch_k6(const K6Args &, hipStream_t);
// mask[row] |= 1 << column block for every texel of `src` that rfx_launch_k6 with the same block loads for rows [y0, y1): the draw's streak
// set-up and tap addressing without the loads (velocity is always read through its band view)
hipError_t rfx_launch_k6_reach(const K6Args &, hipStream_t);

// K7 export (k7_export.hip): `pixels` RGBA32F texels from `src` -> the packed stream at `dst`, laid out by rfx_launch.h rfx_export_plan_for
struct K7Args {
    const uint4 *src;  // first exported texel
    void *dst;         // staging buffer (at least 16-byte aligned)
    int groups;        // lanes [0, groups) own four pixels each
    int tail_start, tail_pixels;  // lane `groups` writes these with element-wide stores
    float exposure;
};
// format / channels / tonemap select the specialisation (hipErrorInvalidValue for a combination the export does not have); `blocks` from the plan
hipError_t rfx_launch_k7(const K7Args &, int blocks, int format, int channels, int tonemap, hipStream_t);
// K7 into a device image (k7_export.hip k7_export_strided): `rows` rows of W RGBA32F texels from `src` (row pitch W) -> the caller's image,
// addressed by element strides, in one of the store forms of rfx_launch.h rfx_export_device_plan_for (never TIGHT: that is rfx_launch_k7)
struct K7StridedArgs {
    const uint4 *src;       // first exported texel
    void *dst;              // the element of column 0, the first exported row, channel 0
    long long sx, sy, sc;   // in elements of the format
    int W, rows;
    int groups_x, tail_x, tail_pixels, lanes_x;  // per row: lanes [0, groups_x) own four pixels each, lane groups_x the tail; lanes_x of them
    int form;               // RFX_EXPORT_FORM_INTERLEAVED / _PLANAR / _ELEMENT
    float exposure;
};
// grid_x x grid_y workgroups of RFX_K7_DEV_BX x RFX_K7_DEV_BY lanes; the specialisation as for rfx_launch_k7
hipError_t rfx_launch_k7_strided(const K7StridedArgs &, int grid_x, int grid_y, int format, int channels, int tonemap, hipStream_t);

// K8 PNG encode (k8_png.h over k8_coder.h, built into k7_export.hip): K7's staged U8 stream -> the result buffer of include/rfx.h "PNG fragments", laid out by
// rfx_launch.h rfx_png_plan_for.  Three launches on `stream`: one wave per scanline into the scratch slots, the scan, the gather.
struct K8Args {
    const unsigned char *src;     // K7's stream: `rows` rows of `rowbytes` bytes, row 0 = bottom
    unsigned char *result;        // 32-byte header, then the fragment
    unsigned char *slots;         // rows * slot_stride bytes of scratch: one whole chunk per scanline
    unsigned *meta;               // rows * 4: chunk bytes, the two Adler partial sums, 1 for a chunk in the match form
    unsigned long long *offsets;  // rows: where each chunk starts in the fragment
    unsigned long long fragment_cap;  // bound - 32
    int rows, rowbytes, bpp, filter;
    unsigned slot_stride;
};
// matches: the scanline kernel is k8_png_rows<true> (the match form where it is smaller) instead of k8_png_rows<false> (literals only)
hipError_t rfx_launch_k8(const K8Args &, hipStream_t, bool matches = false);

// K8 EXR encode (k8_exr.h, built into k7_export.hip): K7's staged F16 stream -> the result buffer of include/rfx.h "EXR fragments", laid out by
// rfx_launch.h rfx_exr_plan_for.  Four launches on `stream`: the byte planes, one wave per scanline into the scratch slots, the scan, the gather.
struct K8ExrArgs {
    const unsigned short *src;    // K7's stream: `rows` rows of `width` pixels of `channels` halfs, row 0 = bottom
    unsigned char *result;        // 32-byte header, then the fragment
    unsigned char *slots;         // rows * slot_stride bytes of scratch: one whole chunk per scanline
    unsigned char *planes;        // rows * plane_stride bytes of scratch: each scanline's low bytes, then its high bytes
    unsigned *meta;               // rows * 4: chunk bytes, 1 for a raw chunk, 1 for a chunk in the match form, 0
    unsigned long long *offsets;  // rows: where each chunk starts in the fragment
    unsigned long long fragment_cap;  // bound - 32
    int rows, width, channels;
    int first_y;                  // the EXR y of the tile's top scanline
    unsigned slot_stride, plane_stride;
};
// matches: the scanline kernel is k8_exr_rows<true> instead of k8_exr_rows<false>
hipError_t rfx_launch_k8_exr(const K8ExrArgs &, hipStream_t, bool matches = false);

// K9 EXR import (k9_exr_import.hip): the packed blocks of an OpenEXR file — scanline chunks or tiles, a rectangle of the frame each — -> the typed
// AOV staging planes k0_aov_pack reads (include/rfx.h "streamed EXR frames", "EXR blocks").  Four launches on `stream`: k9_inflate (one wave per
// block: zlib stream or raw block -> the block's scratch slot), k9_rle (one wave per block: the RLE parts' blocks), k9_exr_planes (one block of
// threads per file block: predictor and byte split, or PXR24's differences, undone, the mapped channels scattered, rows flipped), k9_exr_finish
// (the rectangle of a bad block reads as not covered; the status words); with PIZ streams in the band two more in front of the planes: k9_piz_huf
// (one wave per block: reverse lookup table, Huffman tables and decode, csrc/k9_piz.h) and k9_piz_planes (the wavelet in cells, the lookup, the
// scatter).  The tables are device copies of the call's descriptor, built by
// rfx_exr_import.hip's exr_blocks_plan for every entry point.
struct K9Chunk {
    unsigned long long src, dst;  // 256-byte-aligned offsets of the packed bytes / of the scratch slot (raw bytes, which is the LZ77 window too)
    unsigned int packed, raw;     // packed == raw: the raw block itself
    unsigned int expect;          // what the decoder must produce: raw, but for PXR24 3 bytes per FLOAT sample
    int part, x, y, cols, rows;   // the block's top-left texel (EXR scanline 0 = top) and size; a scanline chunk: x = 0, cols = W
    int index;                    // in the descriptor's chunk / block table (what the status reports)
    int piz;                      // a PIZ stream: its slot in K9Args.piz_tables
};
// plane < 0: dropped; off / pxr_off: bytes per texel of the part's channels before this one, raw and as PXR24 stores them — the channel's samples
// of a block's row start cols x that many bytes behind the row's start
struct K9Chan { int half, plane, comp; unsigned int off, pxr_off; };
struct K9Part { int chan0, nchan; unsigned int texel_bytes, pxr_bytes; int compression; };  // OpenEXR's number (rfx.h RFX_EXR_*)
struct K9Args {
    const K9Chunk *chunks;
    const K9Part *parts;
    const K9Chan *chans;
    int nchunks;
    int rle_chunks;            // how many of them are RLE streams (0: k9_rle is not launched)
    int piz_chunks;            // ... PIZ streams (0: k9_piz_huf and k9_piz_planes are not launched)
    unsigned char *piz_tables; // piz_chunks slots of k9_piz.h's K9_PIZ_TABLE_BYTES: reverse lookup table, sorted symbols, mx
    const unsigned char *packed;
    unsigned char *scratch;
    int *err;                  // per chunk: k9_inflate.h's / k9_rle.h's K9_E_* (0: decoded)
    int *status;               // [0] bad chunks, [1] 0x7fffffff - ((index << 8) | code) of the first bad chunk (0: none), zeroed before the launches
    int W, H;
    int nseg;                  // rfx_aov_plan's segments: frame rows [seg_row0, seg_row0 + seg_rows) and where each plane's rows of them are staged
    int seg_row0[3], seg_rows[3];
    void *seg_plane[3][8];     // null: the segment does not read the plane
    int plane_ch[8], plane_half[8];
    int depth_bad_nan;         // the depth plane of a bad block's rectangle: 0 -> 1.0; else NaN in every channel (AOV conventions: view z, position)
};
hipError_t rfx_launch_k9(const K9Args &, hipStream_t);
