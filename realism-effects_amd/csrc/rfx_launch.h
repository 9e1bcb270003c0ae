// rfx_launch.h — what a launch decides on the host before it launches: K1's table layout, a scaled tile's target rows, K3's tile geometry, the
// "whole frame" test, the step from a run-time option to a template argument, and what is remembered per kernel and device.  Host code
// (rfx_device.h comes in for UvPlanes and the two vUv expressions the kernels and the row plan share).  The plans are pure functions of their
// arguments (no HIP call, no context): rfx_draw.hip exports them as rfx_internal_k1_table / rfx_internal_k3_tile / rfx_internal_scaled_rows / rfx_internal_export_plan / rfx_internal_export_device_plan / rfx_internal_aov_plan / rfx_internal_aov_device_plan / rfx_internal_exr_piz_tables and
// the CPU tests call them as built (tests/test_k1_table_layout.py, tests/test_k3_tile_geometry.py, tests/test_resolution_scale_rows_cpu.py).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>
#include "rfx_device.h"

// ---------------------------------------------------------------- K1: the march's (min, max) table
// The table lives in every workgroup's LDS (four workgroups per CU): the cell edge is doubled until the table fits.  Two layouts (k1_tap_at):
// rows padded to a power of two, at least 2^cell_shift cells — a tap's LDS address is then two shifts and one v_bitop3_b32 — when that fits the
// 36 KiB at the SAME cell size as plain rows of cells_w cells would (4K: 32-texel cells, 128 x 68 cells = 34 KiB; every 16:9 frame); plain rows
// otherwise (an ultrawide frame, a frame taller than 9216 rows: the padded table of such a frame holds at least H cells)
constexpr int RFX_K1_TABLE_BYTES = 36864;
// cells_w x cells_h cells of 2^cell_shift texels; pitch: cells per table row — cells_w (pitch_log2 0) or, pow2, the next power of two, at
// least 2^cell_shift; vec4: the table in whole uint4s
struct rfx_k1_table_plan { int cell_shift, cells_w, cells_h, pitch, pitch_log2, pow2, vec4; };
inline rfx_k1_table_plan rfx_k1_table(int W, int H) {
    const auto k1_table = [&](int shift, bool pow2, int &cw, int &ch, int &pitch, int &pitch_log2) {
        cw = (W + (1 << shift) - 1) >> shift;
        ch = (H + (1 << shift) - 1) >> shift;
        pitch = cw;
        pitch_log2 = 0;
        if (pow2) {
            pitch_log2 = shift;  // (at least 2^cell_shift cells per row: the row term of k1_tap_at is then a LEFT shift by >= 2)
            while ((1 << pitch_log2) < cw) pitch_log2++;
            pitch = 1 << pitch_log2;
        }
        return (size_t)((pitch * ch + 3) / 4) * 16;  // bytes, whole uint4s
    };
    rfx_k1_table_plan t;
    t.pow2 = 0;
    for (t.cell_shift = 4;; t.cell_shift++) {
        if (k1_table(t.cell_shift, false, t.cells_w, t.cells_h, t.pitch, t.pitch_log2) <= (size_t)RFX_K1_TABLE_BYTES || t.cell_shift >= 12) break;
    }
    int cw, ch, pitch, pl2;
    if (k1_table(t.cell_shift, true, cw, ch, pitch, pl2) <= (size_t)RFX_K1_TABLE_BYTES) {
        t.pow2 = 1;
        t.pitch = pitch;
        t.pitch_log2 = pl2;
    }
    t.vec4 = (t.pitch * t.cells_h + 3) / 4;
    return t;
}

// ---------------------------------------------------------------- resolutionScale < 1: the rows of the smaller target a row tile draws
// K1 draws a Ws x Hs target, K2 reads it NEAREST at the full-resolution vUv: position (gx, gy) of the frame takes target row
// iy(gy) = rfx_nearest_idx(rfx_frag_v(frame uv, gy), Hs, Hs) (k2_body's staging loop).  K2 stages the rows gy of [y0 - apron, y1 - 1 + apron]
// that lie in the frame for its launch rows [y0, y1), so a tile has to draw exactly the target rows [j0, j1) those positions address: iy is
// monotonic in gy and, Hs <= H, moves by at most one row per frame row — the range has no gap.  The plan calls rfx_device.h rfx_frag_v /
// rfx_nearest_idx themselves (declared for the host too); it is a pure function of its arguments, exported as rfx_internal_scaled_rows and held
// against a brute force over gy under both vUv models (tests/test_resolution_scale_rows_cpu.py).  Everything that addresses a scaled tile's
// target — K1's launch, K2's argument block, the hit mask, the trace -> shade hand-over plane — takes (j0, j1) from here.
struct rfx_scaled_rows_plan { int j0, j1; };
// frame_uv: the planes of the W x H frame (rfx_uv_planes); Hs: rows of the target
inline rfx_scaled_rows_plan rfx_scaled_rows(const UvPlanes &frame_uv, int Hs, int y0, int y1, int apron) {
    int lo = y0 - apron, hi = y1 - 1 + apron;
    if (lo < 0) lo = 0;
    if (hi > frame_uv.H - 1) hi = frame_uv.H - 1;
    rfx_scaled_rows_plan t = {0, 0};
    if (hi < lo) return t;
    t.j0 = rfx_nearest_idx(rfx_frag_v(frame_uv, lo), (float)Hs, Hs);
    t.j1 = rfx_nearest_idx(rfx_frag_v(frame_uv, hi), (float)Hs, Hs) + 1;
    return t;
}

// ---------------------------------------------------------------- K3: the staged tile
constexpr int RFX_K3_TW = 64, RFX_K3_TH = 8;  // pixels per workgroup tile (64 x 16, 128 x 8, 64 x 7 measured slower: profiles/r05_k3)
constexpr int K3_LDS_MAX = 80 * 1024;         // dynamic LDS a tiled launch may ask for (80 KiB: at least two workgroups per CU; the CU has 160 KiB, handed out in
                                              // 1 280-byte granules: <= 53 760 B fit three times, <= 40 960 B four times — profiles/r05_microbench/lds_occupancy.txt)
// (Rx, Ry): the apron, LW x LH: the staged rectangle, texels; pitch: its LDS row pitch, a template argument of the tiled kernels (0: the
// rectangle is wider than any of them); skip: texels shaved off each end of the rectangle (k3_tiled_body); tiled 0: k3_generic
struct rfx_k3_tile_plan { int Rx, Ry, LW, LH, pitch, skip; size_t lds_bytes; int tiled; };
inline rfx_k3_tile_plan rfx_k3_tile(float fW, float fH, float radius, bool temporal, int textureCount) {
    constexpr int TW = RFX_K3_TW, TH = RFX_K3_TH;
    rfx_k3_tile_plan t;
    // apron of the tap footprint: anisotropic because the reference rotates in UV space
    const float aspect = fW / fH;
    const float rx = radius * fmaxf(1.0f, aspect), ry = radius * fmaxf(1.0f, 1.0f / aspect);
    // the apron the taps can address (k3_denoise.hip); SLACK covers the rounding of the tap coordinate itself (one ulp of vUv * size: 1e-3 pixel
    // on a 16K frame) — a tap offset that close to a half-integer (nearest) or an integer (linear) boundary stages one texel more
    const float SLACK = 4e-3f;
    const auto k3_apron = [&](float r) {  // (never below 1: the 2x2-quad partners and the centre's own LINEAR fetch)
        const int a = temporal ? (int)floorf(r + 0.5f + SLACK) : (int)floorf(r + SLACK) + 1;
        return a < 1 ? 1 : a;
    };
    t.Rx = k3_apron(rx);
    t.Ry = k3_apron(ry);
    t.LW = TW + 2 * t.Rx;
    t.LH = TH + 2 * t.Ry;
    t.skip = 0;
    // LDS row pitch: a compile-time constant of the tiled kernels (the footprint's second row is an immediate offset; padding it by 1 / 2 / 4 texels
    // moves neither the time nor the bank-conflict share: the conflicts are collisions of per-pixel-rotated taps, profiles/r04_k3)
    t.pitch = t.LW <= TW + 8 ? TW + 8 : t.LW <= TW + 10 ? TW + 10 : t.LW <= TW + 12 ? TW + 12 : t.LW <= TW + 16 ? TW + 16 : t.LW <= TW + 32 ? TW + 32 : 0;
    t.lds_bytes = (size_t)t.pitch * t.LH * (16 + 4 + 2 * (temporal ? 16 : 8));
    if (temporal && textureCount == 2 && t.pitch == t.LW && t.pitch != 0) {
        // The corners of the staged rectangle no tap reaches: a tap's offset from its pixel, in pixels, lies in the ellipse (dx / rx)^2 + (dy / ry)^2 <= 1
        // (the rotation acts in UV space, flatness <= 1, |POISSON[k]| <= 1), and the rectangle's first row is addressed only by the tile's first
        // row of pixels with dy in [-Ry - 0.5, -Ry + 0.5): there |dx| <= rx * sqrt(1 - ((Ry - 0.5) / ry)^2), i.e. a NEAREST tap reaches at most X texels
        // sideways and the first Rx - X texels of that row (and, mirrored, the last Rx - X of the last row) are never read.  Pass 0 only (the later
        // passes' LINEAR footprints reach further and their LDS size is nowhere near a granule boundary).
        const float q = ((float)t.Ry - 0.5f - SLACK) / ry;
        const int X = (int)floorf(0.5f + rx * sqrtf(fmaxf(0.0f, 1.0f - q * q)) + SLACK);
        int skip = t.Rx - X;
        if (skip > 4) skip = 4;  // (the pad in front of the depth array holds four floats)
        const int ntex = t.pitch * t.LH;
        while (skip > 0 && ((ntex - 2 * skip) & 3) != 0) skip--;  // the float4 arrays behind the depth array stay 16-byte aligned
        if (skip > 0) {
            t.skip = skip;
            t.lds_bytes = 16 + (size_t)(ntex - 2 * skip) * (4 + 16 + 32) + (size_t)skip * 32;  // pad | depth | geometry | interleaved inputs | pad
        }
    }
    // at least two workgroups per CU (160 KiB LDS) keep the staging of one tile under the arithmetic of another (4K: three of either pass kind)
    t.tiled = radius >= 0.0f && t.pitch != 0 && t.lds_bytes <= (size_t)K3_LDS_MAX;
    return t;
}

// ---------------------------------------------------------------- K7: the export's flat stream
// The exported rows are one flat run of `pixels` = tile_rows * W texels (source and destination are both contiguous: row ends need no case of
// their own).  Lane t < groups owns the pixels [4 t, 4 t + 4): four 16-byte loads and group_bytes = 4 * pixel_bytes = 12, 16, 24, 32, 48 or 64
// bytes stored at t * group_bytes — always whole dwords at a dword-aligned offset.  The pixels [tail_start, pixels), pixels mod 4 of them, are
// written by ONE lane (t == groups) with element-wide stores.  A pure function of its arguments, exported as rfx_internal_export_plan and held
// against a brute force over the output bytes (tests/test_export_cpu.py).
constexpr int RFX_K7_BLOCK = 256;
struct rfx_export_plan {
    int pixels, groups, blocks;    // groups of four pixels; workgroups of RFX_K7_BLOCK lanes (the tail's lane included)
    int tail_start, tail_pixels;   // pixels - pixels mod 4, pixels mod 4
    int elem_bytes, pixel_bytes, group_bytes;
    unsigned long long bytes;      // pixels * pixel_bytes: rfx_export_bytes
};
// false (and *out untouched) for a format or channel count the export does not have
inline bool rfx_export_plan_for(int pixels, int format, int channels, rfx_export_plan *out) {
    if (pixels <= 0 || (channels != 3 && channels != 4)) return false;
    const int elem = format == RFX_EXPORT_F32 ? 4 : format == RFX_EXPORT_F16 ? 2 : format == RFX_EXPORT_U8_SRGB ? 1 : 0;
    if (!elem) return false;
    rfx_export_plan t;
    t.pixels = pixels;
    t.groups = pixels / 4;
    t.tail_start = t.groups * 4;
    t.tail_pixels = pixels - t.tail_start;
    const int lanes = t.groups + (t.tail_pixels ? 1 : 0);
    t.blocks = (lanes + RFX_K7_BLOCK - 1) / RFX_K7_BLOCK;
    t.elem_bytes = elem;
    t.pixel_bytes = elem * channels;
    t.group_bytes = 4 * t.pixel_bytes;
    t.bytes = (unsigned long long)pixels * (unsigned long long)t.pixel_bytes;
    *out = t;
    return true;
}

// ---------------------------------------------------------------- K7 into a device image: rfx_export_device's store form and launch
// The image of include/rfx.h rfx_device_image is written where the caller keeps it: the element of column x, tile row r and channel ch goes
// stride_x x + stride_y r + stride_c ch ELEMENTS from `data`.  One form per call, uniform over the launch (k7_export.hip k7_export_strided
// branches on it per wave):
//   TIGHT        interleaved (stride_c == 1, stride_x == channels), stride_y == W x channels, `data` on a 4-byte boundary: the flat k7_export on
//                the caller's pointer over the whole run (`flat` is its plan);
//   INTERLEAVED  stride_c == 1, stride_x == channels, `data` and stride_y x element bytes multiples of 4: a lane's 4 C elements are one run of
//                whole dwords, 16 C element bytes from its neighbour's;
//   PLANAR       stride_x == 1, `data` aligned to four elements, stride_y and stride_c multiples of four elements: per channel, a lane's four
//                elements are one aligned 16- / 8- / 4-byte store (F32 / F16 / U8);
//   ELEMENT      everything else: element-wide stores.
// The strided launch: a lane owns four consecutive pixels of ONE row — groups_x = W / 4 groups per row, the W mod 4 pixels from tail_x on go to
// lane groups_x of the row, element by element; workgroups of RFX_K7_DEV_BX x RFX_K7_DEV_BY lanes (along the row x rows), grid_x x grid_y.
// The block shape: 64 lanes along the row make every wave one row segment of 256 pixels — its loads are 4 KiB of consecutive texels and its
// stores consecutive runs in every vector form, whatever the row pitch is — and 4 rows per workgroup keep the 256 lanes of k7_export, so a
// 97 x 55 frame already has 14 workgroups along the rows and a 4K row is 15 workgroups wide.
// Refused (the RFX_EINVAL case in words): a format or channel count the export does not have; data == 0; an address that is not a multiple of
// the element size; an extent, (1 + sum over the axes of |stride| (count - 1)) elements, beyond 2^62 - 1 bytes (64-bit arithmetic that cannot
// overflow); strides that do not nest — of the axes with count > 1, sorted by |stride|, the smallest must be >= 1 and every later one >= the
// one before it x that axis's count (sufficient for an image that does not alias itself, not necessary).
// A pure function of its arguments, exported as rfx_internal_export_device_plan (tests/test_export_device_cpu.py restates it).
enum { RFX_EXPORT_FORM_TIGHT = 0, RFX_EXPORT_FORM_INTERLEAVED = 1, RFX_EXPORT_FORM_PLANAR = 2, RFX_EXPORT_FORM_ELEMENT = 3 };
constexpr int RFX_K7_DEV_BX = 64, RFX_K7_DEV_BY = 4;
struct rfx_export_device_plan {
    int form;
    int elem_bytes;
    int groups_x, tail_x, tail_pixels, lanes_x;
    int grid_x, grid_y;
    rfx_export_plan flat;  // TIGHT: k7_export's plan over rows x W pixels (zeroed otherwise)
};
// addr: the image's `data` as an integer (read for alignment only); stride_*: in elements.  0, or the RFX_EINVAL case in words.
inline const char *rfx_export_device_plan_for(int W, int rows, int format, int channels, unsigned long long addr, long long stride_x, long long stride_y,
                                              long long stride_c, rfx_export_device_plan *out) {
    rfx_export_device_plan t = {};
    if (W <= 0 || rows <= 0 || (long long)W * rows > 0x7fffffffll || !rfx_export_plan_for(W * rows, format, channels, &t.flat)) return "bad format or channel count";
    if (!addr) return "dst->data is NULL";
    const unsigned long long e = (unsigned long long)t.flat.elem_bytes;
    if (addr % e) return "dst->data is not aligned to the element size";
    const unsigned long long lim = ((1ull << 62) - 1ull) / e;
    const long long s[3] = {stride_x, stride_y, stride_c};
    const int n[3] = {W, rows, channels};
    unsigned long long mag[3], total = 1;
    for (int k = 0; k < 3; k++) {
        mag[k] = s[k] < 0 ? 0ull - (unsigned long long)s[k] : (unsigned long long)s[k];
        const unsigned long long steps = (unsigned long long)(n[k] - 1);
        if (steps && mag[k] > (lim - total) / steps) return "the image's extent does not fit in 62 bits of bytes";
        total += mag[k] * steps;
    }
    // the nesting rule over the axes that step at all (every |stride| x count below is under 2^63: the extent above)
    int axis[3], m = 0;
    for (int k = 0; k < 3; k++)
        if (n[k] > 1) axis[m++] = k;
    for (int i = 1; i < m; i++)
        for (int j = i; j > 0 && mag[axis[j]] < mag[axis[j - 1]]; j--) { const int q = axis[j]; axis[j] = axis[j - 1]; axis[j - 1] = q; }
    for (int i = 0; i < m; i++) {
        if (i == 0 ? mag[axis[0]] < 1ull : mag[axis[i]] < mag[axis[i - 1]] * (unsigned long long)n[axis[i - 1]])
            return "the image's strides do not nest: the image would alias itself (include/rfx.h \"device images\")";
    }
    const long long per = (long long)(4ull / e);  // elements per dword
    const bool interleaved = stride_c == 1 && stride_x == channels;
    t.elem_bytes = (int)e;
    if (interleaved && addr % 4ull == 0 && stride_y == (long long)W * channels) t.form = RFX_EXPORT_FORM_TIGHT;
    else if (interleaved && addr % 4ull == 0 && stride_y % per == 0) t.form = RFX_EXPORT_FORM_INTERLEAVED;
    else if (stride_x == 1 && addr % (4ull * e) == 0 && stride_y % 4 == 0 && stride_c % 4 == 0) t.form = RFX_EXPORT_FORM_PLANAR;
    else t.form = RFX_EXPORT_FORM_ELEMENT;
    t.groups_x = W / 4;
    t.tail_x = t.groups_x * 4;
    t.tail_pixels = W - t.tail_x;
    t.lanes_x = t.groups_x + (t.tail_pixels ? 1 : 0);
    t.grid_x = (t.lanes_x + RFX_K7_DEV_BX - 1) / RFX_K7_DEV_BX;
    t.grid_y = (rows + RFX_K7_DEV_BY - 1) / RFX_K7_DEV_BY;
    if (t.form != RFX_EXPORT_FORM_TIGHT) t.flat = rfx_export_plan{};
    *out = t;
    return nullptr;
}

// ---------------------------------------------------------------- K8: the PNG fragment's buffers
// rfx_png_bound and the layout of the device buffer behind one staged PNG: the result (header + fragment, `bound` bytes), one scratch slot
// per scanline (a whole chunk in its stored form, rounded up to dwords, plus one dword: the bit window leaves as whole dwords), the per-scanline
// sizes and Adler partial sums, the chunk offsets.  A pure function of its arguments.
struct rfx_png_plan {
    int rows, rowbytes, line_bytes, stored_blocks;  // line_bytes = n = 1 + W * channels
    unsigned slot_stride;
    unsigned long long bound, slots_at, meta_at, offsets_at, device_bytes;
};
inline bool rfx_png_plan_for(int rows, int W, int channels, rfx_png_plan *out) {
    if (rows <= 0 || W <= 0 || (channels != 3 && channels != 4)) return false;
    rfx_png_plan t;
    t.rows = rows;
    t.rowbytes = W * channels;
    t.line_bytes = t.rowbytes + 1;
    t.stored_blocks = (t.line_bytes + 65534) / 65535;
    const unsigned long long chunk = 12ull + 5ull * (unsigned long long)t.stored_blocks + (unsigned long long)t.line_bytes;
    t.bound = 32ull + (unsigned long long)rows * chunk;
    t.slot_stride = (unsigned)((chunk + 3ull) & ~3ull) + 4u;
    t.slots_at = (t.bound + 255ull) & ~255ull;
    t.meta_at = t.slots_at + (((unsigned long long)rows * t.slot_stride + 255ull) & ~255ull);
    t.offsets_at = t.meta_at + (((unsigned long long)rows * 16ull + 255ull) & ~255ull);
    t.device_bytes = t.offsets_at + (unsigned long long)rows * 8ull;
    *out = t;
    return true;
}

// ---------------------------------------------------------------- K8: the EXR fragment's buffers
// rfx_exr_bound and the layout of the device buffer behind one staged EXR fragment: the result (header + fragment, `bound` bytes), one scratch
// slot per scanline (a whole chunk in its raw form, rounded up to dwords, plus one dword: the bit window leaves as whole dwords), one byte
// plane per scanline (n bytes rounded up to dwords: the coder reads it dword-wise), the per-scanline sizes, the chunk offsets.  A pure function
// of its arguments.
struct rfx_exr_plan {
    int rows, width, channels, line_bytes;  // line_bytes = n = W * channels * 2
    unsigned slot_stride, plane_stride;
    unsigned long long bound, slots_at, planes_at, meta_at, offsets_at, device_bytes;
};
inline bool rfx_exr_plan_for(int rows, int W, int channels, rfx_exr_plan *out) {
    if (rows <= 0 || rows > 65535 || W <= 0 || (channels != 3 && channels != 4)) return false;
    rfx_exr_plan t;
    t.rows = rows; t.width = W; t.channels = channels;
    t.line_bytes = 2 * W * channels;
    const unsigned long long chunk = 8ull + (unsigned long long)t.line_bytes;
    t.bound = 32ull + (unsigned long long)rows * chunk;
    t.slot_stride = (unsigned)((chunk + 3ull) & ~3ull) + 4u;
    t.plane_stride = ((unsigned)t.line_bytes + 3u) & ~3u;
    t.slots_at = (t.bound + 255ull) & ~255ull;
    t.planes_at = t.slots_at + (((unsigned long long)rows * t.slot_stride + 255ull) & ~255ull);
    t.meta_at = t.planes_at + (((unsigned long long)rows * t.plane_stride + 255ull) & ~255ull);
    t.offsets_at = t.meta_at + (((unsigned long long)rows * 16ull + 255ull) & ~255ull);
    t.device_bytes = t.offsets_at + (unsigned long long)rows * 8ull;
    *out = t;
    return true;
}

// K9's PIZ table scratch (k9_piz.h): one slot per PIZ stream of a call — blocks in flight are the blocks of the call, every one its own wave —, each
// the reverse lookup table (65536 x 2 bytes), the sorted symbol list (65537 x 2 bytes, rounded up to 256) and the info words (256).  A pure
// function of its argument, exported as rfx_internal_exr_piz_tables.
constexpr int RFX_EXR_PIZ_CELL = 64;  // the side of a wavelet cell: a block with both sides >= 2 cells is refused (include/rfx.h)
struct rfx_exr_piz_tables { unsigned long long rev_bytes, symbol_bytes, info_bytes, slot_bytes, bytes; };
inline bool rfx_exr_piz_tables_for(int piz_blocks, rfx_exr_piz_tables *out) {
    if (piz_blocks < 0 || piz_blocks >= (1 << 23)) return false;
    rfx_exr_piz_tables t;
    t.rev_bytes = 65536ull * 2ull;
    t.symbol_bytes = (65537ull * 2ull + 255ull) & ~255ull;
    t.info_bytes = 256ull;
    t.slot_bytes = t.rev_bytes + t.symbol_bytes + t.info_bytes;
    t.bytes = t.slot_bytes * (unsigned long long)piz_blocks;
    *out = t;
    return true;
}

// ---------------------------------------------------------------- K0 AOV staging: rfx_stage_aov's rows, staging area and launches
// The planes of an AOV frame (include/rfx.h rfx_aov_frame, in the struct's order) cover the band [row0, row0 + rows) of the frame.  DEPTH is held
// whole, GBUFFER / VELOCITY / DIRECT_LIGHT hold the rows [held_row0, held_row0 + held_rows), so the band falls into at most three SEGMENTS of
// whole rows: the rows below the held ones and the rows above them, where only depth is written (`full` 0), and the rows in between, where every
// slot the frame names is written (`full` 1).  On a whole-frame context, or when the frame names no slot but DEPTH, there is one segment.  A
// plane is copied for the rows of the segments that read it — depth for all of them, every other plane for the full one — each piece to a
// 256-byte-aligned offset of the context's staging area, and every segment is one launch over its flat run of `pixels` = rows * W texels: lane
// t < groups owns the pixels [4 t, 4 t + 4), the pixels [tail_start, pixels) go to the lane after the last group (rfx_export_plan_for's shape).
// A pure function of its arguments, exported as rfx_internal_aov_plan (tests/test_stage_aov_cpu.py restates the row rule).
enum { RFX_AOV_DIFFUSE, RFX_AOV_NORMAL, RFX_AOV_ROUGHNESS, RFX_AOV_METALNESS, RFX_AOV_EMISSIVE, RFX_AOV_VELOCITY, RFX_AOV_DEPTH, RFX_AOV_DIRECT, RFX_AOV_PLANES };
constexpr int RFX_K0_AOV_BLOCK = 256;
struct rfx_aov_segment {
    int row0, rows, full;
    int pixels, groups, blocks, tail_start, tail_pixels;
    unsigned long long offset[RFX_AOV_PLANES];  // of the plane's rows of this segment in the staging area; ~0: the segment does not read the plane
};
struct rfx_aov_plan {
    int nseg;
    rfx_aov_segment seg[3];
    int plane_row0[RFX_AOV_PLANES], plane_rows[RFX_AOV_PLANES];  // the frame rows of each plane that are copied (rows 0: none)
    int elem_bytes[RFX_AOV_PLANES];                              // 4 / 2 / 0 (the plane is not given)
    int write_gbuffer, write_velocity, write_direct;            // the slots the frame names besides DEPTH
    unsigned long long copy_bytes, stage_bytes;                  // host -> device bytes (rfx_aov_stage_bytes); the staging area
};
// type / channels: per plane, channels 0 = the plane is not given.  0, or the RFX_EINVAL case in words.
// depth_kind, velocity_kind: include/rfx.h "AOV conventions" — under POSITION the depth plane has three channels; under CAMERAS there is no
// velocity plane and VELOCITY is written iff normal is given.  (0, 0): rfx_aov_plan_for.
inline const char *rfx_aov_plan_conv_for(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, int row0, int rows, int depth_kind,
                                         int velocity_kind, rfx_aov_plan *out) {
    const bool position = depth_kind == RFX_AOV_DEPTH_POSITION, cameras = velocity_kind == RFX_AOV_VELOCITY_CAMERAS;
    const int want[RFX_AOV_PLANES] = {4, 3, 1, 1, 3, 2, position ? 3 : 1, 4};
    if (depth_kind < 0 || depth_kind > RFX_AOV_DEPTH_POSITION || velocity_kind < 0 || velocity_kind > RFX_AOV_VELOCITY_CAMERAS) return "an unknown depth or velocity kind";
    if (W <= 0 || H <= 0 || held_rows < 0) return "bad geometry";
    rfx_aov_plan t = {};
    for (int i = 0; i < RFX_AOV_PLANES; i++) {
        if (!channels[i]) continue;
        if (type[i] != RFX_PLANE_F32 && type[i] != RFX_PLANE_F16) return "a plane's type must be RFX_PLANE_F32 or RFX_PLANE_F16";
        const bool rgb_or_rgba = i == RFX_AOV_DIFFUSE || i == RFX_AOV_DIRECT;
        if (channels[i] != want[i] && !(rgb_or_rgba && channels[i] == 3))
            return i == RFX_AOV_DEPTH && (position || channels[i] == 3) ? "the depth plane holds a world position (3 channels) under RFX_AOV_DEPTH_POSITION and under it alone"
                                                                         : "a plane's channel count (diffuse, direct: 3 or 4; normal, emissive: 3; velocity: 2; the others: 1)";
        t.elem_bytes[i] = type[i] == RFX_PLANE_F16 ? 2 : 4;
    }
    if (!channels[RFX_AOV_DEPTH]) return "the depth plane is required";
    const bool normal = channels[RFX_AOV_NORMAL] != 0;
    const int g = (channels[RFX_AOV_DIFFUSE] != 0) + (channels[RFX_AOV_ROUGHNESS] != 0) + (channels[RFX_AOV_METALNESS] != 0) + (channels[RFX_AOV_EMISSIVE] != 0);
    t.write_gbuffer = g == 4 && normal;
    if (cameras && channels[RFX_AOV_VELOCITY]) return "a velocity plane under RFX_AOV_VELOCITY_CAMERAS";
    t.write_velocity = cameras ? normal : channels[RFX_AOV_VELOCITY] != 0;
    t.write_direct = channels[RFX_AOV_DIRECT] != 0;
    if (t.write_velocity && !normal) return "a velocity plane needs the normal plane";
    if (!t.write_gbuffer && (g != 0 || (normal && !t.write_velocity)))
        return "diffuse, normal, roughness, metalness and emissive come together (all five write GBUFFER) or not at all";
    if (rows <= 0 || row0 < 0 || row0 + rows > H) return "row band outside the rows DEPTH holds";
    // band ∩ held rows
    int a = row0 > held_row0 ? row0 : held_row0, b = row0 + rows < held_row0 + held_rows ? row0 + rows : held_row0 + held_rows;
    if (!(t.write_gbuffer || t.write_velocity || t.write_direct) || b <= a) a = b = row0 + rows;  // (no full segment: the band is "below")
    const int cut[4] = {row0, a, b, row0 + rows};
    for (int k = 0; k < 3; k++) {
        if (cut[k + 1] <= cut[k]) continue;
        rfx_aov_segment &s = t.seg[t.nseg++];
        s.row0 = cut[k]; s.rows = cut[k + 1] - cut[k]; s.full = k == 1;
        s.pixels = s.rows * W;  // (< 2^28: rfx_create)
        s.groups = s.pixels / 4;
        s.tail_start = s.groups * 4;
        s.tail_pixels = s.pixels - s.tail_start;
        s.blocks = (s.groups + (s.tail_pixels ? 1 : 0) + RFX_K0_AOV_BLOCK - 1) / RFX_K0_AOV_BLOCK;
        for (int i = 0; i < RFX_AOV_PLANES; i++) {
            s.offset[i] = ~0ull;
            if (!channels[i] || (i != RFX_AOV_DEPTH && !s.full)) continue;
            s.offset[i] = t.stage_bytes;
            const unsigned long long bytes = (unsigned long long)s.pixels * (unsigned long long)(channels[i] * t.elem_bytes[i]);
            t.copy_bytes += bytes;
            t.stage_bytes += (bytes + 255ull) & ~255ull;
            if (!t.plane_rows[i]) t.plane_row0[i] = s.row0;
            t.plane_rows[i] += s.rows;  // (depth's segments are adjacent: one run of rows)
        }
    }
    *out = t;
    return nullptr;
}
inline const char *rfx_aov_plan_for(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, int row0, int rows, rfx_aov_plan *out) {
    return rfx_aov_plan_conv_for(W, H, held_row0, held_rows, type, channels, row0, rows, RFX_AOV_DEPTH_FRAGCOORD, RFX_AOV_VELOCITY_UV, out);
}

// ---------------------------------------------------------------- K0 device planes: rfx_stage_aov_device's layouts and launches
// The planes of include/rfx.h rfx_aov_device_frame are read where the producer left them: the element of frame column x, band row r and channel
// ch of plane i sits stride_x x + stride_y r + stride_c ch ELEMENTS from its `data`.  Rows, segments, written slots and every refusal of
// rfx_stage_aov come from rfx_aov_plan_conv_for (`rows` below; its staging offsets only say which planes a segment reads).  On top of that:
//   layout[i]    the plane's class, uniform over the call (the kernel branches on it per wave, k0_import.hip k0_aov_pack_strided):
//                INTERLEAVED  stride_c == 1 and stride_x == channels — a lane's 4 C elements are contiguous;
//                PLANAR       stride_x == 1 — per channel, a lane's four elements are contiguous;
//                both only when `data` is aligned to four elements and stride_y (PLANAR: stride_c too) is a multiple of four, so that every
//                lane's run starts on a 16-byte (halves: 8-byte) boundary in every row; ELEMENT otherwise.  A 1-channel plane has no stride_c.
//   flat[k]      segment k is served by k0_aov_pack on the caller's pointers: every plane it reads is interleaved with stride_y == W x channels
//                and starts, in the segment's first row, on a 16-byte boundary — the staging area's layout.
//   seg_offset   elements from `data` to the segment's first row.
//   the strided launch: a lane owns four consecutive pixels of ONE row — groups_x = W / 4 groups per row, the W mod 4 pixels from tail_x on go
//   to lane groups_x of the row, element by element; workgroups of RFX_K0_DEV_BX x RFX_K0_DEV_BY lanes (along the row x rows), grid_x x grid_y[k].
// Refused on top of rfx_aov_plan_conv_for's cases: an address that is not a multiple of the element size; a plane whose extent over the band,
// (1 + sum over the axes of |stride| (count - 1)) elements, does not fit in 2^62 - 1 bytes (64-bit arithmetic that cannot overflow).
// A pure function of its arguments, exported as rfx_internal_aov_device_plan (tests/test_stage_aov_device_cpu.py restates it).
enum { RFX_AOV_LAYOUT_NONE = 0, RFX_AOV_LAYOUT_INTERLEAVED = 1, RFX_AOV_LAYOUT_PLANAR = 2, RFX_AOV_LAYOUT_ELEMENT = 3 };
constexpr int RFX_K0_DEV_BX = 64, RFX_K0_DEV_BY = 4;
struct rfx_aov_device_plan {
    rfx_aov_plan rows;
    int layout[RFX_AOV_PLANES];
    int flat[3];
    int groups_x, tail_x, tail_pixels, lanes_x;
    int grid_x, grid_y[3];
    long long seg_offset[3][RFX_AOV_PLANES];
};
// addr: the planes' `data` as integers (read for alignment only); stride_*: in elements.  0, or the RFX_EINVAL case in words.
inline const char *rfx_aov_device_plan_for(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, const unsigned long long *addr,
                                           const long long *stride_x, const long long *stride_y, const long long *stride_c, int row0, int rows, int depth_kind,
                                           int velocity_kind, rfx_aov_device_plan *out) {
    rfx_aov_device_plan t = {};
    if (const char *bad = rfx_aov_plan_conv_for(W, H, held_row0, held_rows, type, channels, row0, rows, depth_kind, velocity_kind, &t.rows)) return bad;
    long long sc[RFX_AOV_PLANES];
    for (int i = 0; i < RFX_AOV_PLANES; i++) {
        if (!channels[i]) continue;
        const unsigned long long e = (unsigned long long)t.rows.elem_bytes[i];
        if (addr[i] % e) return "a plane's data is not aligned to its element size";
        sc[i] = channels[i] > 1 ? stride_c[i] : 1;
        // the extent in elements, kept below lim at every step
        const unsigned long long lim = ((1ull << 62) - 1ull) / e;
        const long long s[3] = {stride_x[i], stride_y[i], channels[i] > 1 ? stride_c[i] : 0};
        const int n[3] = {W, rows, channels[i]};
        unsigned long long total = 1;
        for (int k = 0; k < 3; k++) {
            const unsigned long long mag = s[k] < 0 ? 0ull - (unsigned long long)s[k] : (unsigned long long)s[k], steps = (unsigned long long)(n[k] - 1);
            if (steps && mag > (lim - total) / steps) return "a plane's extent does not fit in 62 bits of bytes";
            total += mag * steps;
        }
        const bool aligned4 = addr[i] % (4ull * e) == 0 && stride_y[i] % 4 == 0;
        if (sc[i] == 1 && stride_x[i] == channels[i]) t.layout[i] = aligned4 ? RFX_AOV_LAYOUT_INTERLEAVED : RFX_AOV_LAYOUT_ELEMENT;
        else if (stride_x[i] == 1) t.layout[i] = aligned4 && sc[i] % 4 == 0 ? RFX_AOV_LAYOUT_PLANAR : RFX_AOV_LAYOUT_ELEMENT;
        else t.layout[i] = RFX_AOV_LAYOUT_ELEMENT;
    }
    t.groups_x = W / 4;
    t.tail_x = t.groups_x * 4;
    t.tail_pixels = W - t.tail_x;
    t.lanes_x = t.groups_x + (t.tail_pixels ? 1 : 0);
    t.grid_x = (t.lanes_x + RFX_K0_DEV_BX - 1) / RFX_K0_DEV_BX;
    for (int k = 0; k < t.rows.nseg; k++) {
        const rfx_aov_segment &g = t.rows.seg[k];
        t.grid_y[k] = (g.rows + RFX_K0_DEV_BY - 1) / RFX_K0_DEV_BY;
        t.flat[k] = 1;
        for (int i = 0; i < RFX_AOV_PLANES; i++) {
            if (g.offset[i] == ~0ull) continue;
            t.seg_offset[k][i] = (long long)(g.row0 - row0) * stride_y[i];  // (inside the extent checked above)
            const unsigned long long first = addr[i] + (unsigned long long)t.seg_offset[k][i] * (unsigned long long)t.rows.elem_bytes[i];
            const bool tight = sc[i] == 1 && stride_x[i] == channels[i] && stride_y[i] == (long long)W * channels[i];
            if (!tight || first % 16ull) t.flat[k] = 0;
        }
    }
    *out = t;
    return nullptr;
}

// ---------------------------------------------------------------- shared by the launchers
// Every view is the whole frame (a context that owns no row tile; a null pointer counts as whole): the kernels then skip row rebasing and
// halo accounting.  TexView and TexViewW alike.
template <class... V>
inline bool rfx_views_whole(int H, const V &...v) {
    return ((v.ptr == nullptr || (v.row0 == 0 && v.rows == H)) && ...);
}

// A run-time option becomes a template argument: f is called with the std::integral_constant of the value, and a kernel is instantiated for
// exactly the values a call lists.  rfx_with_int returns false (and calls nothing) when x is none of Vs.
template <class F>
inline void rfx_with_bool(bool b, F &&f) {
    b ? f(std::true_type{}) : f(std::false_type{});
}
template <int... Vs, class F>
inline bool rfx_with_int(int x, F &&f) {
    return ((x == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// A value asked for once per kernel and device (a process may hold contexts on several devices): K3's "dynamic-LDS attribute set", K1's
// blocks per CU.  Beyond 64 device ordinals nothing is remembered.
template <auto Kernel, class T, class F>
inline T rfx_per_device(F &&get) {
    static T value[64];
    static bool have[64] = {false};
    int dev = 0;
    hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) return get();
    if (!have[dev]) { value[dev] = get(); have[dev] = true; }
    return value[dev];
}
