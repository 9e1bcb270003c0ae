// rfx_draw.hip — the C ABI's draws K1–K5 (rfx_ssgi_march / _trace / _shade, rfx_temporal_reproject, rfx_copy_framebuffer, rfx_poisson_denoise,
// rfx_compose, rfx_final_compose), the traced rays' row masks, and the launch plans of rfx_launch.h as the library computes them (rfx_internal_*).
#include <math.h>
#include "rfx_host.h"

// The rows of an Hs-row smaller target (resolutionScale != 1) this context's RFX_TEX_SSGI holds, stored from the start of the slot: all of them on
// a whole-frame context; on a row tile the rows K2's staging of the tile addresses (rfx_launch.h rfx_scaled_rows), with the apron min(halo, 2)
// K1 widens its launch by at scale 1.  rfx_set_row_window does not apply: K2 under a window reads rows K1 has drawn regardless.
static rfx_scaled_rows_plan ctx_scaled_rows(const rfx_ctx *c, int Hs) {
    if (c->tile_y0 == 0 && c->tile_rows == c->H) return {0, Hs};
    return rfx_scaled_rows(rfx_uv_planes(c->uv_model, c->W, c->H), Hs, c->tile_y0, c->tile_y0 + c->tile_rows, c->halo < 2 ? c->halo : 2);
}
// ... and whether they fit the slot (sized for the held band at full width) and the trace -> shade hand-over plane (sized like it)
static bool scaled_rows_fit(const rfx_ctx *c, int Ws, const rfx_scaled_rows_plan &t) {
    return (size_t)(t.j1 - t.j0) * Ws <= (size_t)c->slots[RFX_TEX_SSGI].rows * c->W;
}
// Is `rs` a resolutionScale this context can draw at, and the size of its target (SSGIPass.setSize :52-57)?  The caller words the error.
static bool scaled_target(const rfx_ctx *c, float rs, int *Ws, int *Hs) {
    const float fw = (float)c->W * rs, fh = (float)c->H * rs;
    if (!(rs > 0.0f && rs <= 1.0f) || fw != floorf(fw) || fh != floorf(fh) || fw < 1.0f || fh < 1.0f) return false;
    *Ws = (int)fw; *Hs = (int)fh;
    return true;
}
static int need(rfx_ctx *c, const int *ids, int n) {
    for (int i = 0; i < n; i++) {
        int rc = ensure(c, ids[i]);
        if (rc) return rc;
    }
    return RFX_OK;
}

// ---- K1: rfx_ssgi_march / _trace / _shade.  ssgi_draw (below) runs these steps in order.
static int ssgi_history_slot(const rfx_ssgi_params *p) {
    return p->historySource == 1 ? RFX_TEX_TEMPORAL0 : (p->historySource == 3 ? RFX_TEX_COMPOSE_RGB : RFX_TEX_COMPOSE);
}
static float ssgi_resolution_scale(const rfx_ssgi_params *p) { return p->resolutionScale == 0.0f ? 1.0f : p->resolutionScale; }

// step 1: the parameters and the context's state; makes the slots the draw touches
static int ssgi_validate(rfx_ctx *c, const rfx_ssgi_params *p) {
    if (!c || !p) return RFX_EINVAL;
    if (p->mode != 0 && p->mode != 1) return fail(c, RFX_EINVAL, "rfx_ssgi_march/trace/shade: mode must be 0 (MODE_SSGI) or 1 (MODE_SSR)");
    if (p->importanceSampling && (!p->useEnvMap || !c->env_tables_set))
        return fail(c, RFX_ESTATE, "rfx_ssgi_march/trace/shade: importanceSampling needs useEnvMap and rfx_set_environment_importance");
    if (p->useEnvMap && !c->env) return fail(c, RFX_ESTATE, "rfx_ssgi_march/trace/shade: useEnvMap without rfx_set_environment");
    if (p->steps < 1 || p->refineSteps < 0) return fail(c, RFX_EINVAL, "rfx_ssgi_march/trace/shade: steps/refineSteps");
    RFX_ENTER(c);
    if (p->historySource < 0 || p->historySource > 3) return fail(c, RFX_EINVAL, "rfx_ssgi_march/trace/shade: historySource");
    if (p->historySource == 1 && (c->tile_y0 != 0 || c->tile_rows != c->H))
        return fail(c, RFX_EUNSUPPORTED, "rfx_ssgi_march/trace/shade: historySource TEMPORAL0 (denoiseMode \"temporal\") needs a whole-frame context: K1 gathers it anywhere on screen");
    const int ids[] = {RFX_TEX_DEPTH, RFX_TEX_GBUFFER, RFX_TEX_DIRECT_LIGHT, ssgi_history_slot(p), RFX_TEX_BLUE_NOISE, RFX_TEX_SSGI};
    int rc = need(c, ids, 6);
    if (rc) return rc;
    if (!c->slots[RFX_TEX_DEPTH].uploaded || !c->slots[RFX_TEX_GBUFFER].uploaded || !c->slots[RFX_TEX_BLUE_NOISE].uploaded)
        return fail(c, RFX_ESTATE, "rfx_ssgi_march/trace/shade: depth / gbuffer / blue-noise not uploaded");
    const float rs = ssgi_resolution_scale(p);
    if (rs != 1.0f) {
        int Ws, Hs;
        if (!scaled_target(c, rs, &Ws, &Hs)) return fail(c, RFX_EINVAL, "rfx_ssgi_march/trace/shade: resolutionScale must be in (0, 1] with whole W*s and H*s");
        if (!scaled_rows_fit(c, Ws, ctx_scaled_rows(c, Hs)))
            return fail(c, RFX_EINVAL, "rfx_ssgi_march/trace/shade: the target rows of this tile at this resolutionScale do not fit the held band (more halo rows)");
    }
    return RFX_OK;
}

// step 3: K1's scratch — the view-Z plane, the base cells, the march's table, the tile counter, the foreground maps: all five buffers or none
static int k1_scratch(rfx_ctx *c, const rfx_k1_table_plan &T, int coarse_w, int coarse_h) {
    if (c->viewz) return RFX_OK;
    hipError_t e = hipMalloc((void **)&c->viewz, (size_t)c->W * c->H * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&c->coarse, (size_t)coarse_w * coarse_h * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc((void **)&c->cells, (size_t)T.vec4 * 16);
    if (e == hipSuccess) e = hipMalloc((void **)&c->k1_tiles, 64 * 128);
    // the two foreground maps (rfx_ctx.h): ceil(W / 64) x ceil(H / 8) bytes each, 16 KiB at 4K, in whole 256-byte units (K3 reads a byte's word)
    c->fg_w = (c->W + 63) / 64;
    c->fg_stride = (((size_t)c->fg_w * ((c->H + 7) / 8)) + 255) & ~(size_t)255;
    if (e == hipSuccess) e = hipMalloc((void **)&c->fg_tiles, 2 * c->fg_stride);
    if (e == hipSuccess) return RFX_OK;
    // a later draw must not find viewz set and the tables missing
    if (c->viewz) hipFree(c->viewz);
    if (c->coarse) hipFree(c->coarse);
    if (c->cells) hipFree(c->cells);
    if (c->k1_tiles) hipFree(c->k1_tiles);
    if (c->fg_tiles) hipFree(c->fg_tiles);
    c->viewz = nullptr; c->coarse = nullptr; c->cells = nullptr; c->k1_tiles = nullptr; c->fg_tiles = nullptr;
    return fail(c, RFX_ENOMEM, "hipMalloc(K1 scratch)", e);
}

// ... and, for a split draw, the trace -> shade hand-over plane
static int k1_hand_over(rfx_ctx *c, int stage) {
    if (stage == 0) return RFX_OK;
    // indexed like the output texture (a scaled target's rows are checked against W * held rows: ssgi_validate)
    const size_t n = (size_t)c->W * c->slots[RFX_TEX_SSGI].rows * 2;
    if (stage == 2 && (!c->hits || !c->hits_traced)) return fail(c, RFX_ESTATE, "rfx_ssgi_shade: no rfx_ssgi_trace of this frame to finish");
    if (!c->hits) {
        hipError_t e = hipMalloc((void **)&c->hits, n * sizeof(float4));
        if (e != hipSuccess) return fail(c, RFX_ENOMEM, "hipMalloc(K1 trace hand-over)", e);
    }
    return RFX_OK;
}

// step 4: the argument block (no HIP call).  Returns whether the march has rows to produce.
static bool k1_args(rfx_ctx *c, const rfx_ssgi_params *p, int stage, const rfx_k1_table_plan &T, int coarse_w, int coarse_h, K1Args &A) {
    A.dims = dims(c);
    // K2's neighbourhood clamp reads +-2 rows of K1's output: produce them redundantly in the halo
    bool any = launch_rows(c, RFX_TEX_SSGI, c->halo < 2 ? c->halo : 2, &A.y0, &A.y1);
    A.out_w = c->W; A.out_h = c->H;
    const float rs = ssgi_resolution_scale(p);
    int out_j0 = 0;
    if (rs != 1.0f) {  // (validated: whole W * rs and H * rs, target rows that fit the slot)
        A.out_w = (int)((float)c->W * rs); A.out_h = (int)((float)c->H * rs);
        const rfx_scaled_rows_plan t = ctx_scaled_rows(c, A.out_h);  // TARGET rows: every one, or the rows K2's staging of this tile addresses
        A.y0 = out_j0 = t.j0; A.y1 = t.j1;
        any = t.j1 > t.j0;  // the row window does not apply to the scaled target
    }
    A.out_uv = rfx_uv_planes(c->uv_model, A.out_w, A.out_h);
    A.depth = view(c, RFX_TEX_DEPTH); A.gbuffer = view(c, RFX_TEX_GBUFFER); A.direct = view(c, RFX_TEX_DIRECT_LIGHT);
    A.history = view(c, ssgi_history_slot(p));
    A.blue = c->slots[RFX_TEX_BLUE_NOISE].ptr;
    blue_noise_shift(p->blueNoiseIndex, &A.shift_x, &A.shift_y);
    A.out = wview(c, RFX_TEX_SSGI);
    // a scaled tile keeps its target rows [j0, j1) at the start of the slot: the kernel addresses target row y at y * out_w, so it is handed the
    // address row 0 WOULD have (never dereferenced below row j0: the launch draws [j0, j1), which scaled_rows_fit has checked against the slot)
    A.out.ptr = (void *)((uintptr_t)A.out.ptr - (size_t)out_j0 * A.out_w * sizeof(uint4));
    A.p = *p;
    // SSGIPass.js:84-87: computed in JS doubles, then rounded to float uniforms
    A.nearMulFar = (float)((double)p->camera.near_ * (double)p->camera.far_);
    A.farMinusNear = (float)((double)p->camera.far_ - (double)p->camera.near_);
    A.nearMinusFar = (float)((double)p->camera.near_ - (double)p->camera.far_);
    A.coarse_w = coarse_w; A.coarse_h = coarse_h;
    A.cell_shift = T.cell_shift; A.cells_w = T.cells_w; A.cells_h = T.cells_h;
    A.cells_pitch = T.pitch; A.cells_pitch_log2 = T.pitch_log2; A.cells_pow2 = T.pow2; A.cells_vec4 = T.vec4;
    A.viewz = c->viewz; A.coarse = c->coarse; A.cells = c->cells;
    A.tile_counter = c->k1_tiles; A.n_cu = c->n_cu;
    // the pre-pass fills the foreground map the previous pre-pass did not: that one is still read by the K3 draws queued since (the pre-pass
    // runs under them; it waits for ev_k1_done, i.e. for every draw that read the map it overwrites)
    A.fg_tiles = c->fg_tiles + (size_t)(c->fg_cur ^ 1) * c->fg_stride;
    A.fg_w = c->fg_w;
    A.env = c->env;
    A.env_w = c->env_w; A.env_h = c->env_h; A.env_levels = c->env_levels;
    A.env_marginal = c->env_marginal; A.env_conditional = c->env_conditional;
    A.totalSumWhole = c->env_sum_whole; A.totalSumDecimal = c->env_sum_decimal;
    A.env_sums = c->env_sums_on_device ? rfx_env_tables_sums(c->env_k10) : nullptr;
    memcpy(A.env_off, c->env_off, sizeof A.env_off);
    {   // getMaxMipLevel (src/ssgi/utils/Utils.js:30-34): floor(log2(max(w, h))) + 1
        int m = c->env_w > c->env_h ? c->env_w : c->env_h, lg = 0;
        while ((m >> (lg + 1)) > 0) lg++;
        A.maxEnvMapMipLevel = c->env ? (float)(lg + 1) : 0.0f;
    }
    A.hits = stage != 0 ? (float4 *)((uintptr_t)c->hits - (size_t)out_j0 * A.out_w * 2 * sizeof(float4)) : nullptr;  // (rebased like `out`)
    return any;
}

// step 5: the depth pre-pass.  It runs on EVERY draw but the shade stage's (which reuses the trace's): the depth plane is an input that changes
// every frame.  On its own stream (rfx_ctx.h prep_stream) unless the depth plane lives in a caller's buffer: after the depth plane's last
// writer and after the previous K1 launch (which read the scratch planes), NOT after the draws queued since — it overlaps them.
static int k1_prepass(rfx_ctx *c, const K1Args &A) {
    if (c->depth_external) {
        ProfScope prof(c, RFX_PROF_K1_PREPASS, c->stream);
        HIPCHK(c, rfx_launch_k1_prepare(A, c->stream));
    } else {
        if (c->depth_event_set) HIPCHK(c, hipStreamWaitEvent(c->prep_stream, c->ev_depth, 0));
        if (c->k1_event_set) HIPCHK(c, hipStreamWaitEvent(c->prep_stream, c->ev_k1_done, 0));
        {
            ProfScope prof(c, RFX_PROF_K1_PREPASS, c->prep_stream);
            HIPCHK(c, rfx_launch_k1_prepare(A, c->prep_stream));
        }
        HIPCHK(c, hipEventRecord(c->ev_prep_done, c->prep_stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_prep_done, 0));
    }
    c->fg_cur ^= 1;            // (the map k1_args pointed the pre-pass at)
    c->fg_gen = c->depth_gen;  // the map describes the depth plane as it is now: every later writer of the slot bumps depth_gen
    return RFX_OK;
}

// stage 0: rfx_ssgi_march (one launch); 1: rfx_ssgi_trace; 2: rfx_ssgi_shade
static int ssgi_draw(rfx_ctx *c, const rfx_ssgi_params *p, int stage) {
    int rc = ssgi_validate(c, p);
    if (rc) return rc;
    const rfx_k1_table_plan T = rfx_k1_table(c->W, c->H);  // step 2
    const int base = rfx_k1_base_cell(), coarse_w = (c->W + base - 1) / base, coarse_h = (c->H + base - 1) / base;
    if ((rc = k1_scratch(c, T, coarse_w, coarse_h))) return rc;
    if ((rc = k1_hand_over(c, stage))) return rc;
    K1Args A;
    const bool any = k1_args(c, p, stage, T, coarse_w, coarse_h, A);
    if (stage != 2 && (rc = k1_prepass(c, A))) return rc;
    // step 6: the march.  Its kernel hands its tiles out from a counter: the pre-pass zeroes it; the shade stage has no pre-pass of its own
    if (any && stage == 2) HIPCHK(c, hipMemsetAsync(c->k1_tiles, 0, 64 * 128, c->stream));
    if (any) {
        ProfScope prof(c, RFX_PROF_K1_MARCH, c->stream);
        HIPCHK(c, rfx_launch_k1(A, stage, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev_k1_done, c->stream));  // the next pre-pass overwrites what this launch reads
    c->k1_event_set = true;
    c->hits_traced = stage == 1;
    if (stage == 1) { c->trace_y0 = A.y0; c->trace_y1 = any ? A.y1 : A.y0; c->trace_missed = p->missedRays; c->trace_scaled = ssgi_resolution_scale(p) != 1.0f; c->trace_out_w = A.out_w; c->trace_out_h = A.out_h; }
    return RFX_OK;
}

extern "C" {

// the launch plans as built, for the CPU tests (rfx_launch.h)
int rfx_internal_k1_table(int W, int H, struct rfx_k1_table_plan *out) {
    *out = rfx_k1_table(W, H);
    return RFX_OK;
}
int rfx_internal_scaled_rows(int W, int H, int Hs, int uv_model, int y0, int y1, int apron, int *j0, int *j1) {
    const rfx_scaled_rows_plan t = rfx_scaled_rows(rfx_uv_planes(uv_model, W, H), Hs, y0, y1, apron);
    *j0 = t.j0; *j1 = t.j1;
    return RFX_OK;
}
int rfx_internal_export_plan(int pixels, int format, int channels, struct rfx_export_plan *out) {
    return rfx_export_plan_for(pixels, format, channels, out) ? RFX_OK : RFX_EINVAL;
}
int rfx_internal_export_device_plan(int W, int rows, int format, int channels, unsigned long long addr, long long stride_x, long long stride_y, long long stride_c,
                                    struct rfx_export_device_plan *out) {
    return rfx_export_device_plan_for(W, rows, format, channels, addr, stride_x, stride_y, stride_c, out) ? RFX_EINVAL : RFX_OK;
}
int rfx_internal_aov_plan(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, int row0, int rows, struct rfx_aov_plan *out) {
    return rfx_aov_plan_for(W, H, held_row0, held_rows, type, channels, row0, rows, out) ? RFX_EINVAL : RFX_OK;
}
int rfx_internal_aov_plan_conv(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, int row0, int rows, int depth_kind, int velocity_kind,
                               struct rfx_aov_plan *out) {
    return rfx_aov_plan_conv_for(W, H, held_row0, held_rows, type, channels, row0, rows, depth_kind, velocity_kind, out) ? RFX_EINVAL : RFX_OK;
}
int rfx_internal_aov_device_plan(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, const unsigned long long *addr,
                                 const long long *stride_x, const long long *stride_y, const long long *stride_c, int row0, int rows, int depth_kind, int velocity_kind,
                                 struct rfx_aov_device_plan *out) {
    return rfx_aov_device_plan_for(W, H, held_row0, held_rows, type, channels, addr, stride_x, stride_y, stride_c, row0, rows, depth_kind, velocity_kind, out) ? RFX_EINVAL
                                                                                                                                                                : RFX_OK;
}
int rfx_internal_exr_piz_tables(int piz_blocks, struct rfx_exr_piz_tables *out) { return out && rfx_exr_piz_tables_for(piz_blocks, out) ? 0 : -1; }
int rfx_internal_k3_tile(int W, int H, float radius, int inputIsTemporal, int textureCount, struct rfx_k3_tile_plan *out) {
    *out = rfx_k3_tile((float)W, (float)H, radius, inputIsTemporal != 0, textureCount);
    return RFX_OK;
}

int rfx_internal_hit_mask_enqueue(rfx_ctx *c, int ranks) {
    if (!c->hits || !c->hits_traced) return fail(c, RFX_ESTATE, "rfx_gather_history_rows / rfx_ssgi_hit_mask: no rfx_ssgi_trace of this frame is waiting for its shade");
    RFX_ENTER(c);
    int rc = hit_mask_scratch(c, ranks);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->hit_mask_dev, 0, (size_t)c->H * sizeof(unsigned int), c->stream));
    if (c->trace_y1 > c->trace_y0 && c->trace_scaled)  // trace_y0 / trace_y1 are TARGET rows then
        HIPCHK(c, rfx_launch_k1_hit_mask_scaled(dims(c), rfx_uv_planes(c->uv_model, c->trace_out_w, c->trace_out_h), c->trace_out_w, c->trace_y0, c->trace_y1,
                                                view(c, RFX_TEX_DEPTH), c->hits, c->trace_missed != 0, c->hit_mask_dev, c->stream));
    else if (c->trace_y1 > c->trace_y0)
        HIPCHK(c, rfx_launch_k1_hit_mask(dims(c), c->trace_y0, c->trace_y1, view(c, RFX_TEX_DEPTH), wview(c, RFX_TEX_SSGI), c->hits, c->trace_missed != 0, c->hit_mask_dev, c->stream));
    return RFX_OK;
}

int rfx_ssgi_hit_mask(rfx_ctx *c, unsigned int *row_mask, int rows) {
    if (!c || !row_mask) return RFX_EINVAL;
    if (rows != c->H) return fail(c, RFX_EINVAL, "rfx_ssgi_hit_mask: one word per frame row (rows == height)");
    int rc = rfx_internal_hit_mask_enqueue(c, 1);
    if (rc) return rc;
    return hit_mask_read_back(c, row_mask);
}

// the first and the last row of that mask with a bit set (a diagnostic: the gathers plan with the mask itself)
int rfx_ssgi_hit_rows(rfx_ctx *c, int *row_lo, int *row_hi) {
    if (!c || !row_lo || !row_hi) return RFX_EINVAL;
    int rc = rfx_internal_hit_mask_enqueue(c, 1);
    if (rc || (rc = hit_mask_read_back(c, nullptr))) return rc;
    int lo = 0x7fffffff, hi = -1;
    for (int y = 0; y < c->H; y++)
        if (c->hit_mask_host[y]) {
            if (hi < 0) lo = y;
            hi = y;
        }
    *row_lo = lo;
    *row_hi = hi;
    return RFX_OK;
}

int rfx_ssgi_target_rows(rfx_ctx *c, float resolutionScale, int *row0, int *rows) {
    if (!c) return RFX_EINVAL;
    const float rs = resolutionScale == 0.0f ? 1.0f : resolutionScale;
    rfx_scaled_rows_plan t = {c->slots[RFX_TEX_SSGI].row0, c->slots[RFX_TEX_SSGI].row0 + c->slots[RFX_TEX_SSGI].rows};  // scale 1: the held band
    if (rs != 1.0f) {
        int Ws, Hs;
        if (!scaled_target(c, rs, &Ws, &Hs)) return fail(c, RFX_EINVAL, "rfx_ssgi_target_rows: resolutionScale must be in (0, 1] with whole W*s and H*s");
        t = ctx_scaled_rows(c, Hs);
    }
    if (row0) *row0 = t.j0;
    if (rows) *rows = t.j1 - t.j0;
    return RFX_OK;
}

int rfx_ssgi_march(rfx_ctx *c, const rfx_ssgi_params *p) { return ssgi_draw(c, p, 0); }
int rfx_ssgi_trace(rfx_ctx *c, const rfx_ssgi_params *p) { return ssgi_draw(c, p, 1); }
int rfx_ssgi_shade(rfx_ctx *c, const rfx_ssgi_params *p) { return ssgi_draw(c, p, 2); }

int rfx_temporal_reproject(rfx_ctx *c, const rfx_temporal_params *p) {
    if (!c || !p) return RFX_EINVAL;
    if (!((p->inputType == 0 && p->textureCount == 2) || ((p->inputType == 1 || p->inputType == 2) && p->textureCount == 1)))
        return fail(c, RFX_EINVAL, "rfx_temporal_reproject: inputType/textureCount combination");
    if (p->historySource < 0 || p->historySource > 2) return fail(c, RFX_EINVAL, "rfx_temporal_reproject: historySource");
    RFX_ENTER(c);
    const int h0 = p->historySource == 0 ? RFX_TEX_DENOISE_B0 : (p->historySource == 1 ? RFX_TEX_FBCOPY_F16 : RFX_TEX_FBCOPY_F32);
    // with one texture the reference binds the same history to every index (TemporalReprojectPass.js:148-151)
    const int h1 = (p->historySource == 0 && p->textureCount == 2) ? RFX_TEX_DENOISE_B1 : h0;
    const int o1 = p->textureCount == 2 ? RFX_TEX_TEMPORAL1 : RFX_TEX_TEMPORAL0;
    const int ids[] = {RFX_TEX_SSGI, RFX_TEX_VELOCITY, h0, h1, RFX_TEX_TEMPORAL0, o1};
    int rc = need(c, ids, 6);
    if (rc) return rc;
    if (!c->slots[RFX_TEX_VELOCITY].uploaded) return fail(c, RFX_ESTATE, "rfx_temporal_reproject: velocity not uploaded");
    K2Args A;
    A.dims = dims(c);
    if (!launch_rows(c, RFX_TEX_TEMPORAL0, 0, &A.y0, &A.y1)) return RFX_OK;
    A.ssgi = view(c, RFX_TEX_SSGI); A.velocity = view(c, RFX_TEX_VELOCITY);
    A.hist0 = view(c, h0);
    A.hist1 = view(c, h1);
    A.hist_f32 = p->historySource == 2;
    A.in_w = p->inputWidth > 0 ? p->inputWidth : c->W;
    A.in_h = p->inputHeight > 0 ? p->inputHeight : c->H;
    if (A.in_w > c->W || A.in_h > c->H) return fail(c, RFX_EINVAL, "rfx_temporal_reproject: inputWidth/inputHeight larger than the frame");
    {   // a smaller input texture: the target rows K1 left at the start of the slot (every row on a whole-frame context)
        const rfx_scaled_rows_plan t = ctx_scaled_rows(c, A.in_h);
        A.in_j0 = t.j0; A.in_rows = t.j1 - t.j0;
        if ((A.in_w != c->W || A.in_h != c->H) && (A.in_rows < 1 || !scaled_rows_fit(c, A.in_w, t)))
            return fail(c, RFX_EINVAL, "rfx_temporal_reproject: the input texture's rows of this tile do not fit the held band (more halo rows)");
    }
    A.out0 = wview(c, RFX_TEX_TEMPORAL0); A.out1 = wview(c, o1);
    A.p = *p;
    // TemporalReprojectPass.js:135: invTexSize.set(1 / width, 1 / height) in doubles
    A.invW = (float)(1.0 / (double)c->W); A.invH = (float)(1.0 / (double)c->H);
    {   // IEEE fp32 reciprocals of those two uniforms (volatile: no folding into double arithmetic)
        volatile float iw = A.invW, ih = A.invH;
        A.rcpInvW = 1.0f / iw; A.rcpInvH = 1.0f / ih;
    }
    // prevProjectionMatrix * prevViewMatrix (reproject.frag:183), fp32, column by column like GLSL
    const float *Pm = p->prevCamera.projectionMatrix, *Vm = p->prevCamera.matrixWorldInverse;
    for (int col = 0; col < 4; col++)
        for (int row = 0; row < 4; row++) {
            volatile float acc = Pm[0 * 4 + row] * Vm[col * 4 + 0];
            volatile float t1 = Pm[1 * 4 + row] * Vm[col * 4 + 1]; acc = acc + t1;
            volatile float t2 = Pm[2 * 4 + row] * Vm[col * 4 + 2]; acc = acc + t2;
            volatile float t3 = Pm[3 * 4 + row] * Vm[col * 4 + 3]; acc = acc + t3;
            A.prevPV[col * 4 + row] = acc;
        }
    ProfScope prof(c, RFX_PROF_K2, c->stream);
    HIPCHK(c, rfx_launch_k2(A, c->stream));
    return RFX_OK;
}

int rfx_copy_framebuffer(rfx_ctx *c, rfx_tex dst) {
    if (!c) return RFX_EINVAL;
    if (dst != RFX_TEX_FBCOPY_F16 && dst != RFX_TEX_FBCOPY_F32) return fail(c, RFX_EINVAL, "rfx_copy_framebuffer: dst must be RFX_TEX_FBCOPY_F16 or _F32");
    RFX_ENTER(c);
    const int ids[] = {RFX_TEX_TEMPORAL0, (int)dst};
    int rc = need(c, ids, 2);
    if (rc) return rc;
    int y0, y1;
    if (!launch_rows(c, dst, 0, &y0, &y1)) return RFX_OK;
    HIPCHK(c, rfx_launch_copy_fb(dims(c), y0, y1, view(c, RFX_TEX_TEMPORAL0), wview(c, dst), dst == RFX_TEX_FBCOPY_F16, c->stream));
    return RFX_OK;
}

int rfx_poisson_denoise(rfx_ctx *c, const rfx_denoise_params *p) {
    if (!c || !p) return RFX_EINVAL;
    if (p->textureCount != 1 && p->textureCount != 2) return fail(c, RFX_EINVAL, "rfx_poisson_denoise: textureCount");
    RFX_ENTER(c);
    const int in0 = p->inputIsTemporal ? RFX_TEX_TEMPORAL0 : (p->writeToB ? RFX_TEX_DENOISE_A0 : RFX_TEX_DENOISE_B0);
    const int in1 = p->inputIsTemporal ? RFX_TEX_TEMPORAL1 : (p->writeToB ? RFX_TEX_DENOISE_A1 : RFX_TEX_DENOISE_B1);
    const int out0 = p->writeToB ? RFX_TEX_DENOISE_B0 : RFX_TEX_DENOISE_A0;
    const int out1 = p->writeToB ? RFX_TEX_DENOISE_B1 : RFX_TEX_DENOISE_A1;
    const int ids[] = {RFX_TEX_DEPTH, RFX_TEX_GBUFFER, RFX_TEX_BLUE_NOISE, in0, in1, out0, out1};
    int rc = need(c, ids, 7);
    if (rc) return rc;
    if (!c->slots[RFX_TEX_DEPTH].uploaded || !c->slots[RFX_TEX_GBUFFER].uploaded || !c->slots[RFX_TEX_BLUE_NOISE].uploaded)
        return fail(c, RFX_ESTATE, "rfx_poisson_denoise: depth / gbuffer / blue-noise not uploaded");
    K3Args A;
    A.dims = dims(c);
    if (!launch_rows(c, out0, 0, &A.y0, &A.y1)) return RFX_OK;
    A.depth = view(c, RFX_TEX_DEPTH); A.gbuffer = view(c, RFX_TEX_GBUFFER);
    A.in0 = view(c, in0);
    A.in1 = view(c, p->textureCount == 2 ? in1 : in0);  // `#define inputTexture2 inputTexture` (poisson_denoise.frag:30-32)
    A.blue = c->slots[RFX_TEX_BLUE_NOISE].ptr;
    blue_noise_shift(p->blueNoiseIndex, &A.shift_x, &A.shift_y);
    A.out0 = wview(c, out0); A.out1 = wview(c, out1);
    A.p = *p;
    // the foreground map of the last K1 pre-pass, while it still describes the depth plane these draws read: no writer of the slot since
    // (depth_gen), not a caller's buffer (written by work this library cannot see), and tile rows that are the map's (launch rows from a
    // multiple of 8: a row window or a row tile may start anywhere).  rfx_launch_k3 drops it unless every view is the whole frame.
    A.fg_tiles = (c->fg_tiles && c->fg_gen == c->depth_gen && !c->depth_external && (A.y0 & 7) == 0) ? c->fg_tiles + (size_t)c->fg_cur * c->fg_stride : nullptr;
    ProfScope prof(c, p->inputIsTemporal ? RFX_PROF_K3_PASS0 : RFX_PROF_K3_PASSN, c->stream);
    HIPCHK(c, rfx_launch_k3(A, c->stream));
    return RFX_OK;
}

int rfx_compose(rfx_ctx *c, const rfx_compose_params *p) {
    if (!c || !p) return RFX_EINVAL;
    if (p->inputType != 0 && p->inputType != 2)
        return fail(c, RFX_EUNSUPPORTED, "rfx_compose: inputType diffuseSpecular (0) and specular (2) are built");
    RFX_ENTER(c);
    if (p->giSource != 0 && p->giSource != 1) return fail(c, RFX_EINVAL, "rfx_compose: giSource");
    const int g0 = p->giSource ? RFX_TEX_TEMPORAL0 : RFX_TEX_DENOISE_B0, g1 = p->giSource ? RFX_TEX_TEMPORAL1 : RFX_TEX_DENOISE_B1;
    const int ids[] = {RFX_TEX_DEPTH, RFX_TEX_GBUFFER, g0, g1, RFX_TEX_COMPOSE, RFX_TEX_DIRECT_LIGHT};
    int rc = need(c, ids, 6);
    if (rc) return rc;
    K4Args A;
    A.dims = dims(c);
    launch_rows(c, RFX_TEX_COMPOSE, 0, &A.y0, &A.y1);
    if (A.y0 < c->tile_y0) A.y0 = c->tile_y0;  // COMPOSE is held whole: write only the tile
    if (A.y1 > c->tile_y0 + c->tile_rows) A.y1 = c->tile_y0 + c->tile_rows;
    const bool any = A.y1 > A.y0;
    A.depth = view(c, RFX_TEX_DEPTH); A.gbuffer = view(c, RFX_TEX_GBUFFER);
    A.gi0 = view(c, g0); A.gi1 = view(c, g1);
    A.scene = view(c, RFX_TEX_DIRECT_LIGHT);  // Denoiser.js:101-103: sceneTexture = the composer's input buffer
    A.out = wview(c, RFX_TEX_COMPOSE);
    A.rgb_out = nullptr;
    if (p->writeHistoryRGB) {
        const int rgb[] = {RFX_TEX_COMPOSE_RGB};
        if ((rc = need(c, rgb, 1))) return rc;
        A.rgb_out = (float *)c->slots[RFX_TEX_COMPOSE_RGB].ptr;  // held whole, like COMPOSE: frame row y at y * W
    }
    A.p = *p;
    if (c->peer_release_pending) {  // rfx_peer_gather_history: this draw overwrites rows a peer's kernel may still be pulling
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_peer_release, 0));
        c->peer_release_pending = false;
    }
    if (any) {
        ProfScope prof(c, RFX_PROF_K4, c->stream);
        HIPCHK(c, rfx_launch_k4(A, c->stream));
    }
    return RFX_OK;
}

int rfx_final_compose(rfx_ctx *c, const rfx_final_params *p) {
    if (!c || !p) return RFX_EINVAL;
    if (p->fogMode < 0 || p->fogMode > 2) return fail(c, RFX_EINVAL, "rfx_final_compose: fogMode");
    RFX_ENTER(c);
    if (p->inputSource < 0 || p->inputSource > 2) return fail(c, RFX_EINVAL, "rfx_final_compose: inputSource");
    const int src = p->inputSource == 0 ? RFX_TEX_COMPOSE : (p->inputSource == 1 ? RFX_TEX_TEMPORAL0 : RFX_TEX_DENOISE_B0);
    const int ids[] = {RFX_TEX_DEPTH, src, RFX_TEX_DIRECT_LIGHT, RFX_TEX_FINAL};
    int rc = need(c, ids, 4);
    if (rc) return rc;
    K5Args A;
    A.dims = dims(c);
    if (!launch_rows(c, RFX_TEX_FINAL, 0, &A.y0, &A.y1)) return RFX_OK;
    A.depth = view(c, RFX_TEX_DEPTH); A.gi = view(c, src); A.scene = view(c, RFX_TEX_DIRECT_LIGHT);
    A.out = wview(c, RFX_TEX_FINAL);
    A.p = *p;
    ProfScope prof(c, RFX_PROF_K5, c->stream);
    HIPCHK(c, rfx_launch_k5(A, c->stream));
    return RFX_OK;
}

}  // extern "C"
