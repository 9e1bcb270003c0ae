// rfx_ctx.h — the context object behind the opaque rfx_ctx handle, shared by the host files of the C ABI (through rfx_host.h: slots, uploads,
// draws, export) and by rfx_comm.hip / rfx_peer.hip (the exchanges of a row-tiled run).  Private to librfx_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/rfx.h"

struct Slot {
    void *ptr = nullptr;
    bool owned = false;
    int row0 = 0, rows = 0;  // held band (frame rows)
    size_t texel = 0;
    int width = 0;
    bool uploaded = false;
    // streaming dumps (rfx_stage_upload / rfx_stage_flip): the BACK buffer the next frame's plane is copied into while the draws read `ptr`
    void *back = nullptr;
    bool back_filled = false;
};

struct rfx_ctx {
    int device = 0;
    int W = 0, H = 0, tile_y0 = 0, tile_rows = 0, halo = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    unsigned int *halo_violations = nullptr;
    float *viewz = nullptr;    // K1 scratch: view-space Z plane (full frame)
    float4 *hits = nullptr;    // K1 trace -> shade hand-over (rfx_ssgi_trace), 2 texels per SSGI texel
    bool hits_traced = false;  // a trace is waiting for its shade
    int trace_y0 = 0, trace_y1 = 0, trace_missed = 0;  // the rows and the missedRays option of that trace (rfx_gather_history_rows)
    bool trace_scaled = false;                         // ... and whether it drew a smaller target (resolutionScale != 1):
    int trace_out_w = 0, trace_out_h = 0;              //     its size; trace_y0 / trace_y1 are then TARGET rows (rfx_launch.h rfx_scaled_rows)
    // the bounded gather's row masks (rfx_gather_history_rows, rfx_ssgi_hit_mask): one word per frame row; device: [0, H) this tile's, [H, (n+1) H) every rank's
    unsigned int *hit_mask_dev = nullptr, *hit_mask_host = nullptr;
    int hit_mask_ranks = 0;  // ranks the two buffers are sized for (each holds (2 n + 2) H words: the masks, then the packed transfer's row offsets)
    void *hist_staging = nullptr;      // the bounded gather's packed messages: what this rank sends, then what it receives
    size_t hist_staging_bytes = 0;
    // K1's depth pre-pass (view-Z plane + (min, max) cells) depends on the frame's depth plane only: it runs on its own stream, after
    // the PREVIOUS frame's K1 (the last reader of the scratch it overwrites) and under that frame's K2 / K3 / K4, which are still queued
    // or executing when the host issues the next frame.  ev_depth: the depth slot's last asynchronous writer (rfx_stage_flip / rfx_clear).
    hipStream_t prep_stream = nullptr;
    hipEvent_t ev_depth = nullptr, ev_k1_done = nullptr, ev_prep_done = nullptr;
    bool depth_event_set = false, k1_event_set = false, depth_external = false;
    int win_y0 = 0, win_y1 = 0x7fffffff;  // rfx_set_row_window: rows the draws may produce
    int blur_armed = -1;  // row-tiled rfx_motion_blur: the source slot RFX_TEX_BLUR_SOURCE was last staged for (rfx_motion_blur_stage / _gather), -1 = none
    int uv_model = RFX_UV_REFERENCE_GL;    // rfx_set_uv_model (the default: the vUv the parity oracle's GL interpolates)
    float2 *coarse = nullptr;  // K1 scratch: exact (min,max) view Z per 16x16 base cell
    unsigned int *cells = nullptr;  // K1 scratch: the march's half-packed (min,max) table
    unsigned int *k1_tiles = nullptr;  // K1 scratch: the persistent march kernel's tile counter
    int n_cu = 0;                      // compute units of the device
    // K3's foreground map: one byte per frame-aligned 64 x 8-texel tile, 0 = every depth texel of the tile is 1.0 (all of its
    // pixels discard), written by K1's depth pre-pass.  TWO maps in one allocation, fg_stride bytes apart: the pre-pass of frame n + 1 runs
    // under frame n's K3 draws, so it fills the map the previous pre-pass did not (fg_cur: the one the last pre-pass filled).
    unsigned char *fg_tiles = nullptr;
    size_t fg_stride = 0;
    int fg_w = 0, fg_cur = 0;
    // ... and its validity: every entry point that can write the DEPTH slot bumps depth_gen; the pre-pass records the value it read (fg_gen)
    unsigned long long depth_gen = 1, fg_gen = 0;
    float4 *env = nullptr;     // scene.environment: the whole mip chain, float4 texels
    float *env_marginal = nullptr, *env_conditional = nullptr;  // EquirectHdrInfo inverse-CDF tables (importanceSampling)
    float env_sum_whole = 1.0f, env_sum_decimal = 0.0f;
    int env_w = 0, env_h = 0, env_levels = 0;
    unsigned int env_off[16] = {0};
    // The context owns the chain and the tables with their capacities in bytes (env_cap; env_tab_cap: marginal, conditional), so that the
    // stream-ordered updates (rfx_set_environment_cube, rfx_build_environment_importance) re-use them when the sizes repeat; the blocking entry
    // points free and allocate exactly, as they always did.  env_tables_set: the tables describe the held environment (importanceSampling is
    // refused otherwise); env_sums_on_device: K10 built them, K1 reads the two sums from env_k10 and not from env_sum_whole / env_sum_decimal.
    size_t env_cap = 0, env_tab_cap[2] = {0, 0};
    bool env_tables_set = false, env_sums_on_device = false;
    // ... and the areas of the device path, grown on demand like aov_stage: the equirect staging the cube pass draws into and the mip kernel reads,
    // the cube's own chain, K10's scratch (rfx_kernels.h rfx_env_tables_scratch_bytes); the event behind the copy of the caller's faces
    void *env_stage = nullptr, *env_cube = nullptr, *env_k10 = nullptr;
    size_t env_stage_cap = 0, env_cube_cap = 0, env_k10_cap = 0;
    hipEvent_t ev_env_copied = nullptr;
    Slot slots[RFX_TEX_COUNT];
    // row-tiled runs (rfx_comm.hip): the RCCL communicator of the tile ring, a second stream the exchanges run on, and the two
    // events that order it against the draw stream
    void *comm = nullptr;            // ncclComm_t
    bool comm_owned = false;
    int comm_rank = 0, comm_nranks = 1;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_draws = nullptr, ev_comm = nullptr;
    bool comm_pending = false;       // exchanges issued since the last rfx_comm_wait
    // streaming dumps: a third stream for the host-to-device copies of the NEXT frame and the two events that order it against the draws
    hipStream_t upload_stream = nullptr;
    hipEvent_t ev_staged = nullptr, ev_frame_done = nullptr;
    hipEvent_t ev_batch[2] = {nullptr, nullptr};  // the copies published by the last two flips (recorded on upload_stream)
    unsigned int flips = 0;
    // rfx_queue_wait_stream / rfx_stream_wait_queue (include/rfx.h "device images and stream ordering"): [0] is recorded on the caller's stream
    // and waited for by a queue of the context, [1] the other way round; created at the first use of either call
    hipEvent_t ev_order[2] = {nullptr, nullptr};
    // rfx_stage_aov: the staging area the planes of an AOV frame are copied into on the upload stream and its pack kernel reads (rfx_launch.h
    // rfx_aov_plan).  One is enough: the stream is in order, the next call's copies queue behind this call's kernel.  Grown on demand; neither a
    // texture slot nor checkpoint state
    void *aov_stage = nullptr;
    size_t aov_stage_cap = 0;
    // rfx_set_aov_conventions (include/rfx.h "AOV conventions"): what the next staging call reads; aov_conv_on false: the default, whatever
    // aov_conv holds.  Context state, not checkpoint state
    bool aov_conv_on = false;
    rfx_aov_conventions aov_conv = {};
    // rfx_stage_exr_aov: the device area of a call's tables, packed chunks and inflate scratch (the same owner and growth rule); two pinned host
    // blocks the tables are written into before they are copied (batch n uses block n & 1: rfx_stage_flip's back pressure says the copies of batch
    // n - 2 have executed; calls of one batch append); the pinned status words and the event behind their copy
    void *exr_stage = nullptr;
    size_t exr_stage_cap = 0;
    void *exr_tables_host[2] = {nullptr, nullptr};
    size_t exr_tables_cap[2] = {0, 0}, exr_tables_used[2] = {0, 0};
    unsigned int exr_tables_batch[2] = {0, 0};
    int *exr_status_host = nullptr;
    hipEvent_t ev_exr_status = nullptr;
    bool exr_staged = false;
    // streamed export (rfx_stage_export): a fourth stream for the device-to-host copies, two device staging buffers the encodes alternate
    // between (export n uses buffer n & 1), and per buffer the event behind its last encode (draw stream) and its last copy (download stream)
    hipStream_t download_stream = nullptr;
    void *export_buf[2] = {nullptr, nullptr};
    size_t export_cap[2] = {0, 0};
    hipEvent_t ev_export_encoded[2] = {nullptr, nullptr}, ev_export_copied[2] = {nullptr, nullptr};
    unsigned int exports = 0;  // tickets issued so far (ticket t = export t - 1)
    // rfx_stage_png / rfx_stage_exr: K8's device buffers (result + scratch, rfx_launch.h rfx_png_plan / rfx_exr_plan), one per staging buffer;
    // same owner, same growth rule
    void *png_buf[2] = {nullptr, nullptr};
    size_t png_cap[2] = {0, 0};
    // the peer-load history gather (rfx_peer.hip): this rank's flag block (fine-grained), the device table of every rank's plane and flag block
    // ([0, n) planes, [n, 2 n) flag blocks), what the last call's kernels reported ([0] status bits, [1] texels pulled), the mappings to close
    unsigned long long *peer_flags = nullptr;
    void **peer_table_dev = nullptr;
    unsigned long long *peer_status_dev = nullptr, *peer_status_host = nullptr;
    std::vector<void *> peer_mapped;
    hipEvent_t ev_peer_release = nullptr;  // recorded after the "every rank has pulled" barrier: the next compose draw waits for it
    bool peer_release_pending = false;
    int peer_n = 0, peer_rank = 0, peer_tex = -1;
    unsigned long long peer_epoch = 0;
    // rfx_profile: event pairs around the launches of every draw since the last reset (kind, start, stop), and the events free for re-use
    struct ProfRec { int kind; hipEvent_t a, b; };
    bool profiling = false;
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_free;
    std::string err;
};
void rfx_comm_release(rfx_ctx *c);  // rfx_comm.hip: called by rfx_destroy
// rfx_comm.hip, for rfx_peer.hip too: create the exchange stream and its two events once; order the exchange stream after every draw enqueued
// so far; record the exchange issued since as pending for rfx_comm_wait
int rfx_ensure_streams(rfx_ctx *c);
int rfx_comm_begin(rfx_ctx *c);
int rfx_comm_end(rfx_ctx *c);
void rfx_peer_release(rfx_ctx *c);  // rfx_peer.hip: called by rfx_destroy (before rfx_comm_release: it drains the exchange stream)
// rfx_draw.hip, for rfx_comm.hip / rfx_peer.hip: enqueue on the draw stream the reduction of the traced rays' row masks into the first H words
// of c->hit_mask_dev (allocated here for `ranks` gathered copies)
extern "C" int rfx_internal_hit_mask_enqueue(rfx_ctx *c, int ranks);  // (internal: not part of include/rfx.h)
// ... and (rfx_blur.hip) of the texels a row-tiled rfx_motion_blur with these (validated) params will load, in the same words
extern "C" int rfx_internal_blur_reach_enqueue(rfx_ctx *c, const rfx_motion_blur_params *p, int ranks);
// ... and (rfx_draw.hip), for the CPU tests: the launch plans of rfx_launch.h as the library computes them (K1's table layout, K3's tile geometry)
extern "C" int rfx_internal_k1_table(int W, int H, struct rfx_k1_table_plan *out);
extern "C" int rfx_internal_scaled_rows(int W, int H, int Hs, int uv_model, int y0, int y1, int apron, int *j0, int *j1);
extern "C" int rfx_internal_export_plan(int pixels, int format, int channels, struct rfx_export_plan *out);
// (addr: the image's `data`; strides in elements — rfx_launch.h rfx_export_device_plan_for)
extern "C" int rfx_internal_export_device_plan(int W, int rows, int format, int channels, unsigned long long addr, long long stride_x, long long stride_y,
                                               long long stride_c, struct rfx_export_device_plan *out);
// (held_row0, held_rows: the rows GBUFFER / VELOCITY / DIRECT_LIGHT hold; type, channels: eight entries in rfx_aov_frame's order, channels 0 = not given)
extern "C" int rfx_internal_aov_plan(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, int row0, int rows, struct rfx_aov_plan *out);
// ... with the kinds of include/rfx.h "AOV conventions" (rfx_launch.h rfx_aov_plan_conv_for)
extern "C" int rfx_internal_aov_plan_conv(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, int row0, int rows, int depth_kind,
                                          int velocity_kind, struct rfx_aov_plan *out);
// (addr, stride_*: eight entries each — rfx_launch.h rfx_aov_device_plan_for)
extern "C" int rfx_internal_aov_device_plan(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, const unsigned long long *addr,
                                            const long long *stride_x, const long long *stride_y, const long long *stride_c, int row0, int rows, int depth_kind,
                                            int velocity_kind, struct rfx_aov_device_plan *out);
extern "C" int rfx_internal_exr_piz_tables(int piz_blocks, struct rfx_exr_piz_tables *out);
extern "C" int rfx_internal_k3_tile(int W, int H, float radius, int inputIsTemporal, int textureCount, struct rfx_k3_tile_plan *out);

extern thread_local std::string g_create_err;

static inline size_t texel_bytes(int id) {
    switch (id) {
    case RFX_TEX_DEPTH: return 4;
    case RFX_TEX_BLUE_NOISE: return 4;
    case RFX_TEX_COMPOSE_RGB: return 12;
    case RFX_TEX_DENOISE_A0: case RFX_TEX_DENOISE_A1: case RFX_TEX_DENOISE_B0: case RFX_TEX_DENOISE_B1: case RFX_TEX_FBCOPY_F16: return 8;
    default: return 16;
    }
}

static inline int fail(rfx_ctx *c, int code, const char *what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess) {
        snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        (void)hipGetLastError();  // reported here: not again by the next launch check of this thread (HIP keeps the last error until it is read)
    } else snprintf(buf, sizeof buf, "%s", what);
    if (c) c->err = buf;
    else g_create_err = buf;
    return code;
}
#define HIPCHK(c, call)                                              \
    do {                                                             \
        hipError_t e__ = (call);                                     \
        if (e__ != hipSuccess) return fail(c, RFX_EDEVICE, #call, e__); \
    } while (0)

