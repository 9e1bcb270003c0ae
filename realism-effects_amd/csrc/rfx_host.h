// rfx_host.h — what the host files of the C ABI share (rfx_api, rfx_stage, rfx_exr_import, rfx_env, rfx_draw, rfx_blur, rfx_export): the context,
// the kernels' argument blocks and launch plans, and the helpers more than one of them uses, as static inline functions.  The few shared functions
// that are defined once (rfx_stage.hip) are declared at the end, hidden: the library exports nothing new.  Private to librfx_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/rfx.h"
#include "rfx_kernels.h"
#include "rfx_launch.h"

#include "rfx_ctx.h"

// every entry point that takes a context: select its device
#define RFX_ENTER(c) hipSetDevice((c)->device)
// rfx_profile: bracket the launches of one draw with two events on `stream` (no-ops unless profiling is on)
static inline hipEvent_t prof_event(rfx_ctx *c) {
    hipEvent_t e = nullptr;
    if (!c->prof_free.empty()) { e = c->prof_free.back(); c->prof_free.pop_back(); return e; }
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}
static inline void prof_recycle(rfx_ctx *c) {
    for (const rfx_ctx::ProfRec &r : c->prof_recs) { c->prof_free.push_back(r.a); c->prof_free.push_back(r.b); }
    c->prof_recs.clear();
}
struct ProfScope {
    rfx_ctx *c;
    hipStream_t stream;
    hipEvent_t a = nullptr, b = nullptr;
    int kind;
    ProfScope(rfx_ctx *c_, int kind_, hipStream_t s) : c(c_), stream(s), kind(kind_) {
        if (!c->profiling || c->prof_recs.size() >= 8192) return;
        a = prof_event(c); b = prof_event(c);
        if (!a || !b || hipEventRecord(a, stream) != hipSuccess) drop();  // (a capturing user stream refuses the record: the draw is simply not timed)
    }
    void drop() { if (a) c->prof_free.push_back(a); if (b) c->prof_free.push_back(b); a = b = nullptr; }
    ~ProfScope() {
        if (!a) return;
        if (hipEventRecord(b, stream) != hipSuccess) { drop(); return; }  // never a half-recorded pair in prof_recs
        c->prof_recs.push_back({kind, a, b});
    }
};

// The depth slot has a new writer.  Every entry point that can write the slot calls this: the foreground map of the last K1 pre-pass no
// longer describes the plane (depth_gen, rfx_ctx.h), and the next pre-pass must know what to wait for.
enum DepthWriter {
    DEPTH_WRITTEN,   // the write is complete: nothing for the pre-pass to wait for
    DEPTH_PENDING,   // the caller has just recorded ev_depth behind the write: the pre-pass waits for it on its own stream
    DEPTH_EXTERNAL,  // written by work this library cannot see, ordered against the draw stream only: the pre-pass stays in the draw stream
};
static inline void depth_new_writer(rfx_ctx *c, DepthWriter w) {
    if (w == DEPTH_EXTERNAL) c->depth_external = true;
    else c->depth_event_set = w == DEPTH_PENDING;
    c->depth_gen++;
}

static inline int ensure(rfx_ctx *c, int id) {
    Slot &s = c->slots[id];
    if (s.ptr) return RFX_OK;
    const size_t bytes = (size_t)s.rows * s.width * s.texel;
    hipError_t e = hipMalloc(&s.ptr, bytes);
    if (e != hipSuccess) return fail(c, RFX_ENOMEM, "hipMalloc(texture)", e);
    s.owned = true;
    // render targets start zeroed: `discard`ed fragments expose the initial contents (Appendix D-10)
    e = hipMemsetAsync(s.ptr, 0, bytes, c->stream);
    if (e != hipSuccess) return fail(c, RFX_EDEVICE, "hipMemsetAsync", e);
    return RFX_OK;
}

static inline int band_check(rfx_ctx *c, int id, int row0, int rows) {
    if (id < 0 || id >= RFX_TEX_COUNT) return fail(c, RFX_EINVAL, "bad texture id");
    const Slot &s = c->slots[id];
    if (rows <= 0 || row0 < s.row0 || row0 + rows > s.row0 + s.rows) return fail(c, RFX_EINVAL, "row band outside the rows this context holds");
    return RFX_OK;
}
// where frame row `frame_row` (a row of the held band) starts in a slot's buffer, and in its back buffer
static inline size_t slot_row_offset(const Slot &s, int frame_row) { return (size_t)(frame_row - s.row0) * s.width * s.texel; }
static inline char *slot_row(const Slot &s, int frame_row) { return (char *)s.ptr + slot_row_offset(s, frame_row); }
static inline char *slot_back_row(const Slot &s, int frame_row) { return (char *)s.back + slot_row_offset(s, frame_row); }
// An input slot holds something: a host-filled plane must have been uploaded (packed, staged or bound), as K2 / K3 require of theirs; a slot a
// draw writes must at least exist — a draw, an upload or a clear made it
static inline bool slot_filled(const rfx_ctx *c, int id) {
    const bool host_filled = id == RFX_TEX_VELOCITY || id == RFX_TEX_BLUE_NOISE || id == RFX_TEX_DIRECT_LIGHT || id == RFX_TEX_EFFECT_INPUT;
    return host_filled ? c->slots[id].uploaded : c->slots[id].ptr != nullptr;
}
// "fn: what" into the context's error text
static inline int fail_in(rfx_ctx *c, int code, const char *fn, const char *what) {
    char buf[384];
    snprintf(buf, sizeof buf, "%s: %s", fn, what);
    return fail(c, code, buf);
}

// a device buffer of at least `want` bytes in *buf (capacity *cap), replaced when it is too small: the caller knows it idle
static inline int grow_idle(rfx_ctx *c, void **buf, size_t *cap, size_t want, const char *what) {
    if (*cap >= want) return RFX_OK;
    if (*buf) hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(buf, want);
    if (e != hipSuccess) return fail(c, RFX_ENOMEM, what, e);
    *cap = want;
    return RFX_OK;
}

static inline TexView view(rfx_ctx *c, int id) { return {c->slots[id].ptr, c->slots[id].row0, c->slots[id].rows}; }
static inline TexViewW wview(rfx_ctx *c, int id) { return {c->slots[id].ptr, c->slots[id].row0, c->slots[id].rows}; }
// The plane equations of a w x h render target's vUv (rfx_device.h UvPlanes; the host files are compiled with -ffp-contract=off: every product
// below is rounded on its own, as the reference GL's triangle setup rounds them)
static inline UvPlanes rfx_uv_planes(int model, int w, int h) {
    UvPlanes q;
    q.model = model; q.W = w; q.H = h; q.fW = (float)w; q.fH = (float)h;
    const float ooa = 1.0f / ((float)w * (float)h);
    q.du = (float)h * ooa;
    q.dv = (float)w * ooa;
    const float far_u = q.du * ((float)w - 0.5f), far_v = q.dv * ((float)h - 0.5f);
    q.u0_upper = 0.5f * q.du;
    q.u0_lower = 1.0f - far_u;
    q.v0 = 1.0f - far_v;
    return q;
}
static inline FrameDims dims(rfx_ctx *c) {
    FrameDims d;
    d.W = c->W; d.H = c->H; d.fW = (float)c->W; d.fH = (float)c->H;
    d.uv = rfx_uv_planes(c->uv_model, c->W, c->H);
    d.halo_violations = c->halo_violations;
    return d;
}

// blue_noise.glsl:9-34: one pcg4d round of the per-draw seed; the toroidal shift is pixel-independent
static inline void blue_noise_shift(int index, int *sx, int *sy) {
    if (index == 0) { *sx = 0; *sy = 0; return; }  // :38-39 texture-coordinate path == unshifted table
    uint32_t i = (uint32_t)index;
    uint32_t v[4] = {i, i * 15843u, i * 31u + 4566u, i * 2345u + 58585u};
    for (int k = 0; k < 4; k++) v[k] = v[k] * 1664525u + 1013904223u;
    v[0] += v[1] * v[3]; v[1] += v[2] * v[0]; v[2] += v[0] * v[1]; v[3] += v[1] * v[2];
    for (int k = 0; k < 4; k++) v[k] ^= v[k] >> 16;
    v[0] += v[1] * v[3]; v[1] += v[2] * v[0]; v[2] += v[0] * v[1]; v[3] += v[1] * v[2];
    *sx = (int)((v[0] % 0x0fffffffu) % 128u);
    *sy = (int)((v[1] % 0x0fffffffu) % 128u);
}

// Rows a launch produces: the tile, widened by `extra` rows on each side (clipped to what the
// output slot holds).
static inline bool launch_rows(rfx_ctx *c, int out_id, int extra, int *y0, int *y1) {
    const Slot &s = c->slots[out_id];
    int a = c->tile_y0 - extra, b = c->tile_y0 + c->tile_rows + extra;
    if (a < s.row0) a = s.row0;
    if (b > s.row0 + s.rows) b = s.row0 + s.rows;
    if (a < c->win_y0) a = c->win_y0;  // rfx_set_row_window
    if (b > c->win_y1) b = c->win_y1;
    *y0 = a; *y1 = b;
    return b > a;  // false: nothing to draw
}

// the row-mask scratch of the bounded gathers (rfx_ctx.h hit_mask_dev / hit_mask_host), sized for `ranks` gathered copies
static inline int hit_mask_scratch(rfx_ctx *c, int ranks) {
    if (ranks < 1) ranks = 1;
    if (!c->hit_mask_dev || c->hit_mask_ranks < ranks) {
        if (c->hit_mask_dev) {
            // the packing kernels and the offset copy of an earlier rfx_gather_history_rows run on comm_stream and read these buffers (the row
            // offsets live in the same allocation): both streams drain before they go
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (c->comm_stream) HIPCHK(c, hipStreamSynchronize(c->comm_stream));
            hipFree(c->hit_mask_dev); hipHostFree(c->hit_mask_host); c->hit_mask_dev = nullptr; c->hit_mask_host = nullptr;
        }
        const size_t words = (size_t)(2 * ranks + 2) * c->H;  // [0, H) this tile's mask, [H, (n + 1) H) every rank's, then (n + 1) H row offsets
        hipError_t e = hipMalloc((void **)&c->hit_mask_dev, words * sizeof(unsigned int));
        if (e == hipSuccess) e = hipHostMalloc((void **)&c->hit_mask_host, words * sizeof(unsigned int), hipHostMallocDefault);
        if (e != hipSuccess) return fail(c, RFX_ENOMEM, "rfx_ssgi_hit_mask: scratch", e);
        c->hit_mask_ranks = ranks;
    }
    return RFX_OK;
}
// the first H words of hit_mask_dev (the mask an enqueue left on the draw stream) -> hit_mask_host, and into row_mask when given
static inline int hit_mask_read_back(rfx_ctx *c, unsigned int *row_mask) {
    const size_t bytes = (size_t)c->H * sizeof(unsigned int);
    HIPCHK(c, hipMemcpyAsync(c->hit_mask_host, c->hit_mask_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (row_mask) memcpy(row_mask, c->hit_mask_host, bytes);
    return RFX_OK;
}

// ---- rfx_stage.hip, for rfx_exr_import.hip too (hidden: not exported by the library)
#define RFX_HIDDEN __attribute__((visibility("hidden")))
// What rfx_stage_aov and the rfx_stage_exr_* calls do first and last with their plan.  First, every check before anything is enqueued: the slots the
// plan writes exist and are the context's own (`fn`: the entry point, for the error text), the upload stream and their back buffers exist.
// Last: those back buffers are marked for rfx_stage_flip.
RFX_HIDDEN int stage_plan_begin(rfx_ctx *c, const rfx_aov_plan &t, const char *fn);
RFX_HIDDEN void stage_plan_end(rfx_ctx *c, const rfx_aov_plan &t);
// a device area of the context grows: the one wait of the staged paths (an earlier call's kernels may still be using the area that goes)
RFX_HIDDEN int grow_stage_area(rfx_ctx *c, void **area, size_t *cap, size_t need, const char *what);
// one segment's pack launch on the upload stream: A holds the segment's staged planes, their half mask and the rgb(a) channel counts
RFX_HIDDEN hipError_t aov_pack_segment(rfx_ctx *c, const rfx_aov_plan &t, const rfx_aov_segment &g, K0AovArgs A);
// the kinds the next staging call plans with (include/rfx.h "AOV conventions"; the default where nothing is set)
RFX_HIDDEN int aov_depth_kind(const rfx_ctx *c);
RFX_HIDDEN int aov_velocity_kind(const rfx_ctx *c);
