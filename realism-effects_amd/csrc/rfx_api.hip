// rfx_api.hip — the C ABI of librfx_hip.so (include/rfx.h) but for the exchanges of a row-tiled run (rfx_comm.hip, rfx_peer.hip).
// Host side only; the kernels live in the k*.hip files.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "../../include/rfx.h"
#include "rfx_kernels.h"
#include "rfx_launch.h"

#include "rfx_ctx.h"

thread_local std::string g_create_err;

// every entry point that takes a context: select its device
#define RFX_ENTER(c) hipSetDevice((c)->device)
// rfx_profile: bracket the launches of one draw with two events on `stream` (no-ops unless profiling is on)
static hipEvent_t prof_event(rfx_ctx *c) {
    hipEvent_t e = nullptr;
    if (!c->prof_free.empty()) { e = c->prof_free.back(); c->prof_free.pop_back(); return e; }
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}
static void prof_recycle(rfx_ctx *c) {
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

extern "C" {

int rfx_abi_version(void) { return RFX_ABI_VERSION; }

size_t rfx_tex_texel_bytes(rfx_tex id) { return (id >= 0 && id < RFX_TEX_COUNT) ? texel_bytes(id) : 0; }

rfx_ctx *rfx_create(int device, int width, int height, int tile_y0, int tile_rows, int halo_rows) {
    if (width <= 0 || height <= 0 || tile_y0 < 0 || tile_rows <= 0 || tile_y0 + tile_rows > height || halo_rows < 0) {
        fail(nullptr, RFX_EINVAL, "rfx_create: bad geometry");
        return nullptr;
    }
    // kernels address texels with 24-bit multiplies and 32-bit byte offsets: a plane stays < 4 GiB (16K x 16K RGBA32F)
    if (width > 32768 || height > 32768 || (size_t)width * height > ((size_t)1 << 28)) {
        fail(nullptr, RFX_EINVAL, "rfx_create: frames above 32768 in an edge or 2^28 texels are not supported");
        return nullptr;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || device < 0 || device >= ndev) {
        fail(nullptr, RFX_EDEVICE, "rfx_create: no such HIP device", e);
        return nullptr;
    }
    rfx_ctx *c = new rfx_ctx();
    c->device = device;
    c->W = width; c->H = height; c->tile_y0 = tile_y0; c->tile_rows = tile_rows; c->halo = halo_rows;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipMalloc((void **)&c->halo_violations, sizeof(unsigned int)) != hipSuccess) {
        fail(nullptr, RFX_EDEVICE, "rfx_create: stream/event creation failed");
        c->stream = c->own_stream;
        rfx_destroy(c);  // releases whatever was created
        return nullptr;
    }
    hipMemset(c->halo_violations, 0, sizeof(unsigned int));
    c->stream = c->own_stream;
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu <= 0) c->n_cu = 256;
    // K1's depth pre-pass stream and the events that order it, created HERE and not lazily by the first draw: every asynchronous writer of
    // the depth slot (rfx_stage_flip, rfx_clear) records ev_depth from the first frame on, so the first pre-pass already waits for the
    // first staged copy (round 3 created them inside the first rfx_ssgi_*: frame 0's pre-pass raced the copy that filled its input)
    if (hipStreamCreateWithFlags(&c->prep_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_depth, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_k1_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_prep_done, hipEventDisableTiming) != hipSuccess) {
        fail(nullptr, RFX_EDEVICE, "rfx_create: K1 pre-pass stream/event creation failed");
        rfx_destroy(c);
        return nullptr;
    }
    const int b0 = tile_y0 - halo_rows < 0 ? 0 : tile_y0 - halo_rows;
    const int b1 = tile_y0 + tile_rows + halo_rows > height ? height : tile_y0 + tile_rows + halo_rows;
    for (int i = 0; i < RFX_TEX_COUNT; i++) {
        Slot &s = c->slots[i];
        s.texel = texel_bytes(i);
        s.width = width;
        // K1 gathers depth and last frame's composed GI anywhere on screen -> held whole
        // ... and a row-tiled motion blur its source (RFX_TEX_BLUR_SOURCE: allocated, like every slot, on first use)
        const bool whole = (i == RFX_TEX_DEPTH || i == RFX_TEX_COMPOSE || i == RFX_TEX_COMPOSE_RGB || i == RFX_TEX_BLUR_SOURCE);
        s.row0 = whole ? 0 : b0;
        s.rows = whole ? height : b1 - b0;
        if (i == RFX_TEX_BLUE_NOISE) { s.row0 = 0; s.rows = 128; s.width = 128; }
    }
    return c;
}

void rfx_destroy(rfx_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    rfx_peer_release(c);
    rfx_comm_release(c);
    // a staged copy may still be writing a back buffer: drain the upload stream before any buffer goes
    if (c->upload_stream) { hipStreamSynchronize(c->upload_stream); hipStreamDestroy(c->upload_stream); }
    // ... and a staged export may still be copying out of a staging buffer
    if (c->download_stream) { hipStreamSynchronize(c->download_stream); hipStreamDestroy(c->download_stream); }
    for (int b = 0; b < 2; b++) {
        if (c->export_buf[b]) hipFree(c->export_buf[b]);
        if (c->png_buf[b]) hipFree(c->png_buf[b]);
        if (c->ev_export_encoded[b]) hipEventDestroy(c->ev_export_encoded[b]);
        if (c->ev_export_copied[b]) hipEventDestroy(c->ev_export_copied[b]);
    }
    for (int i = 0; i < RFX_TEX_COUNT; i++) {
        if (c->slots[i].owned && c->slots[i].ptr) hipFree(c->slots[i].ptr);
        if (c->slots[i].back) hipFree(c->slots[i].back);
    }
    if (c->aov_stage) hipFree(c->aov_stage);
    if (c->exr_stage) hipFree(c->exr_stage);
    for (void *p : c->exr_tables_host)
        if (p) hipHostFree(p);
    if (c->exr_status_host) hipHostFree(c->exr_status_host);
    if (c->ev_exr_status) hipEventDestroy(c->ev_exr_status);
    for (hipEvent_t e : c->ev_batch)
        if (e) hipEventDestroy(e);
    if (c->ev_staged) hipEventDestroy(c->ev_staged);
    if (c->ev_frame_done) hipEventDestroy(c->ev_frame_done);
    if (c->halo_violations) hipFree(c->halo_violations);
    if (c->viewz) hipFree(c->viewz);
    if (c->prep_stream) { hipStreamSynchronize(c->prep_stream); hipStreamDestroy(c->prep_stream); }
    for (hipEvent_t e : {c->ev_depth, c->ev_k1_done, c->ev_prep_done})
        if (e) hipEventDestroy(e);
    if (c->hits) hipFree(c->hits);
    if (c->hit_mask_dev) hipFree(c->hit_mask_dev);
    if (c->hit_mask_host) hipHostFree(c->hit_mask_host);
    if (c->hist_staging) hipFree(c->hist_staging);
    if (c->coarse) hipFree(c->coarse);
    if (c->cells) hipFree(c->cells);
    if (c->k1_tiles) hipFree(c->k1_tiles);
    if (c->fg_tiles) hipFree(c->fg_tiles);
    if (c->env) hipFree(c->env);
    if (c->env_marginal) hipFree(c->env_marginal);
    if (c->env_conditional) hipFree(c->env_conditional);
    prof_recycle(c);
    for (hipEvent_t e : c->prof_free) hipEventDestroy(e);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
}

const char *rfx_last_error(const rfx_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int rfx_get_geometry(const rfx_ctx *c, int *width, int *height, int *tile_y0, int *tile_rows, int *halo_rows) {
    if (!c) return RFX_EINVAL;
    if (width) *width = c->W;
    if (height) *height = c->H;
    if (tile_y0) *tile_y0 = c->tile_y0;
    if (tile_rows) *tile_rows = c->tile_rows;
    if (halo_rows) *halo_rows = c->halo;
    return RFX_OK;
}

int rfx_set_stream(rfx_ctx *c, void *hip_stream) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    // work already enqueued (uploads, the zero-fill of fresh render targets) must not race kernels on the new stream
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return RFX_OK;
}

int rfx_set_row_window(rfx_ctx *c, int y0, int y1) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    if (y1 <= y0) { c->win_y0 = 0; c->win_y1 = 0x7fffffff; }  // reset
    else { c->win_y0 = y0; c->win_y1 = y1; }
    return RFX_OK;
}

int rfx_set_uv_model(rfx_ctx *c, int model) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    if (model != RFX_UV_IDEAL && model != RFX_UV_REFERENCE_GL) return fail(c, RFX_EINVAL, "rfx_set_uv_model: unknown model");
    c->uv_model = model;
    return RFX_OK;
}

int rfx_tex_held_rows(const rfx_ctx *c, rfx_tex id, int *row0, int *rows) {
    if (!c || id < 0 || id >= RFX_TEX_COUNT) return RFX_EINVAL;
    if (row0) *row0 = c->slots[id].row0;
    if (rows) *rows = c->slots[id].rows;
    return RFX_OK;
}

// The depth slot has a new writer.  Every entry point that can write the slot calls this: the foreground map of the last K1 pre-pass no
// longer describes the plane (depth_gen, rfx_ctx.h), and the next pre-pass must know what to wait for.
enum DepthWriter {
    DEPTH_WRITTEN,   // the write is complete: nothing for the pre-pass to wait for
    DEPTH_PENDING,   // the caller has just recorded ev_depth behind the write: the pre-pass waits for it on its own stream
    DEPTH_EXTERNAL,  // written by work this library cannot see, ordered against the draw stream only: the pre-pass stays in the draw stream
};
static void depth_new_writer(rfx_ctx *c, DepthWriter w) {
    if (w == DEPTH_EXTERNAL) c->depth_external = true;
    else c->depth_event_set = w == DEPTH_PENDING;
    c->depth_gen++;
}

static int ensure(rfx_ctx *c, int id) {
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

static int band_check(rfx_ctx *c, int id, int row0, int rows) {
    if (id < 0 || id >= RFX_TEX_COUNT) return fail(c, RFX_EINVAL, "bad texture id");
    const Slot &s = c->slots[id];
    if (rows <= 0 || row0 < s.row0 || row0 + rows > s.row0 + s.rows) return fail(c, RFX_EINVAL, "row band outside the rows this context holds");
    return RFX_OK;
}
// where frame row `frame_row` (a row of the held band) starts in a slot's buffer, and in its back buffer
static size_t slot_row_offset(const Slot &s, int frame_row) { return (size_t)(frame_row - s.row0) * s.width * s.texel; }
static char *slot_row(const Slot &s, int frame_row) { return (char *)s.ptr + slot_row_offset(s, frame_row); }
static char *slot_back_row(const Slot &s, int frame_row) { return (char *)s.back + slot_row_offset(s, frame_row); }
// An input slot holds something: a host-filled plane must have been uploaded (packed, staged or bound), as K2 / K3 require of theirs; a slot a
// draw writes must at least exist — a draw, an upload or a clear made it
static bool slot_filled(const rfx_ctx *c, int id) {
    const bool host_filled = id == RFX_TEX_VELOCITY || id == RFX_TEX_BLUE_NOISE || id == RFX_TEX_DIRECT_LIGHT || id == RFX_TEX_EFFECT_INPUT;
    return host_filled ? c->slots[id].uploaded : c->slots[id].ptr != nullptr;
}
// "fn: what" into the context's error text
static int fail_in(rfx_ctx *c, int code, const char *fn, const char *what) {
    char buf[384];
    snprintf(buf, sizeof buf, "%s: %s", fn, what);
    return fail(c, code, buf);
}

int rfx_upload(rfx_ctx *c, rfx_tex id, const void *host, int row0, int rows) {
    if (!c || !host) return RFX_EINVAL;
    int rc = band_check(c, id, row0, rows);
    if (rc) return rc;
    if ((rc = ensure(c, id))) return rc;
    RFX_ENTER(c);
    Slot &s = c->slots[id];
    const size_t pitch = (size_t)s.width * s.texel;
    HIPCHK(c, hipMemcpyAsync(slot_row(s, row0), host, (size_t)rows * pitch, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller may free `host` as soon as we return
    s.uploaded = true;
    if (id == RFX_TEX_DEPTH) depth_new_writer(c, DEPTH_WRITTEN);
    return RFX_OK;
}

int rfx_download(rfx_ctx *c, rfx_tex id, void *host, int row0, int rows) {
    if (!c || !host) return RFX_EINVAL;
    int rc = band_check(c, id, row0, rows);
    if (rc) return rc;
    if ((rc = ensure(c, id))) return rc;
    RFX_ENTER(c);
    Slot &s = c->slots[id];
    const size_t pitch = (size_t)s.width * s.texel;
    HIPCHK(c, hipMemcpyAsync(host, slot_row(s, row0), (size_t)rows * pitch, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RFX_OK;
}

// ---- streaming dumps: the next frame's planes cross PCIe on their own stream while the current frame is drawn
void *rfx_host_alloc(size_t bytes) {
    void *p = nullptr;
    return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void rfx_host_free(void *p) {
    if (p) hipHostFree(p);
}

static bool is_dump_input(int id) { return id == RFX_TEX_DEPTH || id == RFX_TEX_GBUFFER || id == RFX_TEX_VELOCITY || id == RFX_TEX_DIRECT_LIGHT; }

// the upload stream and the events that order it against the draws, created by the first staged call
static int stage_streams(rfx_ctx *c) {
    if (c->upload_stream) return RFX_OK;
    hipError_t e = hipStreamCreateWithFlags(&c->upload_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_staged, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_frame_done, hipEventDisableTiming);
    for (hipEvent_t &b : c->ev_batch)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&b, hipEventDisableTiming);
    if (e != hipSuccess) return fail(c, RFX_EDEVICE, "rfx_stage_upload: stream/event creation", e);
    // nothing of an earlier frame can still be reading a back buffer: there is none yet
    HIPCHK(c, hipEventRecord(c->ev_frame_done, c->stream));
    return RFX_OK;
}
// ... and a slot's back buffer
static int stage_back(rfx_ctx *c, Slot &s) {
    if (s.back) return RFX_OK;
    hipError_t e = hipMalloc(&s.back, (size_t)s.rows * s.width * s.texel);
    if (e != hipSuccess) return fail(c, RFX_ENOMEM, "hipMalloc(back buffer)", e);
    return RFX_OK;
}

int rfx_stage_upload(rfx_ctx *c, rfx_tex id, const void *host, int row0, int rows) {
    if (!c || !host) return RFX_EINVAL;
    if (!is_dump_input(id)) return fail(c, RFX_EINVAL, "rfx_stage_upload: only the dump's input planes (depth, gbuffer, velocity, direct light) are double-buffered");
    int rc = band_check(c, id, row0, rows);
    if (rc) return rc;
    if ((rc = ensure(c, id))) return rc;
    RFX_ENTER(c);
    Slot &s = c->slots[id];
    if (!s.owned) return fail(c, RFX_ESTATE, "rfx_stage_upload: the slot is bound to an external buffer");
    const size_t pitch = (size_t)s.width * s.texel;
    if ((rc = stage_streams(c))) return rc;
    if ((rc = stage_back(c, s))) return rc;
    // the buffer being filled was the FRONT buffer until the last flip: the draws that read it were enqueued before that flip
    HIPCHK(c, hipStreamWaitEvent(c->upload_stream, c->ev_frame_done, 0));
    HIPCHK(c, hipMemcpyAsync(slot_back_row(s, row0), host, (size_t)rows * pitch, hipMemcpyHostToDevice, c->upload_stream));
    s.back_filled = true;
    return RFX_OK;
}

// ---- streamed AOV frames (include/rfx.h): the planes of rfx_pack_gbuffer / rfx_pack_velocity / the depth and direct uploads, staged once on the
// upload stream and packed by one fused kernel (k0_import.hip k0_aov_pack) into the back buffers rfx_stage_flip publishes
static const rfx_plane *aov_planes(const rfx_aov_frame *f) { return &f->diffuse; }  // eight rfx_plane in RFX_AOV_* order
static const char *aov_plan(const rfx_ctx *c, const rfx_aov_frame *f, int row0, int rows, rfx_aov_plan *t) {
    static_assert(sizeof(rfx_aov_frame) == RFX_AOV_PLANES * sizeof(rfx_plane), "rfx_aov_frame is eight planes");
    int type[RFX_AOV_PLANES], channels[RFX_AOV_PLANES];
    for (int i = 0; i < RFX_AOV_PLANES; i++) {
        const rfx_plane &p = aov_planes(f)[i];
        type[i] = p.type;
        channels[i] = p.data ? p.channels : 0;
        if (p.data && p.channels <= 0) return "a plane's channel count";
    }
    const Slot &g = c->slots[RFX_TEX_GBUFFER];  // (VELOCITY and DIRECT_LIGHT hold the same rows)
    return rfx_aov_plan_for(c->W, c->H, g.row0, g.rows, type, channels, row0, rows, t);
}

// one segment's pack launch on the upload stream: A holds the segment's staged planes, their half mask and the rgb(a) channel counts
static hipError_t aov_pack_segment(rfx_ctx *c, const rfx_aov_plan &t, const rfx_aov_segment &g, K0AovArgs A) {
    const auto first = [&](int id) { return slot_back_row(c->slots[id], g.row0); };
    A.depth = (float *)first(RFX_TEX_DEPTH);
    if (g.full && t.write_gbuffer) A.gbuffer = (uint4 *)first(RFX_TEX_GBUFFER);
    if (g.full && t.write_velocity) A.velocity = (uint4 *)first(RFX_TEX_VELOCITY);
    if (g.full && t.write_direct) A.direct = (uint4 *)first(RFX_TEX_DIRECT_LIGHT);
    A.groups = g.groups; A.tail_start = g.tail_start; A.tail_pixels = g.tail_pixels;
    return rfx_launch_k0_aov(A, g.blocks, c->upload_stream);
}

size_t rfx_aov_stage_bytes(const rfx_ctx *c, const rfx_aov_frame *f, int row0, int rows) {
    rfx_aov_plan t;
    if (!c || !f || aov_plan(c, f, row0, rows, &t)) return 0;
    return (size_t)t.copy_bytes;
}

int rfx_stage_aov(rfx_ctx *c, const rfx_aov_frame *f, int row0, int rows) {
    if (!c || !f) return RFX_EINVAL;
    RFX_ENTER(c);
    rfx_aov_plan t;
    if (const char *bad = aov_plan(c, f, row0, rows, &t)) return fail_in(c, RFX_EINVAL, "rfx_stage_aov", bad);
    const int ids[4] = {RFX_TEX_DEPTH, RFX_TEX_GBUFFER, RFX_TEX_VELOCITY, RFX_TEX_DIRECT_LIGHT};
    const bool writes[4] = {true, t.write_gbuffer != 0, t.write_velocity != 0, t.write_direct != 0};
    int rc;
    for (int k = 0; k < 4; k++) {  // every check before anything is enqueued
        if (!writes[k]) continue;
        if ((rc = ensure(c, ids[k]))) return rc;
        if (!c->slots[ids[k]].owned) return fail_in(c, RFX_ESTATE, "rfx_stage_aov", "a slot to be written is bound to an external buffer");
    }
    if ((rc = stage_streams(c))) return rc;
    for (int k = 0; k < 4; k++)
        if (writes[k] && (rc = stage_back(c, c->slots[ids[k]]))) return rc;
    if (c->aov_stage_cap < (size_t)t.stage_bytes) {
        // (the one wait of this path, paid when the area grows: an earlier call's kernel may still be reading the area that goes)
        if (c->aov_stage) { HIPCHK(c, hipStreamSynchronize(c->upload_stream)); hipFree(c->aov_stage); }
        c->aov_stage = nullptr;
        c->aov_stage_cap = 0;
        hipError_t e = hipMalloc(&c->aov_stage, (size_t)t.stage_bytes);
        if (e != hipSuccess) return fail(c, RFX_ENOMEM, "rfx_stage_aov: hipMalloc(staging area)", e);
        c->aov_stage_cap = (size_t)t.stage_bytes;
    }
    // rfx_stage_upload's order: the back buffers were the front buffers until the last flip
    HIPCHK(c, hipStreamWaitEvent(c->upload_stream, c->ev_frame_done, 0));
    for (int k = 0; k < t.nseg; k++) {
        const rfx_aov_segment &g = t.seg[k];
        K0AovArgs A = {};
        for (int i = 0; i < RFX_AOV_PLANES; i++) {
            if (g.offset[i] == ~0ull) continue;
            const rfx_plane &p = aov_planes(f)[i];
            const size_t texel = (size_t)p.channels * t.elem_bytes[i];
            void *dev = (char *)c->aov_stage + g.offset[i];
            HIPCHK(c, hipMemcpyAsync(dev, (const char *)p.data + (size_t)(g.row0 - row0) * c->W * texel, (size_t)g.pixels * texel, hipMemcpyHostToDevice, c->upload_stream));
            A.plane[i] = dev;
            if (p.type == RFX_PLANE_F16) A.half_mask |= 1u << i;
        }
        A.diffuse_ch = f->diffuse.channels; A.direct_ch = f->direct.channels;
        HIPCHK(c, aov_pack_segment(c, t, g, A));
    }
    for (int k = 0; k < 4; k++)
        if (writes[k]) c->slots[ids[k]].back_filled = true;
    return RFX_OK;
}

// ---- streamed EXR frames and EXR blocks (include/rfx.h): the file's chunks or tiles cross PCIe packed; K9 (k9_exr_import.hip) turns them into the
// staged planes of the plan above, and the same pack launches follow.  One plan serves both entry points: a block is a rectangle of the frame,
// a scanline chunk the block with x = 0, cols = W.
struct ExrPlan {
    rfx_aov_plan aov;
    int type[RFX_AOV_PLANES], channels[RFX_AOV_PLANES];
    std::vector<K9Part> parts;
    std::vector<K9Chan> chans;
    std::vector<char> mapped;     // per part: one of its channels feeds a plane
    std::vector<K9Chunk> chunks;  // the ones the band needs, in the descriptor's order
    std::vector<unsigned long long> file_offset;  // of each of them
    unsigned long long copy_bytes = 0, packed_bytes = 0, scratch_bytes = 0;  // host -> device; the two device areas (256-byte-aligned pieces)
    int rle_chunks = 0, piz_chunks = 0;
};
static unsigned long long align256(unsigned long long n) { return (n + 255ull) & ~255ull; }

// The parts, their channels and the planes they make.  allowed: bit k set = compression k is taken.  0, or the RFX_EINVAL case in words.
static const char *exr_parts_plan(const rfx_ctx *c, const rfx_exr_part *part, int nparts, unsigned int allowed, const char *bad_compression, int row0, int rows,
                                  ExrPlan *p) {
    static const int want_max[RFX_AOV_PLANES] = {4, 3, 1, 1, 3, 2, 1, 4};
    unsigned int comp_mask[RFX_AOV_PLANES] = {0}, any_float[RFX_AOV_PLANES] = {0};
    p->mapped.assign((size_t)nparts, 0);
    for (int k = 0; k < nparts; k++) {
        const rfx_exr_part &q = part[k];
        if (q.compression < 0 || q.compression > 31 || !(allowed >> q.compression & 1u)) return bad_compression;
        if (q.channels <= 0 || q.channels > 1024 || !q.channel) return "a part's channel list";
        K9Part kp = {(int)p->chans.size(), q.channels, 0u, 0u, q.compression};
        for (int i = 0; i < q.channels; i++) {
            const rfx_exr_channel &ch = q.channel[i];
            if (ch.pixel_type != RFX_EXR_HALF && ch.pixel_type != RFX_EXR_FLOAT) return "a channel's pixel type must be HALF or FLOAT (UINT channels are not streamed)";
            if (ch.plane < RFX_EXR_SKIP || ch.plane >= RFX_AOV_PLANES) return "a channel's plane";
            const bool half = ch.pixel_type == RFX_EXR_HALF;
            if (ch.plane >= 0) {
                if (ch.component < 0 || ch.component >= want_max[ch.plane]) return "a channel's component";
                if (comp_mask[ch.plane] & (1u << ch.component)) return "two channels feed one component of a plane";
                comp_mask[ch.plane] |= 1u << ch.component;
                any_float[ch.plane] |= half ? 0u : 1u;
                p->mapped[k] = 1;
            }
            p->chans.push_back({half ? 1 : 0, ch.plane, ch.plane >= 0 ? ch.component : 0, kp.texel_bytes, kp.pxr_bytes});
            kp.texel_bytes += half ? 2u : 4u;  // (at most 1024 channels: <= 4096)
            kp.pxr_bytes += half ? 2u : 3u;
        }
        p->parts.push_back(kp);
    }
    for (int i = 0; i < RFX_AOV_PLANES; i++) {
        int n = 0;
        while (comp_mask[i] >> n & 1u) n++;
        if (comp_mask[i] != (1u << n) - 1u) return "a plane's components must be 0 .. n-1, each fed by one channel";
        p->channels[i] = n;
        p->type[i] = any_float[i] ? RFX_PLANE_F32 : RFX_PLANE_F16;
    }
    const Slot &g = c->slots[RFX_TEX_GBUFFER];
    return rfx_aov_plan_for(c->W, c->H, g.row0, g.rows, p->type, p->channels, row0, rows, &p->aov);
}

// Coverage of the band's scanlines [y_lo, y_hi) by the blocks of ONE mapped part (first .. last: the rows of each clipped to the band, sorted by
// (lo, hi, x)): every texel in exactly one block.  The x-intervals of a row are sorted and must tile [0, W) — per group of blocks on the same rows
// where such groups follow each other (scanline chunks, tiles), else row by row.
struct ExrSpan { int part, lo, hi, x, cols; };
static const char *exr_cover_row(std::vector<std::pair<int, int>> &iv, int W, const char *overlap, const char *hole) {
    std::sort(iv.begin(), iv.end());
    int x = 0;
    for (const std::pair<int, int> &q : iv) {
        if (q.first < x) return overlap;
        if (q.first > x) return hole;
        x = q.first + q.second;
    }
    return x == W ? nullptr : hole;
}
static const char *exr_cover_part(const ExrSpan *first, const ExrSpan *last, int W, int y_lo, int y_hi, const char *overlap, const char *hole) {
    unsigned long long area = 0;
    for (const ExrSpan *q = first; q != last; q++) area += (unsigned long long)(q->hi - q->lo) * (unsigned long long)q->cols;
    const unsigned long long want = (unsigned long long)(y_hi - y_lo) * (unsigned long long)W;
    if (area != want) return area > want ? overlap : hole;  // (so whatever follows handles at most W x rows texel rows)
    std::vector<std::pair<int, int>> iv;
    bool grouped = true;
    int at = y_lo;
    for (const ExrSpan *g = first; g != last && grouped;) {
        const ExrSpan *e = g;
        while (e != last && e->lo == g->lo && e->hi == g->hi) e++;
        if (g->lo > at) return hole;  // (sorted by lo: nothing later holds scanline `at`)
        grouped = g->lo == at;
        at = g->hi;
        g = e;
    }
    if (grouped) {
        for (const ExrSpan *g = first; g != last;) {
            iv.clear();
            const ExrSpan *e = g;
            for (; e != last && e->lo == g->lo && e->hi == g->hi; e++) iv.push_back({e->x, e->cols});
            if (const char *bad = exr_cover_row(iv, W, overlap, hole)) return bad;
            g = e;
        }
        return nullptr;  // (the groups' rows follow each other from y_lo and the areas add up: they end at y_hi)
    }
    for (int y = y_lo; y < y_hi; y++) {  // blocks of different row ranges side by side
        iv.clear();
        for (const ExrSpan *q = first; q != last && q->lo <= y; q++)
            if (q->hi > y) iv.push_back({q->x, q->cols});
        if (const char *bad = exr_cover_row(iv, W, overlap, hole)) return bad;
    }
    return nullptr;
}

// The blocks: geometry, sizes, the band's blocks and their coverage.  A pure function of the descriptor and the context's geometry, after
// exr_parts_plan.  0, or the RFX_EINVAL case in words.
// accept_piz: a PIZ part's blocks are taken (its geometry rules: include/rfx.h "EXR blocks with PIZ"); the parts' plan has refused one otherwise.
static const char *exr_blocks_plan(const rfx_ctx *c, unsigned long long file_bytes, const rfx_exr_block *block, int nblocks, int row0, int rows, const char *overlap,
                                   const char *hole, ExrPlan *p, bool accept_piz = false) {
    const int W = c->W, H = c->H, nparts = (int)p->parts.size();
    const int y_lo = H - row0 - rows, y_hi = H - row0;  // the band's scanlines, top first
    std::vector<ExrSpan> spans;
    for (int k = 0; k < nblocks; k++) {
        const rfx_exr_block &q = block[k];
        if (q.part < 0 || q.part >= nparts) return "a block's part";
        const K9Part &part = p->parts[q.part];
        if (q.x < 0 || q.y < 0 || q.cols < 1 || q.rows < 1 || q.x >= W || q.y >= H || q.cols > W - q.x || q.rows > H - q.y) return "a block does not lie inside the frame";
        const unsigned long long texels = (unsigned long long)q.rows * (unsigned long long)q.cols, raw = texels * part.texel_bytes;
        if (raw >= (1ull << 30)) return "a block of 2^30 raw bytes or more";
        if (q.packed_bytes == 0 || q.packed_bytes >= (1ull << 30) || (part.compression == RFX_EXR_NONE && q.packed_bytes != raw)) return "a block's packed size does not fit its texels";
        if (q.offset > file_bytes || q.packed_bytes > file_bytes - q.offset) return "a block lies outside the file bytes";
        int piz = 0;
        if (part.compression == RFX_EXR_PIZ) {
            if (!accept_piz) return "a PIZ part";
            if (q.cols >= 2 * RFX_EXR_PIZ_CELL && q.rows >= 2 * RFX_EXR_PIZ_CELL) return "a PIZ block of 128 x 128 texels or more";
            piz = q.packed_bytes != raw;
        }
        if (!p->mapped[q.part] || q.y >= y_hi || q.y + q.rows <= y_lo) continue;
        const unsigned long long expect = part.compression == RFX_EXR_PXR24 && q.packed_bytes != raw ? texels * part.pxr_bytes : raw;
        if (part.compression == RFX_EXR_RLE && q.packed_bytes != raw) p->rle_chunks++;
        p->chunks.push_back({p->packed_bytes, p->scratch_bytes, (unsigned int)q.packed_bytes, (unsigned int)raw, (unsigned int)expect, q.part, q.x, q.y, q.cols, q.rows, k, piz ? p->piz_chunks : 0});
        p->piz_chunks += piz;
        p->file_offset.push_back(q.offset);
        p->copy_bytes += q.packed_bytes;
        p->packed_bytes += align256(q.packed_bytes);
        p->scratch_bytes += align256(raw);
        spans.push_back({q.part, q.y > y_lo ? q.y : y_lo, q.y + q.rows < y_hi ? q.y + q.rows : y_hi, q.x, q.cols});
    }
    std::sort(spans.begin(), spans.end(), [](const ExrSpan &a, const ExrSpan &b) {
        return a.part != b.part ? a.part < b.part : a.lo != b.lo ? a.lo < b.lo : a.hi != b.hi ? a.hi < b.hi : a.x < b.x;
    });
    size_t at = 0;
    for (int k = 0; k < nparts; k++) {
        if (!p->mapped[k]) continue;
        size_t end = at;
        while (end < spans.size() && spans[end].part == k) end++;
        if (const char *bad = exr_cover_part(spans.data() + at, spans.data() + end, W, y_lo, y_hi, overlap, hole)) return bad;
        at = end;
    }
    return nullptr;
}

// rfx_stage_exr_aov's checks and layout: its own rules for a scanline chunk, then the blocks' plan
static const char *exr_plan(const rfx_ctx *c, const rfx_exr_frame *f, int row0, int rows, ExrPlan *p) {
    if (!f->data || !f->bytes || f->parts <= 0 || f->chunks <= 0 || !f->part || !f->chunk) return "an empty descriptor";
    if (f->chunks >= (1 << 23) || f->parts > 4096) return "more than 2^23 chunks or 4096 parts";
    const int W = c->W, H = c->H;
    if (const char *bad = exr_parts_plan(c, f->part, f->parts, 1u << RFX_EXR_NONE | 1u << RFX_EXR_ZIPS | 1u << RFX_EXR_ZIP, "a part's compression is none of NONE, ZIPS, ZIP",
                                         row0, rows, p))
        return bad;
    std::vector<rfx_exr_block> blocks((size_t)f->chunks);
    for (int k = 0; k < f->chunks; k++) {
        const rfx_exr_chunk &q = f->chunk[k];
        if (q.part < 0 || q.part >= f->parts) return "a chunk's part";
        const int per = f->part[q.part].compression == RFX_EXR_ZIP ? 16 : 1;
        if (q.y < 0 || q.y >= H || q.y % per || q.rows != (H - q.y < per ? H - q.y : per)) return "a chunk's scanline or row count does not fit its part's header";
        const unsigned long long raw = (unsigned long long)q.rows * W * p->parts[q.part].texel_bytes;
        if (raw >= (1ull << 30)) return "a chunk of 2^30 raw bytes or more";
        if (q.packed_bytes == 0 || q.packed_bytes >= (1ull << 30) || (f->part[q.part].compression == RFX_EXR_NONE && q.packed_bytes != raw)) return "a chunk's packed size does not fit its rows";
        if (q.offset > f->bytes || q.packed_bytes > f->bytes - q.offset) return "a chunk lies outside the file bytes";
        blocks[(size_t)k] = {q.part, 0, q.y, W, q.rows, 0, q.offset, q.packed_bytes};
    }
    return exr_blocks_plan(c, f->bytes, blocks.data(), f->chunks, row0, rows, "two chunks of a part hold one scanline",
                           "a scanline of the band has no chunk in a part that feeds a plane", p);
}

static const char *exr_block_frame_plan(const rfx_ctx *c, const rfx_exr_block_frame *f, int row0, int rows, ExrPlan *p, bool accept_piz = false) {
    if (!f->data || !f->bytes || f->parts <= 0 || f->blocks <= 0 || !f->part || !f->block) return "an empty descriptor";
    if (f->blocks >= (1 << 23) || f->parts > 4096) return "more than 2^23 blocks or 4096 parts";
    const unsigned int five = 1u << RFX_EXR_NONE | 1u << RFX_EXR_RLE | 1u << RFX_EXR_ZIPS | 1u << RFX_EXR_ZIP | 1u << RFX_EXR_PXR24;
    if (const char *bad = exr_parts_plan(c, f->part, f->parts, accept_piz ? five | 1u << RFX_EXR_PIZ : five,
                                         accept_piz ? "a part's compression is none of NONE, RLE, ZIPS, ZIP, PIZ, PXR24" : "a part's compression is none of NONE, RLE, ZIPS, ZIP, PXR24",
                                         row0, rows, p))
        return bad;
    return exr_blocks_plan(c, f->bytes, f->block, f->blocks, row0, rows, "two blocks of a part hold one texel of the band",
                           "a texel of the band has no block in a part that feeds a plane", p, accept_piz);
}

size_t rfx_exr_aov_stage_bytes(const rfx_ctx *c, const rfx_exr_frame *f, int row0, int rows) {
    ExrPlan p;
    if (!c || !f || exr_plan(c, f, row0, rows, &p)) return 0;
    return (size_t)p.copy_bytes;
}

size_t rfx_exr_blocks_stage_bytes(const rfx_ctx *c, const rfx_exr_block_frame *f, int row0, int rows) {
    ExrPlan p;
    if (!c || !f || exr_block_frame_plan(c, f, row0, rows, &p)) return 0;
    return (size_t)p.copy_bytes;
}

size_t rfx_exr_blocks_piz_stage_bytes(const rfx_ctx *c, const rfx_exr_block_frame *f, int row0, int rows) {
    ExrPlan p;
    if (!c || !f || exr_block_frame_plan(c, f, row0, rows, &p, true)) return 0;
    return (size_t)p.copy_bytes;
}

// a device area of the context grows: the one wait of the staged paths (an earlier call's kernels may still be using the area that goes)
static int grow_stage_area(rfx_ctx *c, void **area, size_t *cap, size_t need, const char *what) {
    if (*cap >= need) return RFX_OK;
    if (*area) { HIPCHK(c, hipStreamSynchronize(c->upload_stream)); hipFree(*area); }
    *area = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(area, need);
    if (e != hipSuccess) return fail(c, RFX_ENOMEM, what, e);
    *cap = need;
    return RFX_OK;
}

// what both entry points do with a plan: the copies, K9's launches, the status read-back and the pack launches, on the upload stream
static int stage_exr_plan(rfx_ctx *c, const ExrPlan &p, const void *data, const char *fn) {
    const rfx_aov_plan &t = p.aov;
    const int ids[4] = {RFX_TEX_DEPTH, RFX_TEX_GBUFFER, RFX_TEX_VELOCITY, RFX_TEX_DIRECT_LIGHT};
    const bool writes[4] = {true, t.write_gbuffer != 0, t.write_velocity != 0, t.write_direct != 0};
    int rc;
    for (int k = 0; k < 4; k++) {  // every check before anything is enqueued
        if (!writes[k]) continue;
        if ((rc = ensure(c, ids[k]))) return rc;
        if (!c->slots[ids[k]].owned) return fail_in(c, RFX_ESTATE, fn, "a slot to be written is bound to an external buffer");
    }
    if ((rc = stage_streams(c))) return rc;
    for (int k = 0; k < 4; k++)
        if (writes[k] && (rc = stage_back(c, c->slots[ids[k]]))) return rc;
    // the device area: parts | channels | chunks | error words | status | packed bytes | inflate scratch | PIZ tables, every piece 256-byte aligned
    rfx_exr_piz_tables piz;
    if (!rfx_exr_piz_tables_for(p.piz_chunks, &piz)) return fail_in(c, RFX_EINVAL, fn, "too many PIZ blocks");
    const size_t n = p.chunks.size();
    const size_t parts_b = align256(p.parts.size() * sizeof(K9Part)), chans_b = align256(p.chans.size() * sizeof(K9Chan)), chunks_b = align256(n * sizeof(K9Chunk));
    const size_t tables_b = parts_b + chans_b + chunks_b, err_b = align256(n * sizeof(int)), status_b = 256;
    const size_t need = tables_b + err_b + status_b + (size_t)p.packed_bytes + (size_t)p.scratch_bytes + (size_t)piz.bytes;
    if ((rc = grow_stage_area(c, &c->aov_stage, &c->aov_stage_cap, (size_t)t.stage_bytes, (std::string(fn) + ": hipMalloc(staging area)").c_str()))) return rc;
    if ((rc = grow_stage_area(c, &c->exr_stage, &c->exr_stage_cap, need, (std::string(fn) + ": hipMalloc(chunk area)").c_str()))) return rc;
    if (!c->ev_exr_status) {
        hipError_t e = hipEventCreateWithFlags(&c->ev_exr_status, hipEventDisableTiming);
        if (e != hipSuccess) return fail(c, RFX_EDEVICE, (std::string(fn) + ": the status event").c_str(), e);
    }
    if (!c->exr_status_host) {
        hipError_t e = hipHostMalloc((void **)&c->exr_status_host, 2 * sizeof(int), hipHostMallocDefault);
        if (e != hipSuccess) { c->exr_status_host = nullptr; return fail(c, RFX_ENOMEM, (std::string(fn) + ": the status block").c_str(), e); }
    }
    // the tables, written into this batch's pinned block behind what an earlier call of the batch put there
    const int hb = (int)(c->flips & 1u);
    if (c->exr_tables_batch[hb] != c->flips) { c->exr_tables_batch[hb] = c->flips; c->exr_tables_used[hb] = 0; }
    if (c->exr_tables_used[hb] + tables_b > c->exr_tables_cap[hb]) {
        if (c->exr_tables_host[hb]) { HIPCHK(c, hipStreamSynchronize(c->upload_stream)); hipHostFree(c->exr_tables_host[hb]); }  // (grown: as the device areas)
        c->exr_tables_host[hb] = nullptr;
        c->exr_tables_cap[hb] = c->exr_tables_used[hb] = 0;
        hipError_t e = hipHostMalloc(&c->exr_tables_host[hb], 2 * tables_b, hipHostMallocDefault);
        if (e != hipSuccess) return fail(c, RFX_ENOMEM, (std::string(fn) + ": hipHostMalloc(tables)").c_str(), e);
        c->exr_tables_cap[hb] = 2 * tables_b;
    }
    char *tables = (char *)c->exr_tables_host[hb] + c->exr_tables_used[hb];
    c->exr_tables_used[hb] += tables_b;
    memset(tables, 0, tables_b);
    memcpy(tables, p.parts.data(), p.parts.size() * sizeof(K9Part));
    memcpy(tables + parts_b, p.chans.data(), p.chans.size() * sizeof(K9Chan));
    memcpy(tables + parts_b + chans_b, p.chunks.data(), n * sizeof(K9Chunk));
    char *dev = (char *)c->exr_stage;
    // rfx_stage_upload's order: the back buffers were the front buffers until the last flip
    HIPCHK(c, hipStreamWaitEvent(c->upload_stream, c->ev_frame_done, 0));
    HIPCHK(c, hipMemcpyAsync(dev, tables, tables_b, hipMemcpyHostToDevice, c->upload_stream));
    HIPCHK(c, hipMemsetAsync(dev + tables_b + err_b, 0, status_b, c->upload_stream));
    char *packed = dev + tables_b + err_b + status_b;
    for (size_t k = 0; k < n; k++)  // exactly the packed bytes of every chunk the band needs
        HIPCHK(c, hipMemcpyAsync(packed + p.chunks[k].src, (const char *)data + p.file_offset[k], p.chunks[k].packed, hipMemcpyHostToDevice, c->upload_stream));
    K9Args A = {};
    A.parts = (const K9Part *)dev; A.chans = (const K9Chan *)(dev + parts_b); A.chunks = (const K9Chunk *)(dev + parts_b + chans_b);
    A.nchunks = (int)n; A.rle_chunks = p.rle_chunks;
    A.err = (int *)(dev + tables_b); A.status = (int *)(dev + tables_b + err_b);
    A.packed = (const unsigned char *)packed; A.scratch = (unsigned char *)packed + p.packed_bytes;
    A.piz_chunks = p.piz_chunks; A.piz_tables = p.piz_chunks ? A.scratch + p.scratch_bytes : nullptr;
    A.W = c->W; A.H = c->H;
    A.nseg = t.nseg;
    unsigned int half_mask = 0;
    for (int i = 0; i < RFX_AOV_PLANES; i++) {
        A.plane_ch[i] = p.channels[i];
        A.plane_half[i] = p.channels[i] && p.type[i] == RFX_PLANE_F16;
        if (A.plane_half[i]) half_mask |= 1u << i;
    }
    for (int k = 0; k < t.nseg; k++) {
        A.seg_row0[k] = t.seg[k].row0; A.seg_rows[k] = t.seg[k].rows;
        for (int i = 0; i < RFX_AOV_PLANES; i++) A.seg_plane[k][i] = t.seg[k].offset[i] == ~0ull ? nullptr : (char *)c->aov_stage + t.seg[k].offset[i];
    }
    HIPCHK(c, rfx_launch_k9(A, c->upload_stream));
    HIPCHK(c, hipMemcpyAsync(c->exr_status_host, A.status, 2 * sizeof(int), hipMemcpyDeviceToHost, c->upload_stream));
    HIPCHK(c, hipEventRecord(c->ev_exr_status, c->upload_stream));
    c->exr_staged = true;
    for (int k = 0; k < t.nseg; k++) {
        K0AovArgs P = {};
        for (int i = 0; i < RFX_AOV_PLANES; i++) P.plane[i] = A.seg_plane[k][i];
        P.half_mask = half_mask;
        P.diffuse_ch = p.channels[RFX_AOV_DIFFUSE]; P.direct_ch = p.channels[RFX_AOV_DIRECT];
        HIPCHK(c, aov_pack_segment(c, t, t.seg[k], P));
    }
    for (int k = 0; k < 4; k++)
        if (writes[k]) c->slots[ids[k]].back_filled = true;
    return RFX_OK;
}

int rfx_stage_exr_aov(rfx_ctx *c, const rfx_exr_frame *f, int row0, int rows) {
    if (!c || !f) return RFX_EINVAL;
    RFX_ENTER(c);
    ExrPlan p;
    if (const char *bad = exr_plan(c, f, row0, rows, &p)) return fail_in(c, RFX_EINVAL, "rfx_stage_exr_aov", bad);
    return stage_exr_plan(c, p, f->data, "rfx_stage_exr_aov");
}

int rfx_stage_exr_blocks(rfx_ctx *c, const rfx_exr_block_frame *f, int row0, int rows) {
    if (!c || !f) return RFX_EINVAL;
    RFX_ENTER(c);
    ExrPlan p;
    if (const char *bad = exr_block_frame_plan(c, f, row0, rows, &p)) return fail_in(c, RFX_EINVAL, "rfx_stage_exr_blocks", bad);
    return stage_exr_plan(c, p, f->data, "rfx_stage_exr_blocks");
}

int rfx_stage_exr_blocks_piz(rfx_ctx *c, const rfx_exr_block_frame *f, int row0, int rows) {
    if (!c || !f) return RFX_EINVAL;
    RFX_ENTER(c);
    ExrPlan p;
    if (const char *bad = exr_block_frame_plan(c, f, row0, rows, &p, true)) return fail_in(c, RFX_EINVAL, "rfx_stage_exr_blocks_piz", bad);
    return stage_exr_plan(c, p, f->data, "rfx_stage_exr_blocks_piz");
}

int rfx_exr_aov_status(rfx_ctx *c, int *bad_chunks, int *first_bad, int *code) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    if (!c->exr_staged) return fail(c, RFX_ESTATE, "rfx_exr_aov_status: no EXR frame has been staged");
    HIPCHK(c, hipEventSynchronize(c->ev_exr_status));
    const int bad = c->exr_status_host[0], key = c->exr_status_host[1] ? 0x7fffffff - c->exr_status_host[1] : -1;
    if (bad_chunks) *bad_chunks = bad;
    if (first_bad) *first_bad = key < 0 ? -1 : key >> 8;
    if (code) *code = key < 0 ? 0 : key & 255;
    return RFX_OK;
}

int rfx_stage_flip(rfx_ctx *c) {
    if (!c) return RFX_EINVAL;
    if (!c->upload_stream) return fail(c, RFX_ESTATE, "rfx_stage_flip: nothing staged");
    RFX_ENTER(c);
    // draws enqueued from now on wait for the staged copies; copies staged from now on wait for the draws enqueued so far
    HIPCHK(c, hipEventRecord(c->ev_staged, c->upload_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_staged, 0));
    HIPCHK(c, hipEventRecord(c->ev_frame_done, c->stream));
    // Host-side back pressure.  Neither rfx_stage_upload nor the flip waits for the GPU, and a staged copy executes only once the
    // draws of two frames earlier have finished — a host running ahead (two alternating sets of pinned planes) could refill a set
    // before the copy that reads it has run.  So this flip returns only when the copies published by the PREVIOUS flip have
    // executed: the planes staged before that flip are free to be rewritten, and the host is never more than two frames ahead.
    const unsigned int k = c->flips++;
    HIPCHK(c, hipEventRecord(c->ev_batch[k & 1], c->upload_stream));
    if (k >= 1) HIPCHK(c, hipEventSynchronize(c->ev_batch[(k - 1) & 1]));
    for (int id = 0; id < RFX_TEX_COUNT; id++) {
        Slot &s = c->slots[id];
        if (!s.back_filled) continue;
        if (id == RFX_TEX_DEPTH) {  // the depth pre-pass of the next K1 waits for this copy on its own stream
            HIPCHK(c, hipEventRecord(c->ev_depth, c->upload_stream));
            depth_new_writer(c, DEPTH_PENDING);  // another plane is the depth slot now
        }
        void *t = s.ptr; s.ptr = s.back; s.back = t;
        s.back_filled = false;
        s.uploaded = true;
    }
    return RFX_OK;
}

int rfx_clear(rfx_ctx *c, rfx_tex id) {
    if (!c || id < 0 || id >= RFX_TEX_COUNT) return RFX_EINVAL;
    int rc = ensure(c, id);
    if (rc) return rc;
    RFX_ENTER(c);
    Slot &s = c->slots[id];
    HIPCHK(c, hipMemsetAsync(s.ptr, 0, (size_t)s.rows * s.width * s.texel, c->stream));
    if (id == RFX_TEX_DEPTH) {
        HIPCHK(c, hipEventRecord(c->ev_depth, c->stream));
        depth_new_writer(c, DEPTH_PENDING);
    }
    return RFX_OK;
}

void *rfx_tex_device_ptr(rfx_ctx *c, rfx_tex id) {
    if (!c || id < 0 || id >= RFX_TEX_COUNT) return nullptr;
    hipSetDevice(c->device);
    if (ensure(c, id)) return nullptr;
    // whoever takes the depth plane's address may write it with work this library cannot see (ordered against the draw stream only, as a
    // bound external buffer is): the pre-pass then stays in the draw stream
    if (id == RFX_TEX_DEPTH) depth_new_writer(c, DEPTH_EXTERNAL);
    return c->slots[id].ptr;
}

int rfx_bind_external(rfx_ctx *c, rfx_tex id, void *device_ptr) {
    if (!c || id < 0 || id >= RFX_TEX_COUNT || !device_ptr) return RFX_EINVAL;
    RFX_ENTER(c);
    Slot &s = c->slots[id];
    if (s.owned && s.ptr) {  // launches that still use the old buffer finish first
        HIPCHK(c, hipStreamSynchronize(c->stream));
        hipFree(s.ptr);
    }
    s.ptr = device_ptr;
    s.owned = false;
    s.uploaded = true;
    if (id == RFX_TEX_DEPTH) depth_new_writer(c, DEPTH_EXTERNAL);  // written by whoever owns the buffer
    return RFX_OK;
}

static TexView view(rfx_ctx *c, int id) { return {c->slots[id].ptr, c->slots[id].row0, c->slots[id].rows}; }
static TexViewW wview(rfx_ctx *c, int id) { return {c->slots[id].ptr, c->slots[id].row0, c->slots[id].rows}; }
// The plane equations of a w x h render target's vUv (rfx_device.h UvPlanes; this file is compiled with -ffp-contract=off: every product
// below is rounded on its own, as the reference GL's triangle setup rounds them)
static UvPlanes rfx_uv_planes(int model, int w, int h) {
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
static FrameDims dims(rfx_ctx *c) {
    FrameDims d;
    d.W = c->W; d.H = c->H; d.fW = (float)c->W; d.fH = (float)c->H;
    d.uv = rfx_uv_planes(c->uv_model, c->W, c->H);
    d.halo_violations = c->halo_violations;
    return d;
}
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

// blue_noise.glsl:9-34: one pcg4d round of the per-draw seed; the toroidal shift is pixel-independent
static void blue_noise_shift(int index, int *sx, int *sy) {
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
static bool launch_rows(rfx_ctx *c, int out_id, int extra, int *y0, int *y1) {
    const Slot &s = c->slots[out_id];
    int a = c->tile_y0 - extra, b = c->tile_y0 + c->tile_rows + extra;
    if (a < s.row0) a = s.row0;
    if (b > s.row0 + s.rows) b = s.row0 + s.rows;
    if (a < c->win_y0) a = c->win_y0;  // rfx_set_row_window
    if (b > c->win_y1) b = c->win_y1;
    *y0 = a; *y1 = b;
    return b > a;  // false: nothing to draw
}

// stage `n` host planes (floats per texel in `ch`) of a band on the device, back to back; returns the device base in *stage
static int stage_planes(rfx_ctx *c, const float *const *host, const int *ch, int n, size_t texels, float **stage, const float **dev) {
    size_t total = 0;
    for (int i = 0; i < n; i++) total += host[i] ? texels * ch[i] : 0;
    hipError_t e = hipMalloc((void **)stage, total * sizeof(float));
    if (e != hipSuccess) return fail(c, RFX_ENOMEM, "hipMalloc(AOV staging)", e);
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        dev[i] = nullptr;
        if (!host[i]) continue;
        dev[i] = *stage + off;
        e = hipMemcpyAsync(*stage + off, host[i], texels * ch[i] * sizeof(float), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { hipFree(*stage); return fail(c, RFX_EDEVICE, "hipMemcpyAsync(AOV plane)", e); }
        off += texels * ch[i];
    }
    return RFX_OK;
}

int rfx_pack_gbuffer(rfx_ctx *c, const rfx_aov_gbuffer *a, int row0, int rows) {
    if (!c || !a || !a->diffuse || !a->normal || !a->roughness || !a->metalness || !a->emissive) return RFX_EINVAL;
    int rc = band_check(c, RFX_TEX_GBUFFER, row0, rows);
    if (rc) return rc;
    if ((rc = ensure(c, RFX_TEX_GBUFFER))) return rc;
    RFX_ENTER(c);
    const float *host[6] = {a->diffuse, a->normal, a->roughness, a->metalness, a->emissive, a->depth}, *dev[6];
    const int ch[6] = {4, 3, 1, 1, 3, 1};
    float *stage = nullptr;
    if ((rc = stage_planes(c, host, ch, 6, (size_t)rows * c->W, &stage, dev))) return rc;
    Slot &s = c->slots[RFX_TEX_GBUFFER];
    hipError_t e = rfx_launch_pack_gbuffer(c->W, rows, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], slot_row(s, row0), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the caller may free the planes as soon as we return
    hipFree(stage);
    if (e != hipSuccess) return fail(c, RFX_EDEVICE, "rfx_pack_gbuffer", e);
    s.uploaded = true;
    return RFX_OK;
}

int rfx_pack_velocity(rfx_ctx *c, const rfx_aov_velocity *a, int row0, int rows) {
    if (!c || !a || !a->velocity || !a->normal || !a->depth) return RFX_EINVAL;
    int rc = band_check(c, RFX_TEX_VELOCITY, row0, rows);
    if (rc) return rc;
    if ((rc = ensure(c, RFX_TEX_VELOCITY))) return rc;
    RFX_ENTER(c);
    const float *host[3] = {a->velocity, a->normal, a->depth}, *dev[3];
    const int ch[3] = {2, 3, 1};
    float *stage = nullptr;
    if ((rc = stage_planes(c, host, ch, 3, (size_t)rows * c->W, &stage, dev))) return rc;
    Slot &s = c->slots[RFX_TEX_VELOCITY];
    hipError_t e = rfx_launch_pack_velocity(c->W, rows, dev[0], dev[1], dev[2], slot_row(s, row0), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(stage);
    if (e != hipSuccess) return fail(c, RFX_EDEVICE, "rfx_pack_velocity", e);
    s.uploaded = true;
    return RFX_OK;
}

// the importance tables of an environment, and the environment with them
static void env_tables_release(rfx_ctx *c) {
    if (c->env_marginal) hipFree(c->env_marginal);
    if (c->env_conditional) hipFree(c->env_conditional);
    c->env_marginal = c->env_conditional = nullptr;
}
static void env_release(rfx_ctx *c) {
    if (c->env) hipFree(c->env);
    c->env = nullptr; c->env_w = c->env_h = c->env_levels = 0;
    env_tables_release(c);
}

int rfx_set_environment(rfx_ctx *c, const float *rgba, int width, int height, int halfFloatType, int halfStoreRTZ) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    if (!rgba) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        env_release(c);
        return RFX_OK;
    }
    if (width < 1 || height < 1 || width > 16384 || height > 16384 || (width & (width - 1)) || (height & (height - 1)))
        return fail(c, RFX_EINVAL, "rfx_set_environment: width and height must be powers of two <= 16384");
    int levels = 0;
    size_t total = 0;
    unsigned int off[16];
    for (int w = width, h = height;; w = w > 1 ? w >> 1 : 1, h = h > 1 ? h >> 1 : 1) {
        off[levels++] = (unsigned int)total;
        total += (size_t)w * h;
        if (w == 1 && h == 1) break;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    env_release(c);  // (the tables of the previous map too: a new one needs its own)
    hipError_t e = hipMalloc((void **)&c->env, total * sizeof(float4));
    if (e != hipSuccess) return fail(c, RFX_ENOMEM, "hipMalloc(environment)", e);
    // staging copy of the base level, then level 0 = the texels in the texture's type, then the chain
    float4 *stage = nullptr;
    e = hipMalloc((void **)&stage, (size_t)width * height * sizeof(float4));
    if (e != hipSuccess) {
        env_release(c);
        return fail(c, RFX_ENOMEM, "hipMalloc(environment staging)", e);
    }
    e = hipMemcpyAsync(stage, rgba, (size_t)width * height * sizeof(float4), hipMemcpyHostToDevice, c->stream);
    // level 0: same size "reduction" = a copy through the type conversion (RNE: the upload of a float image into a half texture)
    if (e == hipSuccess) e = rfx_launch_env_mip(stage, c->env, width, height, width, height, halfFloatType != 0, false, c->stream);
    for (int l = 1, w = width, h = height; l < levels && e == hipSuccess; l++) {
        const int dw = w > 1 ? w >> 1 : 1, dh = h > 1 ? h >> 1 : 1;
        e = rfx_launch_env_mip(c->env + off[l - 1], c->env + off[l], w, h, dw, dh, halfFloatType != 0, halfStoreRTZ != 0, c->stream);
        w = dw; h = dh;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the caller may free `rgba` as soon as we return
    hipFree(stage);
    if (e != hipSuccess) {
        env_release(c);
        return fail(c, RFX_EDEVICE, "rfx_set_environment: building the mip chain", e);
    }
    c->env_w = width; c->env_h = height; c->env_levels = levels;
    memcpy(c->env_off, off, sizeof off);
    return RFX_OK;
}

int rfx_cube_to_equirect(rfx_ctx *c, const float *faces, int size, int generateMipmaps, float *equirect, int width, int height) {
    if (!c || !faces || !equirect) return RFX_EINVAL;
    if (size < 1 || size > 8192 || width < 1 || height < 1 || width > 16384 || height > 16384)
        return fail(c, RFX_EINVAL, "rfx_cube_to_equirect: face size must be 1..8192, the target 1..16384 in each edge");
    RFX_ENTER(c);
    int levels = 1;
    size_t nchain = (size_t)6 * size * size;
    if (generateMipmaps)
        for (int s = size >> 1; s >= 1; s >>= 1) { nchain += (size_t)6 * s * s; levels++; }
    const size_t nin = (size_t)6 * size * size, nout = (size_t)width * height;
    float4 *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void **)&din, nchain * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc((void **)&dout, nout * sizeof(float4));
    if (e != hipSuccess) {
        if (din) hipFree(din);
        return fail(c, RFX_ENOMEM, "hipMalloc(cube chain / equirect target)", e);
    }
    e = hipMemcpyAsync(din, faces, nin * sizeof(float4), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = rfx_launch_cube_to_equirect(din, size, levels, dout, width, height, rfx_uv_planes(c->uv_model, width, height), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(equirect, dout, nout * sizeof(float4), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(din);
    hipFree(dout);
    if (e != hipSuccess) return fail(c, RFX_EDEVICE, "rfx_cube_to_equirect", e);
    return RFX_OK;
}

int rfx_set_environment_importance(rfx_ctx *c, const float *marginal, size_t marginalCount, const float *conditional, size_t conditionalCount,
                                   float totalSumWhole, float totalSumDecimal) {
    if (!c || !marginal || !conditional) return RFX_EINVAL;
    if (!c->env) return fail(c, RFX_ESTATE, "rfx_set_environment_importance: no environment set");
    if (marginalCount != (size_t)c->env_h || conditionalCount != (size_t)c->env_w * c->env_h)
        return fail(c, RFX_EINVAL, "rfx_set_environment_importance: marginalWeights must hold height floats and conditionalWeights width*height");
    RFX_ENTER(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    env_tables_release(c);
    hipError_t e = hipMalloc((void **)&c->env_marginal, (size_t)c->env_h * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&c->env_conditional, (size_t)c->env_w * c->env_h * sizeof(float));
    if (e != hipSuccess) {
        env_tables_release(c);
        return fail(c, RFX_ENOMEM, "hipMalloc(environment importance tables)", e);
    }
    e = hipMemcpyAsync(c->env_marginal, marginal, (size_t)c->env_h * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->env_conditional, conditional, (size_t)c->env_w * c->env_h * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {  // tables with undefined contents must not pass the importanceSampling validation
        env_tables_release(c);
        return fail(c, RFX_EDEVICE, "rfx_set_environment_importance: copying the tables", e);
    }
    c->env_sum_whole = totalSumWhole; c->env_sum_decimal = totalSumDecimal;
    return RFX_OK;
}

int rfx_download_environment(rfx_ctx *c, int level, float *rgba, int *levels) {
    if (!c) return RFX_EINVAL;
    if (levels) *levels = c->env_levels;
    if (!rgba) return RFX_OK;
    if (!c->env || level < 0 || level >= c->env_levels) return fail(c, RFX_EINVAL, "rfx_download_environment: no such level");
    const int w = (c->env_w >> level) > 0 ? c->env_w >> level : 1, h = (c->env_h >> level) > 0 ? c->env_h >> level : 1;
    RFX_ENTER(c);
    HIPCHK(c, hipMemcpyAsync(rgba, c->env + c->env_off[level], (size_t)w * h * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
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
    if (p->importanceSampling && (!p->useEnvMap || !c->env_marginal))
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

// the two launch plans as built, for the CPU tests (rfx_launch.h)
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
int rfx_internal_aov_plan(int W, int H, int held_row0, int held_rows, const int *type, const int *channels, int row0, int rows, struct rfx_aov_plan *out) {
    return rfx_aov_plan_for(W, H, held_row0, held_rows, type, channels, row0, rows, out) ? RFX_EINVAL : RFX_OK;
}
int rfx_internal_exr_piz_tables(int piz_blocks, struct rfx_exr_piz_tables *out) { return out && rfx_exr_piz_tables_for(piz_blocks, out) ? 0 : -1; }
int rfx_internal_k3_tile(int W, int H, float radius, int inputIsTemporal, int textureCount, struct rfx_k3_tile_plan *out) {
    *out = rfx_k3_tile((float)W, (float)H, radius, inputIsTemporal != 0, textureCount);
    return RFX_OK;
}

// the row-mask scratch of the bounded gathers (rfx_ctx.h hit_mask_dev / hit_mask_host), sized for `ranks` gathered copies
static int hit_mask_scratch(rfx_ctx *c, int ranks) {
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

// the first H words of hit_mask_dev (the mask an enqueue above left on the draw stream) -> hit_mask_host, and into row_mask when given
static int hit_mask_read_back(rfx_ctx *c, unsigned int *row_mask) {
    const size_t bytes = (size_t)c->H * sizeof(unsigned int);
    HIPCHK(c, hipMemcpyAsync(c->hit_mask_host, c->hit_mask_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (row_mask) memcpy(row_mask, c->hit_mask_host, bytes);
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

// ---- K6: rfx_motion_blur and, for row-tiled contexts, its reach mask / stage (the gather is in rfx_comm.hip)
static bool is_tiled(const rfx_ctx *c) { return c->tile_y0 != 0 || c->tile_rows != c->H; }

// the parameters, then (the draw only) whether a row-tiled context is armed, then the input slots: rfx_motion_blur's codes for all four calls
static int k6_validate(rfx_ctx *c, const rfx_motion_blur_params *p, bool draw) {
    const auto tap_slot = [](int id) {
        return id == RFX_TEX_FINAL || id == RFX_TEX_TEMPORAL0 || id == RFX_TEX_DIRECT_LIGHT || id == RFX_TEX_SSGI || id == RFX_TEX_EFFECT_INPUT;
    };
    if (!tap_slot(p->source)) return fail(c, RFX_EINVAL, "rfx_motion_blur: source must be FINAL, TEMPORAL0, DIRECT_LIGHT, SSGI or EFFECT_INPUT");
    const int center = p->center == -1 ? p->source : p->center;
    if (!tap_slot(center)) return fail(c, RFX_EINVAL, "rfx_motion_blur: center must be -1 or one of the source slots");
    if (p->samples < 1 || p->samples > 65536) return fail(c, RFX_EINVAL, "rfx_motion_blur: samples must be in [1, 65536]");
    if (!(p->deltaTime > 0.0f) || !(p->deltaTime <= 3.402823466e38f)) return fail(c, RFX_EINVAL, "rfx_motion_blur: deltaTime must be finite and > 0");
    for (int k = 0; k < 2; k++)
        if (!(p->resolution[k] > 0.0f) || !(p->resolution[k] <= 65536.0f)) return fail(c, RFX_EINVAL, "rfx_motion_blur: resolution must be in (0, 65536]");
    if (p->frame < 0) return fail(c, RFX_EINVAL, "rfx_motion_blur: frame must be >= 0 (the reference passes frame % 4096)");
    // a LINEAR footprint at a tile's edge reaches a row the tile does not draw: the source's is gathered (the reach mask names it), another
    // slot's is not.  TRAA's target is NEAREST: the pixel's own texel
    if (is_tiled(c) && p->center != -1 && p->center != RFX_TEX_TEMPORAL0)
        return fail(c, RFX_EUNSUPPORTED, "rfx_motion_blur: on a row-tiled context center must be -1 or RFX_TEX_TEMPORAL0 (another slot is fetched LINEAR, "
                                         "past the rows the tile draws)");
    if (draw && is_tiled(c)) {
        if (c->blur_armed < 0)
            return fail(c, RFX_EUNSUPPORTED, "rfx_motion_blur: needs a whole-frame context (a streak can reach anywhere), or a row-tiled one armed by "
                                             "rfx_motion_blur_stage / rfx_motion_blur_gather");
        if (c->blur_armed != p->source) return fail(c, RFX_ESTATE, "rfx_motion_blur: the row-tiled draw is armed (rfx_motion_blur_stage / rfx_motion_blur_gather) for another source");
    }
    const int ins[] = {RFX_TEX_VELOCITY, RFX_TEX_BLUE_NOISE, p->source, center};
    for (int id : ins)
        if (!slot_filled(c, id))  // (uploaded if the host fills it — the slots a draw writes, FINAL, TEMPORAL0, SSGI, must at least exist)
            return fail(c, RFX_ESTATE, "rfx_motion_blur: an input slot holds nothing yet (upload it or draw into it first)");
    return RFX_OK;
}

// the argument block of the draw and of the reach reduction (no HIP call).  Returns whether there are rows to produce.
static bool k6_args(rfx_ctx *c, const rfx_motion_blur_params *p, K6Args &A) {
    const int center = p->center == -1 ? p->source : p->center;
    const bool tiled = is_tiled(c);
    A.dims = dims(c);
    const bool any = launch_rows(c, RFX_TEX_MOTION_BLUR, 0, &A.y0, &A.y1);
    const Slot &vs = c->slots[RFX_TEX_VELOCITY], &cs = c->slots[center], &os = c->slots[RFX_TEX_MOTION_BLUR];
    A.velocity = (const float4 *)vs.ptr;
    // a row-tiled draw takes its taps — and the own-pass centre, the same buffer — from the whole-frame plane the stage / gather filled
    A.src = (const float4 *)c->slots[tiled ? RFX_TEX_BLUR_SOURCE : p->source].ptr;
    A.center = (tiled && p->center == -1) ? A.src : (const float4 *)cs.ptr;
    A.out = (float4 *)os.ptr;
    A.blue = (const uchar4 *)c->slots[RFX_TEX_BLUE_NOISE].ptr;
    blue_noise_shift(p->frame, &A.shift_x, &A.shift_y);
    // center -1: the own EffectPass, inputColor = texture2D(inputBuffer, vUv), LINEAR on the same buffer as the taps.  An explicit
    // RFX_TEX_TEMPORAL0 is TRAA's render target itself (README form), NearestFilter (TemporalReprojectPass.js:66-67)
    A.center_nearest = p->center == RFX_TEX_TEMPORAL0;
    A.center_alpha_one = p->centerAlphaOne != 0;
    A.target_half = p->targetHalf != 0;
    A.half_rtz = p->halfStoreRTZ != 0;
    A.samples = p->samples;
    A.samplesF = (float)p->samples;  // #define samplesFloat samples.0
    A.rcpSamplesF = 1.0f / A.samplesF;
    A.div2 = A.samplesF + 2.0f;
    A.intensity = p->intensity;
    A.jitter = p->jitter;
    A.frameSpeed = 0.01f / p->deltaTime;  // :25 (1. / 100.) / deltaTime
    A.resX = p->resolution[0];
    A.resY = p->resolution[1];
    A.tiled = tiled;
    A.vel_row0 = vs.row0; A.vel_rows = vs.rows;
    A.center_row0 = cs.row0; A.center_rows = cs.rows;  // (read by the row-tiled draw's NEAREST centre only)
    A.out_row0 = os.row0; A.out_rows = os.rows;
    A.center_is_source = p->center == -1;
    A.reach_mask = nullptr;
    return any;
}

int rfx_motion_blur(rfx_ctx *c, const rfx_motion_blur_params *p) {
    if (!c || !p) return RFX_EINVAL;
    RFX_ENTER(c);
    int rc = k6_validate(c, p, true);
    if (rc) return rc;
    if ((rc = ensure(c, RFX_TEX_MOTION_BLUR))) return rc;
    if (is_tiled(c) && (rc = ensure(c, RFX_TEX_BLUR_SOURCE))) return rc;
    K6Args A;
    if (!k6_args(c, p, A)) return RFX_OK;
    ProfScope prof(c, RFX_PROF_K6, c->stream);
    HIPCHK(c, rfx_launch_k6(A, c->stream));
    return RFX_OK;
}

// enqueue on the draw stream the reach reduction of the tile rows (row window honoured) into the first H words of c->hit_mask_dev
// (allocated here for `ranks` gathered copies); for rfx_motion_blur_gather in rfx_comm.hip too
int rfx_internal_blur_reach_enqueue(rfx_ctx *c, const rfx_motion_blur_params *p, int ranks) {
    RFX_ENTER(c);
    int rc = hit_mask_scratch(c, ranks);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->hit_mask_dev, 0, (size_t)c->H * sizeof(unsigned int), c->stream));
    K6Args A;
    if (!k6_args(c, p, A)) return RFX_OK;
    A.reach_mask = c->hit_mask_dev;
    ProfScope prof(c, RFX_PROF_K6_REACH, c->stream);
    HIPCHK(c, rfx_launch_k6_reach(A, c->stream));
    return RFX_OK;
}

int rfx_motion_blur_reach_mask(rfx_ctx *c, const rfx_motion_blur_params *p, unsigned int *row_mask, int rows) {
    if (!c || !p || !row_mask) return RFX_EINVAL;
    RFX_ENTER(c);
    int rc = k6_validate(c, p, false);
    if (rc) return rc;
    if (rows != c->H) return fail(c, RFX_EINVAL, "rfx_motion_blur_reach_mask: one word per frame row (rows == height)");
    if ((rc = rfx_internal_blur_reach_enqueue(c, p, 1))) return rc;
    return hit_mask_read_back(c, row_mask);
}

int rfx_motion_blur_stage(rfx_ctx *c, const rfx_motion_blur_params *p) {
    if (!c || !p) return RFX_EINVAL;
    RFX_ENTER(c);
    int rc = k6_validate(c, p, false);
    if (rc) return rc;
    if (!is_tiled(c)) return RFX_OK;  // the whole-frame draw reads the source itself
    if ((rc = ensure(c, RFX_TEX_BLUR_SOURCE))) return rc;
    const Slot &s = c->slots[p->source], &b = c->slots[RFX_TEX_BLUR_SOURCE];
    const size_t pitch = (size_t)c->W * 16;  // every source slot is read as RGBA32F; RFX_TEX_BLUR_SOURCE is held whole, as RGBA32F
    HIPCHK(c, hipMemcpyAsync(slot_row(b, c->tile_y0), slot_row(s, c->tile_y0), (size_t)c->tile_rows * pitch, hipMemcpyDeviceToDevice, c->stream));
    c->blur_armed = p->source;
    return RFX_OK;
}

// ---- K7: streamed frame export (include/rfx.h "streamed frame export"; the kernel is in k0_import.hip)
// the parameters alone: what rfx_export_bytes can judge without a context's state.  Returns nullptr when they are good.
static const char *export_params_error(const rfx_export_params *p) {
    const int s = p->source;
    if (s != RFX_TEX_FINAL && s != RFX_TEX_MOTION_BLUR && s != RFX_TEX_COMPOSE && s != RFX_TEX_TEMPORAL0 && s != RFX_TEX_DIRECT_LIGHT && s != RFX_TEX_EFFECT_INPUT)
        return "source must be FINAL, MOTION_BLUR, COMPOSE, TEMPORAL0, DIRECT_LIGHT or EFFECT_INPUT";
    if (p->format != RFX_EXPORT_F32 && p->format != RFX_EXPORT_F16 && p->format != RFX_EXPORT_U8_SRGB) return "format must be RFX_EXPORT_F32, _F16 or _U8_SRGB";
    if (p->channels != 3 && p->channels != 4) return "channels must be 3 or 4";
    if (p->format == RFX_EXPORT_U8_SRGB) {
        if (p->tonemap != 0 && p->tonemap != 1) return "tonemap must be 0 (linear) or 1 (ACES filmic)";
        if (!(p->exposure >= 0.0f) || !(p->exposure <= 3.402823466e38f)) return "exposure must be finite and >= 0";
    } else {
        if (p->tonemap != 0) return "tonemap belongs to RFX_EXPORT_U8_SRGB: must be 0 with another format";
        if (p->exposure != 0.0f && p->exposure != 1.0f) return "exposure belongs to RFX_EXPORT_U8_SRGB: must be 0 or 1 with another format";
    }
    return nullptr;
}

size_t rfx_export_bytes(const rfx_ctx *c, const rfx_export_params *p) {
    rfx_export_plan t;
    if (!c || !p || export_params_error(p) || !rfx_export_plan_for(c->tile_rows * c->W, p->format, p->channels, &t)) return 0;
    return (size_t)t.bytes;
}

// a device buffer of at least `want` bytes in *buf (capacity *cap), replaced when it is too small: the caller knows it idle
static int grow_idle(rfx_ctx *c, void **buf, size_t *cap, size_t want, const char *what) {
    if (*cap >= want) return RFX_OK;
    if (*buf) hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(buf, want);
    if (e != hipSuccess) return fail(c, RFX_ENOMEM, what, e);
    *cap = want;
    return RFX_OK;
}

// png_filter < 0: the plain export (K7's bytes cross PCIe); 0..4: rfx_stage_png — K7 as ever, then K8 on the download stream and its result buffer.
// exr: rfx_stage_exr — the same with K8's EXR pre-transform behind K7's F16 stream.
static int export_enqueue(rfx_ctx *c, const rfx_export_params *p, void *host, size_t bytes, int *ticket, const char *fn, int png_filter = -1, bool exr = false, unsigned flags = 0) {
    if (!c || !p || !host) return RFX_EINVAL;
    RFX_ENTER(c);
    if (const char *bad = export_params_error(p)) return fail_in(c, RFX_EINVAL, fn, bad);
    rfx_export_plan t;
    if (!rfx_export_plan_for(c->tile_rows * c->W, p->format, p->channels, &t)) return fail_in(c, RFX_EINVAL, fn, "bad format or channel count");
    const bool png = png_filter >= 0;
    if (flags & ~RFX_ENCODE_MATCHES) return fail_in(c, RFX_EINVAL, fn, "flags holds a bit other than RFX_ENCODE_MATCHES");
    rfx_png_plan g = {};
    rfx_exr_plan x = {};
    if (png) {
        if (p->format != RFX_EXPORT_U8_SRGB) return fail_in(c, RFX_EINVAL, fn, "format must be RFX_EXPORT_U8_SRGB");
        if (png_filter > 4) return fail_in(c, RFX_EINVAL, fn, "filter must be 0 (adaptive) or 1..4 (None, Sub, Up, Paeth)");
        if (!rfx_png_plan_for(c->tile_rows, c->W, p->channels, &g)) return fail_in(c, RFX_EINVAL, fn, "bad channel count");
        if (bytes != (size_t)g.bound) return fail_in(c, RFX_EINVAL, fn, "bytes != rfx_png_bound(ctx, params)");
    } else if (exr) {
        if (p->format != RFX_EXPORT_F16) return fail_in(c, RFX_EINVAL, fn, "format must be RFX_EXPORT_F16");
        if (!rfx_exr_plan_for(c->tile_rows, c->W, p->channels, &x)) return fail_in(c, RFX_EINVAL, fn, "bad channel count");
        if (bytes != (size_t)x.bound) return fail_in(c, RFX_EINVAL, fn, "bytes != rfx_exr_bound(ctx, params)");
    } else if (bytes != (size_t)t.bytes) return fail_in(c, RFX_EINVAL, fn, "bytes != rfx_export_bytes(ctx, params)");
    const size_t stream_bytes = (size_t)t.bytes;  // K7's output
    // rfx_motion_blur's rule: a host-filled plane must have been uploaded (staged, bound); a slot a draw writes must at least exist
    const Slot &s = c->slots[p->source];
    if (!slot_filled(c, p->source)) return fail_in(c, RFX_ESTATE, fn, "the source slot holds nothing yet (upload it or draw into it first)");
    if (!c->download_stream) {
        hipError_t e = hipStreamCreateWithFlags(&c->download_stream, hipStreamNonBlocking);
        for (int b = 0; b < 2; b++) {
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_export_encoded[b], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_export_copied[b], hipEventDisableTiming);
        }
        if (e != hipSuccess) return fail(c, RFX_EDEVICE, "rfx_stage_export: stream/event creation", e);
    }
    const unsigned int n = c->exports;
    const int b = (int)(n & 1u);
    if (n >= 2) {
        // host-side back pressure (rfx_stage_flip's rule): export n - 2 — the last user of this staging buffer and, with two alternating host
        // buffers, of `host` — has completed before this call returns
        HIPCHK(c, hipEventSynchronize(c->ev_export_copied[b]));
        // ... and the order on the device: this encode overwrites the buffer that copy read
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_export_copied[b], 0));
    }
    int rc;
    // (idle: its last copy has completed)
    if ((rc = grow_idle(c, &c->export_buf[b], &c->export_cap[b], stream_bytes, "rfx_stage_export: hipMalloc(staging buffer)"))) return rc;
    // (idle by the same event: K8 and its copy ran behind that buffer's last encode)
    if (png && (rc = grow_idle(c, &c->png_buf[b], &c->png_cap[b], (size_t)g.device_bytes, "rfx_stage_png: hipMalloc(PNG buffer)"))) return rc;
    if (exr && (rc = grow_idle(c, &c->png_buf[b], &c->png_cap[b], (size_t)x.device_bytes, "rfx_stage_exr: hipMalloc(EXR buffer)"))) return rc;
    K7Args A;
    A.src = (const uint4 *)slot_row(s, c->tile_y0);
    A.dst = c->export_buf[b];
    A.groups = t.groups;
    A.tail_start = t.tail_start;
    A.tail_pixels = t.tail_pixels;
    A.exposure = p->exposure;
    {
        ProfScope prof(c, RFX_PROF_K7, c->stream);
        HIPCHK(c, rfx_launch_k7(A, t.blocks, p->format, p->channels, p->tonemap, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev_export_encoded[b], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->download_stream, c->ev_export_encoded[b], 0));
    const void *from = c->export_buf[b];
    if (png) {
        unsigned char *base = (unsigned char *)c->png_buf[b];
        K8Args E;
        E.src = (const unsigned char *)c->export_buf[b];
        E.result = base;
        E.slots = base + g.slots_at;
        E.meta = (unsigned *)(base + g.meta_at);
        E.offsets = (unsigned long long *)(base + g.offsets_at);
        E.fragment_cap = g.bound - 32ull;
        E.rows = g.rows; E.rowbytes = g.rowbytes; E.bpp = p->channels; E.filter = png_filter;
        E.slot_stride = g.slot_stride;
        ProfScope prof(c, RFX_PROF_K8, c->download_stream);
        HIPCHK(c, rfx_launch_k8(E, c->download_stream, (flags & RFX_ENCODE_MATCHES) != 0));
        from = base;
    } else if (exr) {
        unsigned char *base = (unsigned char *)c->png_buf[b];
        K8ExrArgs E;
        E.src = (const unsigned short *)c->export_buf[b];
        E.result = base;
        E.slots = base + x.slots_at;
        E.planes = base + x.planes_at;
        E.meta = (unsigned *)(base + x.meta_at);
        E.offsets = (unsigned long long *)(base + x.offsets_at);
        E.fragment_cap = x.bound - 32ull;
        E.rows = x.rows; E.width = x.width; E.channels = x.channels;
        E.first_y = c->H - c->tile_y0 - c->tile_rows;
        E.slot_stride = x.slot_stride; E.plane_stride = x.plane_stride;
        ProfScope prof(c, RFX_PROF_K8, c->download_stream);
        HIPCHK(c, rfx_launch_k8_exr(E, c->download_stream, (flags & RFX_ENCODE_MATCHES) != 0));
        from = base;
    }
    // (the whole bound crosses for a PNG or an EXR fragment: copying only fragment_bytes would need the host to wait for the header first — rfx.h)
    HIPCHK(c, hipMemcpyAsync(host, from, bytes, hipMemcpyDeviceToHost, c->download_stream));
    HIPCHK(c, hipEventRecord(c->ev_export_copied[b], c->download_stream));
    c->exports = n + 1;
    if (ticket) *ticket = (int)(n + 1);
    return RFX_OK;
}

int rfx_stage_export(rfx_ctx *c, const rfx_export_params *p, void *host, size_t bytes, int *ticket) {
    if (!ticket) return RFX_EINVAL;
    return export_enqueue(c, p, host, bytes, ticket, "rfx_stage_export");
}

int rfx_export_wait(rfx_ctx *c, int ticket) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    if (ticket < 1 || (unsigned int)ticket > c->exports) return fail(c, RFX_EINVAL, "rfx_export_wait: no such ticket");
    // every export but the last two retired when a later rfx_stage_export returned (its back pressure)
    if ((unsigned int)ticket + 2 <= c->exports) return RFX_OK;
    HIPCHK(c, hipEventSynchronize(c->ev_export_copied[(ticket - 1) & 1]));
    return RFX_OK;
}

int rfx_export(rfx_ctx *c, const rfx_export_params *p, void *host, size_t bytes) {
    int ticket = 0;
    const int rc = export_enqueue(c, p, host, bytes, &ticket, "rfx_export");
    return rc ? rc : rfx_export_wait(c, ticket);
}

// ---- K8: the same export as a finished PNG fragment (include/rfx.h "PNG fragments"; the kernels are in k8_png.h)
size_t rfx_png_bound(const rfx_ctx *c, const rfx_export_params *p) {
    rfx_png_plan g;
    if (!c || !p || export_params_error(p) || p->format != RFX_EXPORT_U8_SRGB || !rfx_png_plan_for(c->tile_rows, c->W, p->channels, &g)) return 0;
    return (size_t)g.bound;
}

int rfx_stage_png(rfx_ctx *c, const rfx_export_params *p, int filter, void *host, size_t bytes, int *ticket) {
    if (!ticket) return RFX_EINVAL;
    if (filter < 0 || filter > 4) return c ? fail_in(c, RFX_EINVAL, "rfx_stage_png", "filter must be 0 (adaptive) or 1..4 (None, Sub, Up, Paeth)") : RFX_EINVAL;
    return export_enqueue(c, p, host, bytes, ticket, "rfx_stage_png", filter);
}

int rfx_png(rfx_ctx *c, const rfx_export_params *p, int filter, void *host, size_t bytes) {
    if (filter < 0 || filter > 4) return c ? fail_in(c, RFX_EINVAL, "rfx_png", "filter must be 0 (adaptive) or 1..4 (None, Sub, Up, Paeth)") : RFX_EINVAL;
    int ticket = 0;
    const int rc = export_enqueue(c, p, host, bytes, &ticket, "rfx_png", filter);
    return rc ? rc : rfx_export_wait(c, ticket);
}

// ---- K8: ... and as a finished EXR fragment, ZIPS chunks (include/rfx.h "EXR fragments"; the kernels are in k8_exr.h)
size_t rfx_exr_bound(const rfx_ctx *c, const rfx_export_params *p) {
    rfx_exr_plan x;
    if (!c || !p || export_params_error(p) || p->format != RFX_EXPORT_F16 || !rfx_exr_plan_for(c->tile_rows, c->W, p->channels, &x)) return 0;
    return (size_t)x.bound;
}

int rfx_stage_exr(rfx_ctx *c, const rfx_export_params *p, void *host, size_t bytes, int *ticket) {
    if (!ticket) return RFX_EINVAL;
    return export_enqueue(c, p, host, bytes, ticket, "rfx_stage_exr", -1, true);
}

int rfx_exr(rfx_ctx *c, const rfx_export_params *p, void *host, size_t bytes) {
    int ticket = 0;
    const int rc = export_enqueue(c, p, host, bytes, &ticket, "rfx_exr", -1, true);
    return rc ? rc : rfx_export_wait(c, ticket);
}

// ---- K8 with run-length matches (include/rfx.h "Match form"; the kernels are in k8_match.h): flags = 0 is the call without _ex
int rfx_stage_png_ex(rfx_ctx *c, const rfx_export_params *p, int filter, unsigned flags, void *host, size_t bytes, int *ticket) {
    if (!ticket) return RFX_EINVAL;
    if (filter < 0 || filter > 4) return c ? fail_in(c, RFX_EINVAL, "rfx_stage_png_ex", "filter must be 0 (adaptive) or 1..4 (None, Sub, Up, Paeth)") : RFX_EINVAL;
    return export_enqueue(c, p, host, bytes, ticket, "rfx_stage_png_ex", filter, false, flags);
}

int rfx_png_ex(rfx_ctx *c, const rfx_export_params *p, int filter, unsigned flags, void *host, size_t bytes) {
    if (filter < 0 || filter > 4) return c ? fail_in(c, RFX_EINVAL, "rfx_png_ex", "filter must be 0 (adaptive) or 1..4 (None, Sub, Up, Paeth)") : RFX_EINVAL;
    int ticket = 0;
    const int rc = export_enqueue(c, p, host, bytes, &ticket, "rfx_png_ex", filter, false, flags);
    return rc ? rc : rfx_export_wait(c, ticket);
}

int rfx_stage_exr_ex(rfx_ctx *c, const rfx_export_params *p, unsigned flags, void *host, size_t bytes, int *ticket) {
    if (!ticket) return RFX_EINVAL;
    return export_enqueue(c, p, host, bytes, ticket, "rfx_stage_exr_ex", -1, true, flags);
}

int rfx_exr_ex(rfx_ctx *c, const rfx_export_params *p, unsigned flags, void *host, size_t bytes) {
    int ticket = 0;
    const int rc = export_enqueue(c, p, host, bytes, &ticket, "rfx_exr_ex", -1, true, flags);
    return rc ? rc : rfx_export_wait(c, ticket);
}

int rfx_sync(rfx_ctx *c) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->download_stream) HIPCHK(c, hipStreamSynchronize(c->download_stream));  // staged exports: their bytes are in the host buffers
    return RFX_OK;
}

int rfx_time_begin(rfx_ctx *c) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    return RFX_OK;
}
int rfx_time_end(rfx_ctx *c, float *elapsed_ms) {
    if (!c || !elapsed_ms) return RFX_EINVAL;
    RFX_ENTER(c);
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(elapsed_ms, c->ev0, c->ev1));
    return RFX_OK;
}

int rfx_profile(rfx_ctx *c, int enable) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    if (enable) {  // events of an earlier run may still be pending: let them execute before they are recorded again
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->prep_stream) HIPCHK(c, hipStreamSynchronize(c->prep_stream));
        if (c->download_stream) HIPCHK(c, hipStreamSynchronize(c->download_stream));  // (K8's pairs are recorded there)
        prof_recycle(c);
    }
    c->profiling = enable != 0;
    return RFX_OK;
}
int rfx_profile_read(rfx_ctx *c, float *ms_sum, int *launches) { return rfx_profile_read_n(c, ms_sum, launches, RFX_PROF_COUNT); }
int rfx_profile_read_n(rfx_ctx *c, float *ms_sum, int *launches, int entries) {
    if (!c || entries < 0) return RFX_EINVAL;
    RFX_ENTER(c);
    // every pair is waited for on its own: the draws may have been enqueued on a stream that is no longer the current one (rfx_set_stream between
    // the draws and this call), which a synchronisation of today's streams would not cover; a pair that cannot be read is skipped, not fatal
    float ms[RFX_PROF_COUNT_ALL] = {0};
    int n[RFX_PROF_COUNT_ALL] = {0};
    for (const rfx_ctx::ProfRec &r : c->prof_recs) {
        float t = 0.0f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) {
            (void)hipGetLastError();
            continue;
        }
        ms[r.kind] += t;
        n[r.kind]++;
    }
    for (int i = 0; i < RFX_PROF_COUNT_ALL && i < entries; i++) {
        if (ms_sum) ms_sum[i] = ms[i];
        if (launches) launches[i] = n[i];
    }
    return RFX_OK;
}

unsigned int rfx_halo_violations(rfx_ctx *c) {
    unsigned int v = 0;
    if (!c) return 0;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    hipMemcpy(&v, c->halo_violations, sizeof v, hipMemcpyDeviceToHost);
    return v;
}

}  // extern "C"
