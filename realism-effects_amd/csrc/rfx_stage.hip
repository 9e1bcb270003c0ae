// rfx_stage.hip — the C ABI's streamed uploads (include/rfx.h "streaming dumps", "streamed AOV frames"): the next frame's planes cross PCIe on their
// own stream into back buffers while the current frame is drawn; rfx_stage_flip publishes them.  The staging helpers rfx_exr_import.hip shares are
// declared in rfx_host.h.
#include "rfx_host.h"

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

// the slots a plan writes: depth always, the packed ones where their planes are given
static const int plan_ids[4] = {RFX_TEX_DEPTH, RFX_TEX_GBUFFER, RFX_TEX_VELOCITY, RFX_TEX_DIRECT_LIGHT};
static bool plan_writes(const rfx_aov_plan &t, int k) { return k == 0 || (k == 1 ? t.write_gbuffer : k == 2 ? t.write_velocity : t.write_direct) != 0; }

int stage_plan_begin(rfx_ctx *c, const rfx_aov_plan &t, const char *fn) {
    int rc;
    for (int k = 0; k < 4; k++) {  // every check before anything is enqueued
        if (!plan_writes(t, k)) continue;
        if ((rc = ensure(c, plan_ids[k]))) return rc;
        if (!c->slots[plan_ids[k]].owned) return fail_in(c, RFX_ESTATE, fn, "a slot to be written is bound to an external buffer");
    }
    if ((rc = stage_streams(c))) return rc;
    for (int k = 0; k < 4; k++)
        if (plan_writes(t, k) && (rc = stage_back(c, c->slots[plan_ids[k]]))) return rc;
    return RFX_OK;
}
void stage_plan_end(rfx_ctx *c, const rfx_aov_plan &t) {
    for (int k = 0; k < 4; k++)
        if (plan_writes(t, k)) c->slots[plan_ids[k]].back_filled = true;
}

int grow_stage_area(rfx_ctx *c, void **area, size_t *cap, size_t need, const char *what) {
    if (*cap >= need) return RFX_OK;
    if (*area) HIPCHK(c, hipStreamSynchronize(c->upload_stream));
    return grow_idle(c, area, cap, need, what);
}

// the conventions in use as the pack kernels read them: the setting as it stands at this call, with a segment's place in the frame
static K0AovConv aov_conv_block(const rfx_ctx *c, int seg_row0) {
    const rfx_aov_conventions &q = c->aov_conv;
    K0AovConv v = {};
    v.depth_kind = q.depth_kind; v.velocity_kind = q.velocity_kind; v.normal_space = q.normal_space; v.perspective = q.perspective;
    v.W = c->W; v.H = c->H; v.row0 = seg_row0;
    v.has_background = q.has_background_position != 0;
    for (int i = 0; i < 3; i++) v.background[i] = q.background_position[i];
    v.scale[0] = q.velocity_scale[0]; v.scale[1] = q.velocity_scale[1];
    v.near_ = q.near_; v.far_ = q.far_;
    memcpy(v.VM, q.velocityMatrix, sizeof v.VM); memcpy(v.PVM, q.prevVelocityMatrix, sizeof v.PVM);
    memcpy(v.P, q.projectionMatrix, sizeof v.P); memcpy(v.Pi, q.projectionMatrixInverse, sizeof v.Pi); memcpy(v.C, q.cameraMatrixWorld, sizeof v.C);
    return v;
}
hipError_t aov_pack_segment(rfx_ctx *c, const rfx_aov_plan &t, const rfx_aov_segment &g, K0AovArgs A) {
    const auto first = [&](int id) { return slot_back_row(c->slots[id], g.row0); };
    A.depth = (float *)first(RFX_TEX_DEPTH);
    if (g.full && t.write_gbuffer) A.gbuffer = (uint4 *)first(RFX_TEX_GBUFFER);
    if (g.full && t.write_velocity) A.velocity = (uint4 *)first(RFX_TEX_VELOCITY);
    if (g.full && t.write_direct) A.direct = (uint4 *)first(RFX_TEX_DIRECT_LIGHT);
    A.groups = g.groups; A.tail_start = g.tail_start; A.tail_pixels = g.tail_pixels;
    if (!c->aov_conv_on) return rfx_launch_k0_aov(A, g.blocks, c->upload_stream);
    const K0AovConv v = aov_conv_block(c, g.row0);
    return rfx_launch_k0_aov(A, g.blocks, c->upload_stream, &v);
}
int aov_depth_kind(const rfx_ctx *c) { return c->aov_conv_on ? c->aov_conv.depth_kind : RFX_AOV_DEPTH_FRAGCOORD; }
int aov_velocity_kind(const rfx_ctx *c) { return c->aov_conv_on ? c->aov_conv.velocity_kind : RFX_AOV_VELOCITY_UV; }

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
    return rfx_aov_plan_conv_for(c->W, c->H, g.row0, g.rows, type, channels, row0, rows, aov_depth_kind(c), aov_velocity_kind(c), t);
}

extern "C" {

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
    int rc = stage_plan_begin(c, t, "rfx_stage_aov");
    if (rc) return rc;
    if ((rc = grow_stage_area(c, &c->aov_stage, &c->aov_stage_cap, (size_t)t.stage_bytes, "rfx_stage_aov: hipMalloc(staging area)"))) return rc;
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
    stage_plan_end(c, t);
    return RFX_OK;
}

// ---- device planes (include/rfx.h): rfx_stage_aov without the copies — the pack kernels read the producer's own memory
int rfx_stage_aov_device(rfx_ctx *c, const rfx_aov_device_frame *f, int row0, int rows, void *producer_stream) {
    if (!c || !f) return RFX_EINVAL;
    RFX_ENTER(c);
    const char *fn = "rfx_stage_aov_device";
    if (producer_stream) return fail_in(c, RFX_EUNSUPPORTED, fn, "a producer stream is not taken yet: make the planes complete before the call and pass NULL");
    static_assert(sizeof(rfx_aov_device_frame) == RFX_AOV_PLANES * sizeof(rfx_device_plane), "rfx_aov_device_frame is eight planes");
    const rfx_device_plane *planes = &f->diffuse;  // eight rfx_device_plane in RFX_AOV_* order
    int type[RFX_AOV_PLANES], channels[RFX_AOV_PLANES];
    unsigned long long addr[RFX_AOV_PLANES];
    long long sx[RFX_AOV_PLANES], sy[RFX_AOV_PLANES], sc[RFX_AOV_PLANES];
    for (int i = 0; i < RFX_AOV_PLANES; i++) {
        const rfx_device_plane &p = planes[i];
        type[i] = p.type;
        channels[i] = p.data ? p.channels : 0;
        if (p.data && p.channels <= 0) return fail_in(c, RFX_EINVAL, fn, "a plane's channel count");
        addr[i] = (unsigned long long)(uintptr_t)p.data;
        sx[i] = p.stride_x; sy[i] = p.stride_y; sc[i] = p.stride_c;
    }
    const Slot &held = c->slots[RFX_TEX_GBUFFER];  // (VELOCITY and DIRECT_LIGHT hold the same rows)
    rfx_aov_device_plan t;
    if (const char *bad = rfx_aov_device_plan_for(c->W, c->H, held.row0, held.rows, type, channels, addr, sx, sy, sc, row0, rows, aov_depth_kind(c), aov_velocity_kind(c), &t))
        return fail_in(c, RFX_EINVAL, fn, bad);
    int rc = stage_plan_begin(c, t.rows, fn);
    if (rc) return rc;
    // rfx_stage_upload's order: the back buffers were the front buffers until the last flip
    HIPCHK(c, hipStreamWaitEvent(c->upload_stream, c->ev_frame_done, 0));
    unsigned int half_mask = 0, layouts = 0;
    for (int i = 0; i < RFX_AOV_PLANES; i++) {
        if (channels[i] && type[i] == RFX_PLANE_F16) half_mask |= 1u << i;
        layouts |= (unsigned int)t.layout[i] << (2 * i);
    }
    for (int k = 0; k < t.rows.nseg; k++) {
        const rfx_aov_segment &g = t.rows.seg[k];
        // the segment's first row of every plane it reads
        const void *first[RFX_AOV_PLANES] = {};
        for (int i = 0; i < RFX_AOV_PLANES; i++)
            if (g.offset[i] != ~0ull) first[i] = (const char *)planes[i].data + t.seg_offset[k][i] * (long long)t.rows.elem_bytes[i];
        if (t.flat[k]) {  // the staging area's own layout: rfx_stage_aov's kernel, on the caller's pointers
            K0AovArgs A = {};
            for (int i = 0; i < RFX_AOV_PLANES; i++) A.plane[i] = first[i];
            A.half_mask = half_mask;
            A.diffuse_ch = f->diffuse.channels; A.direct_ch = f->direct.channels;
            HIPCHK(c, aov_pack_segment(c, t.rows, g, A));
            continue;
        }
        K0AovStridedArgs A = {};
        for (int i = 0; i < RFX_AOV_PLANES; i++) A.plane[i] = {first[i], sx[i], sy[i], channels[i] > 1 ? sc[i] : 0};
        A.half_mask = half_mask; A.layouts = layouts;
        A.diffuse_ch = f->diffuse.channels; A.direct_ch = f->direct.channels;
        A.depth = (float *)slot_back_row(c->slots[RFX_TEX_DEPTH], g.row0);
        if (g.full && t.rows.write_gbuffer) A.gbuffer = (uint4 *)slot_back_row(c->slots[RFX_TEX_GBUFFER], g.row0);
        if (g.full && t.rows.write_velocity) A.velocity = (uint4 *)slot_back_row(c->slots[RFX_TEX_VELOCITY], g.row0);
        if (g.full && t.rows.write_direct) A.direct = (uint4 *)slot_back_row(c->slots[RFX_TEX_DIRECT_LIGHT], g.row0);
        A.W = c->W; A.rows = g.rows;
        A.groups_x = t.groups_x; A.tail_x = t.tail_x; A.tail_pixels = t.tail_pixels; A.lanes_x = t.lanes_x;
        if (c->aov_conv_on) {
            const K0AovConv v = aov_conv_block(c, g.row0);
            HIPCHK(c, rfx_launch_k0_aov_strided(A, t.grid_x, t.grid_y[k], c->upload_stream, &v));
        } else HIPCHK(c, rfx_launch_k0_aov_strided(A, t.grid_x, t.grid_y[k], c->upload_stream));
    }
    stage_plan_end(c, t.rows);
    return RFX_OK;
}

// ---- stream ordering (include/rfx.h "device images and stream ordering"): a queue of the context against a caller's stream, one event record
// and one stream wait, no host wait.  -> the queue's stream, the two events in place; an RFX_* code in *rc otherwise
static hipStream_t order_queue(rfx_ctx *c, int queue, void *hip_stream, const char *fn, int *rc) {
    *rc = RFX_OK;
    if (queue != RFX_QUEUE_DRAW && queue != RFX_QUEUE_UPLOAD) { *rc = fail_in(c, RFX_EINVAL, fn, "queue must be RFX_QUEUE_DRAW or RFX_QUEUE_UPLOAD"); return nullptr; }
    if (!hip_stream) { *rc = fail_in(c, RFX_EINVAL, fn, "hip_stream is NULL (the legacy default stream cannot be named: create a stream)"); return nullptr; }
    for (hipEvent_t &e : c->ev_order) {
        if (e) continue;
        const hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (err != hipSuccess) { e = nullptr; *rc = fail(c, RFX_EDEVICE, "rfx_queue_wait_stream / rfx_stream_wait_queue: event creation", err); return nullptr; }
    }
    if (queue == RFX_QUEUE_DRAW) return c->stream;
    if ((*rc = stage_streams(c))) return nullptr;
    return c->upload_stream;
}
int rfx_queue_wait_stream(rfx_ctx *c, int queue, void *hip_stream) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    int rc;
    hipStream_t q = order_queue(c, queue, hip_stream, "rfx_queue_wait_stream", &rc);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_order[0], (hipStream_t)hip_stream));
    HIPCHK(c, hipStreamWaitEvent(q, c->ev_order[0], 0));
    return RFX_OK;
}
int rfx_stream_wait_queue(rfx_ctx *c, int queue, void *hip_stream) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    int rc;
    hipStream_t q = order_queue(c, queue, hip_stream, "rfx_stream_wait_queue", &rc);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_order[1], q));
    HIPCHK(c, hipStreamWaitEvent((hipStream_t)hip_stream, c->ev_order[1], 0));
    return RFX_OK;
}

int rfx_set_aov_conventions(rfx_ctx *c, const rfx_aov_conventions *q) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    const char *fn = "rfx_set_aov_conventions";
    if (!q) { c->aov_conv_on = false; return RFX_OK; }
    if (q->depth_kind < 0 || q->depth_kind > RFX_AOV_DEPTH_POSITION) return fail_in(c, RFX_EINVAL, fn, "an unknown depth_kind");
    if (q->velocity_kind < 0 || q->velocity_kind > RFX_AOV_VELOCITY_CAMERAS) return fail_in(c, RFX_EINVAL, fn, "an unknown velocity_kind");
    if (q->normal_space < 0 || q->normal_space > RFX_AOV_NORMAL_VIEW) return fail_in(c, RFX_EINVAL, fn, "an unknown normal_space");
    if (q->velocity_kind == RFX_AOV_VELOCITY_SCALED && !(isfinite(q->velocity_scale[0]) && isfinite(q->velocity_scale[1])))
        return fail_in(c, RFX_EINVAL, fn, "a non-finite velocity_scale");
    if (q->depth_kind == RFX_AOV_DEPTH_VIEW_Z) {
        const float *P = q->projectionMatrix;  // P[c][r] = P[4 c + r]
        if (!(P[2] == 0.0f && P[3] == 0.0f && P[6] == 0.0f && P[7] == 0.0f))
            return fail_in(c, RFX_EINVAL, fn, "RFX_AOV_DEPTH_VIEW_Z needs projectionMatrix[0][2], [0][3], [1][2] and [1][3] to be 0: clip z and w must depend on view z alone");
    }
    if (q->depth_kind == RFX_AOV_DEPTH_FRAGCOORD && q->velocity_kind == RFX_AOV_VELOCITY_CAMERAS && !(isfinite(q->near_) && isfinite(q->far_) && q->near_ < q->far_))
        return fail_in(c, RFX_EINVAL, fn, "near_ >= far_ (or a non-finite one) where the depth is turned back into view z");
    c->aov_conv = *q;
    // (all three kinds 0 is the default: the default kernels run and nothing else of the struct is read)
    c->aov_conv_on = q->depth_kind != 0 || q->velocity_kind != 0 || q->normal_space != 0;
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

}  // extern "C"
