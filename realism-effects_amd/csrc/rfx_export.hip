// rfx_export.hip — the C ABI's streamed frame export (include/rfx.h "streamed frame export", "PNG fragments", "EXR fragments", "Match form"):
// K7 packs a slot on the draw stream, K8 encodes the packed stream on the download stream, the bytes cross PCIe behind them (the kernels are in
// k7_export.hip and the k8_*.h it includes)
#include "rfx_host.h"

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

// the filter of a PNG call, refused in the name of the entry point `fn` (a null context has nowhere to keep the text)
static int png_filter_check(rfx_ctx *c, const char *fn, int filter) {
    if (filter >= 0 && filter <= 4) return RFX_OK;
    return c ? fail_in(c, RFX_EINVAL, fn, "filter must be 0 (adaptive) or 1..4 (None, Sub, Up, Paeth)") : RFX_EINVAL;
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
    int rc;
    if (png) {
        if (p->format != RFX_EXPORT_U8_SRGB) return fail_in(c, RFX_EINVAL, fn, "format must be RFX_EXPORT_U8_SRGB");
        if ((rc = png_filter_check(c, fn, png_filter))) return rc;
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

extern "C" {

size_t rfx_export_bytes(const rfx_ctx *c, const rfx_export_params *p) {
    rfx_export_plan t;
    if (!c || !p || export_params_error(p) || !rfx_export_plan_for(c->tile_rows * c->W, p->format, p->channels, &t)) return 0;
    return (size_t)t.bytes;
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

// ---- device images (include/rfx.h "device images and stream ordering"): K7 on the draw stream, straight into the caller's buffer.  Nothing of
// the streamed export is touched: no ticket, no staging buffer, no download stream, no allocation, no wait
int rfx_export_device(rfx_ctx *c, const rfx_export_params *p, const rfx_device_image *dst) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    const char *fn = "rfx_export_device";
    if (!p) return fail_in(c, RFX_EINVAL, fn, "params is NULL");
    if (const char *bad = export_params_error(p)) return fail_in(c, RFX_EINVAL, fn, bad);
    if (!dst) return fail_in(c, RFX_EINVAL, fn, "dst is NULL");
    rfx_export_device_plan t;
    if (const char *bad = rfx_export_device_plan_for(c->W, c->tile_rows, p->format, p->channels, (unsigned long long)(uintptr_t)dst->data, dst->stride_x, dst->stride_y,
                                                     dst->stride_c, &t))
        return fail_in(c, RFX_EINVAL, fn, bad);
    const Slot &s = c->slots[p->source];
    if (!slot_filled(c, p->source)) return fail_in(c, RFX_ESTATE, fn, "the source slot holds nothing yet (upload it or draw into it first)");
    const uint4 *src = (const uint4 *)slot_row(s, c->tile_y0);
    ProfScope prof(c, RFX_PROF_K7, c->stream);
    if (t.form == RFX_EXPORT_FORM_TIGHT) {  // the staging buffer's own layout: rfx_export's kernel, on the caller's pointer
        K7Args A;
        A.src = src;
        A.dst = dst->data;
        A.groups = t.flat.groups;
        A.tail_start = t.flat.tail_start;
        A.tail_pixels = t.flat.tail_pixels;
        A.exposure = p->exposure;
        HIPCHK(c, rfx_launch_k7(A, t.flat.blocks, p->format, p->channels, p->tonemap, c->stream));
        return RFX_OK;
    }
    K7StridedArgs A;
    A.src = src;
    A.dst = dst->data;
    A.sx = dst->stride_x; A.sy = dst->stride_y; A.sc = dst->stride_c;
    A.W = c->W; A.rows = c->tile_rows;
    A.groups_x = t.groups_x; A.tail_x = t.tail_x; A.tail_pixels = t.tail_pixels; A.lanes_x = t.lanes_x;
    A.form = t.form;
    A.exposure = p->exposure;
    HIPCHK(c, rfx_launch_k7_strided(A, t.grid_x, t.grid_y, p->format, p->channels, p->tonemap, c->stream));
    return RFX_OK;
}

// ---- K8: the same export as a finished PNG fragment (include/rfx.h "PNG fragments"; the kernels are in k8_png.h)
size_t rfx_png_bound(const rfx_ctx *c, const rfx_export_params *p) {
    rfx_png_plan g;
    if (!c || !p || export_params_error(p) || p->format != RFX_EXPORT_U8_SRGB || !rfx_png_plan_for(c->tile_rows, c->W, p->channels, &g)) return 0;
    return (size_t)g.bound;
}

int rfx_stage_png(rfx_ctx *c, const rfx_export_params *p, int filter, void *host, size_t bytes, int *ticket) {
    if (!ticket) return RFX_EINVAL;
    if (const int rc = png_filter_check(c, "rfx_stage_png", filter)) return rc;
    return export_enqueue(c, p, host, bytes, ticket, "rfx_stage_png", filter);
}

int rfx_png(rfx_ctx *c, const rfx_export_params *p, int filter, void *host, size_t bytes) {
    if (const int rc = png_filter_check(c, "rfx_png", filter)) return rc;
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

// ---- K8 with run-length matches (include/rfx.h "Match form"; the scanline kernels' <true> instantiations, the token rule is in k8_coder.h): flags = 0 is the call without _ex
int rfx_stage_png_ex(rfx_ctx *c, const rfx_export_params *p, int filter, unsigned flags, void *host, size_t bytes, int *ticket) {
    if (!ticket) return RFX_EINVAL;
    if (const int rc = png_filter_check(c, "rfx_stage_png_ex", filter)) return rc;
    return export_enqueue(c, p, host, bytes, ticket, "rfx_stage_png_ex", filter, false, flags);
}

int rfx_png_ex(rfx_ctx *c, const rfx_export_params *p, int filter, unsigned flags, void *host, size_t bytes) {
    if (const int rc = png_filter_check(c, "rfx_png_ex", filter)) return rc;
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

}  // extern "C"
