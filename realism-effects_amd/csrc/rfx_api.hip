// rfx_api.hip — the C ABI of librfx_hip.so (include/rfx.h): the context's life cycle, its texture slots, timing and profiling.  The other areas of
// the ABI: rfx_stage.hip (streamed uploads, the flip), rfx_exr_import.hip (streamed EXR frames), rfx_env.hip (the importer's packers, the
// environment), rfx_draw.hip (K1–K5), rfx_blur.hip (K6), rfx_export.hip (K7 / K8), rfx_comm.hip and rfx_peer.hip (the exchanges of a row-tiled run).
// Host side only; the kernels live in the k*.hip files.
#include <stdlib.h>
#include <string>
#include "rfx_host.h"

thread_local std::string g_create_err;

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
    for (hipEvent_t e : c->ev_order)
        if (e) hipEventDestroy(e);
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
    for (void *p : {c->env_stage, c->env_cube, c->env_k10})
        if (p) hipFree(p);
    if (c->ev_env_copied) hipEventDestroy(c->ev_env_copied);
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

// pinned host memory for the streamed calls (rfx_stage.hip, rfx_export.hip)
void *rfx_host_alloc(size_t bytes) {
    void *p = nullptr;
    return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void rfx_host_free(void *p) {
    if (p) hipHostFree(p);
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
