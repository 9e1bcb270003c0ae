/*
 * rfx_napi.c — raw N-API addon (node_api.h, no node-gyp / C++ wrappers) that binds the C ABI of
 * librfx_hip.so (include/rfx.h) for the Node host in ../js.
 *
 * Every export is a 1:1 wrapper of one rfx_* entry point; TypedArrays are passed zero-copy
 * (napi_get_typedarray_info).  Pass parameter blocks are plain JS objects whose property names
 * are the reference's uniform / define names (see include/rfx.h for the mapping to the
 * reference files).  Errors become JS exceptions carrying rfx_last_error().
 *
 * All calls are made on the JS main thread; asynchrony comes from the HIP stream inside the
 * context (calls enqueue and return, `sync` blocks), not from JS threads — the same model as the
 * reference, whose draws are asynchronous on the GL command queue.
 */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/rfx.h"

#define NAPI_CALL(env, call)                                          \
    do {                                                              \
        napi_status s__ = (call);                                     \
        if (s__ != napi_ok) {                                         \
            napi_throw_error((env), NULL, "N-API call failed: " #call); \
            return NULL;                                              \
        }                                                             \
    } while (0)

static napi_value throw_rfx(napi_env env, rfx_ctx *c, const char *what, int rc) {
    char buf[640];
    snprintf(buf, sizeof buf, "%s failed (%d): %s", what, rc, rfx_last_error(c));
    napi_throw_error(env, NULL, buf);
    return NULL;
}

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
        napi_throw_type_error(env, NULL, "wrong number of arguments");
        return 0;
    }
    return 1;
}

static rfx_ctx *get_ctx(napi_env env, napi_value v) {
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
        napi_throw_type_error(env, NULL, "expected an rfx context handle");
        return NULL;
    }
    return (rfx_ctx *)p;
}

static int get_int(napi_env env, napi_value v, int32_t *out) {
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok) return 0;
    if (t == napi_boolean) { bool b; napi_get_value_bool(env, v, &b); *out = b ? 1 : 0; return 1; }
    if (t != napi_number) return 0;
    double d;
    napi_get_value_double(env, v, &d);
    *out = (int32_t)d;
    return 1;
}

/* obj[name] as double; missing/undefined -> default */
static double prop_num(napi_env env, napi_value obj, const char *name, double def) {
    napi_value v;
    napi_valuetype t;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok || napi_typeof(env, v, &t) != napi_ok) return def;
    if (t == napi_boolean) { bool b; napi_get_value_bool(env, v, &b); return b ? 1.0 : 0.0; }
    if (t != napi_number) return def;
    double d;
    napi_get_value_double(env, v, &d);
    return d;
}

/* obj[name] = Float32Array | Float64Array | Array of n numbers -> out[n] */
static int prop_floats(napi_env env, napi_value obj, const char *name, float *out, size_t n) {
    napi_value v;
    bool is_ta = false, is_arr = false;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
    napi_is_typedarray(env, v, &is_ta);
    if (is_ta) {
        napi_typedarray_type ty; size_t len; void *data;
        if (napi_get_typedarray_info(env, v, &ty, &len, &data, NULL, NULL) != napi_ok || len < n) return 0;
        if (ty == napi_float32_array) { memcpy(out, data, n * sizeof(float)); return 1; }
        if (ty == napi_float64_array) { for (size_t i = 0; i < n; i++) out[i] = (float)((double *)data)[i]; return 1; }
        return 0;
    }
    napi_is_array(env, v, &is_arr);
    if (!is_arr) return 0;
    for (size_t i = 0; i < n; i++) {
        napi_value e; double d;
        if (napi_get_element(env, v, (uint32_t)i, &e) != napi_ok || napi_get_value_double(env, e, &d) != napi_ok) return 0;
        out[i] = (float)d;
    }
    return 1;
}

static int prop_bool2(napi_env env, napi_value obj, const char *name, int32_t *out) {
    napi_value v, e;
    bool is_arr = false;
    out[0] = out[1] = 0;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
    napi_is_array(env, v, &is_arr);
    if (!is_arr) { int32_t x = 0; if (get_int(env, v, &x)) { out[0] = out[1] = x; return 1; } return 0; }
    for (uint32_t i = 0; i < 2; i++)
        if (napi_get_element(env, v, i, &e) == napi_ok) get_int(env, e, &out[i]);
    return 1;
}

/* camera object: the fields the reference passes read from three's camera */
static int read_camera(napi_env env, napi_value obj, const char *name, rfx_camera *c) {
    napi_value cam;
    napi_valuetype t;
    if (napi_get_named_property(env, obj, name, &cam) != napi_ok || napi_typeof(env, cam, &t) != napi_ok || t != napi_object) {
        napi_throw_type_error(env, NULL, "params.camera / params.prevCamera must be an object");
        return 0;
    }
    if (!prop_floats(env, cam, "projectionMatrix", c->projectionMatrix, 16) || !prop_floats(env, cam, "projectionMatrixInverse", c->projectionMatrixInverse, 16) ||
        !prop_floats(env, cam, "matrixWorld", c->matrixWorld, 16) || !prop_floats(env, cam, "matrixWorldInverse", c->matrixWorldInverse, 16) ||
        !prop_floats(env, cam, "position", c->position, 3)) {
        napi_throw_type_error(env, NULL, "camera needs projectionMatrix, projectionMatrixInverse, matrixWorld, matrixWorldInverse (16 numbers) and position (3)");
        return 0;
    }
    c->near_ = (float)prop_num(env, cam, "near", 0.1);
    c->far_ = (float)prop_num(env, cam, "far", 1000.0);
    c->isPerspective = (int32_t)prop_num(env, cam, "isPerspectiveCamera", 1.0);
    return 1;
}

static void destroy_ctx(napi_env env, void *data, void *hint) { (void)env; (void)hint; rfx_destroy((rfx_ctx *)data); }

/* create(device, width, height, tileY0, tileRows, haloRows) -> handle */
static napi_value n_create(napi_env env, napi_callback_info info) {
    napi_value a[6], out;
    int32_t v[6];
    if (!get_args(env, info, 6, a)) return NULL;
    for (int i = 0; i < 6; i++) if (!get_int(env, a[i], &v[i])) { napi_throw_type_error(env, NULL, "create: integers expected"); return NULL; }
    rfx_ctx *c = rfx_create(v[0], v[1], v[2], v[3], v[4], v[5]);
    if (!c) return throw_rfx(env, NULL, "rfx_create", RFX_EDEVICE);
    NAPI_CALL(env, napi_create_external(env, c, destroy_ctx, NULL, &out));
    return out;
}

static napi_value n_abi_version(napi_env env, napi_callback_info info) {
    (void)info;
    napi_value out;
    NAPI_CALL(env, napi_create_int32(env, rfx_abi_version(), &out));
    return out;
}

/* heldRows(ctx, tex) -> [row0, rows] */
static napi_value n_held_rows(napi_env env, napi_callback_info info) {
    napi_value a[2], arr, e;
    int32_t tex;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex)) return NULL;
    int r0 = 0, n = 0;
    int rc = rfx_tex_held_rows(c, (rfx_tex)tex, &r0, &n);
    if (rc) return throw_rfx(env, c, "rfx_tex_held_rows", rc);
    NAPI_CALL(env, napi_create_array_with_length(env, 2, &arr));
    napi_create_int32(env, r0, &e); napi_set_element(env, arr, 0, e);
    napi_create_int32(env, n, &e); napi_set_element(env, arr, 1, e);
    return arr;
}

/* ssgiTargetRows(ctx, resolutionScale) -> [row0, rows]: rfx_ssgi_target_rows */
static napi_value n_ssgi_target_rows(napi_env env, napi_callback_info info) {
    napi_value a[2], arr, e;
    double scale = 1.0;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    if (napi_get_value_double(env, a[1], &scale) != napi_ok) {
        napi_throw_type_error(env, NULL, "ssgiTargetRows: resolutionScale must be a number");
        return NULL;
    }
    int r0 = 0, n = 0;
    int rc = rfx_ssgi_target_rows(c, (float)scale, &r0, &n);
    if (rc) return throw_rfx(env, c, "rfx_ssgi_target_rows", rc);
    NAPI_CALL(env, napi_create_array_with_length(env, 2, &arr));
    napi_create_int32(env, r0, &e); napi_set_element(env, arr, 0, e);
    napi_create_int32(env, n, &e); napi_set_element(env, arr, 1, e);
    return arr;
}

/* upload(ctx, tex, typedArray, row0, rows) / download(ctx, tex, typedArray, row0, rows) */
static napi_value xfer(napi_env env, napi_callback_info info, int up) {
    napi_value a[5];
    int32_t tex, row0, rows;
    if (!get_args(env, info, 5, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex) || !get_int(env, a[3], &row0) || !get_int(env, a[4], &rows)) return NULL;
    bool is_ta = false;
    napi_is_typedarray(env, a[2], &is_ta);
    if (!is_ta) { napi_throw_type_error(env, NULL, "upload/download: TypedArray expected"); return NULL; }
    napi_typedarray_type ty; size_t len; void *data; napi_value ab; size_t off;
    NAPI_CALL(env, napi_get_typedarray_info(env, a[2], &ty, &len, &data, &ab, &off));
    static const size_t esz[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
    const size_t bytes = len * esz[ty];
    int width = 0;
    rfx_get_geometry(c, &width, NULL, NULL, NULL, NULL);
    if (tex == RFX_TEX_BLUE_NOISE) width = 128;
    const size_t need = (size_t)rows * (size_t)width * rfx_tex_texel_bytes((rfx_tex)tex);
    if (rows <= 0 || need == 0 || bytes != need) {
        napi_throw_range_error(env, NULL, "upload/download: TypedArray byte length != rows * width * texel bytes");
        return NULL;
    }
    int rc = up == 2 ? rfx_stage_upload(c, (rfx_tex)tex, data, row0, rows)
             : up ? rfx_upload(c, (rfx_tex)tex, data, row0, rows) : rfx_download(c, (rfx_tex)tex, data, row0, rows);
    if (rc) return throw_rfx(env, c, up == 2 ? "rfx_stage_upload" : up ? "rfx_upload" : "rfx_download", rc);
    return NULL;
}
/* stageUpload(ctx, tex, typedArray, row0, rows): asynchronous copy into the slot's back buffer (rfx.h "streaming dumps"); the array —
 * ideally a view of hostAlloc() memory — must stay alive and unchanged until the flip that publishes it has been synced */
static napi_value n_stage_upload(napi_env env, napi_callback_info info) { return xfer(env, info, 2); }
static napi_value n_stage_flip(napi_env env, napi_callback_info info) {
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    int rc = rfx_stage_flip(c);
    if (rc) return throw_rfx(env, c, "rfx_stage_flip", rc);
    return NULL;
}
static void host_free_cb(napi_env env, void *data, void *hint) { (void)env; (void)hint; rfx_host_free(data); }
/* hostAlloc(bytes) -> ArrayBuffer over pinned host memory (hipHostMalloc), freed when the buffer is collected */
static napi_value n_host_alloc(napi_env env, napi_callback_info info) {
    napi_value a[1], ab;
    double bytes = 0;
    if (!get_args(env, info, 1, a) || napi_get_value_double(env, a[0], &bytes) != napi_ok || bytes <= 0) {
        napi_throw_range_error(env, NULL, "hostAlloc: a positive byte count");
        return NULL;
    }
    void *p = rfx_host_alloc((size_t)bytes);
    if (!p) { napi_throw_error(env, NULL, "rfx_host_alloc failed"); return NULL; }
    if (napi_create_external_arraybuffer(env, p, (size_t)bytes, host_free_cb, NULL, &ab) != napi_ok) {
        rfx_host_free(p);
        napi_throw_error(env, NULL, "hostAlloc: napi_create_external_arraybuffer failed");
        return NULL;
    }
    return ab;
}
/* an AOV frame from {diffuse, normal, roughness, metalness, emissive, velocity, depth, direct}: a Float32Array is RFX_PLANE_F32, a Uint16Array
 * (IEEE half bits) RFX_PLANE_F16; the channel count is the length over rows * width.  Returns 0 after throwing. */
static int read_aov_frame(napi_env env, rfx_ctx *c, napi_value obj, int32_t rows, rfx_aov_frame *f) {
    static const char *names[8] = {"diffuse", "normal", "roughness", "metalness", "emissive", "velocity", "depth", "direct"};
    rfx_plane *planes = &f->diffuse;
    int32_t W = 0;
    rfx_get_geometry(c, &W, NULL, NULL, NULL, NULL);
    const size_t n = rows > 0 ? (size_t)rows * (size_t)W : 0;
    memset(f, 0, sizeof *f);
    for (int i = 0; i < 8; i++) {
        napi_value v;
        bool has = false;
        napi_valuetype vt = napi_undefined;
        if (napi_has_named_property(env, obj, names[i], &has) == napi_ok && has && napi_get_named_property(env, obj, names[i], &v) == napi_ok) napi_typeof(env, v, &vt);
        if (!has || vt == napi_null || vt == napi_undefined) continue;
        napi_typedarray_type tt;
        size_t len;
        void *ptr;
        if (napi_get_typedarray_info(env, v, &tt, &len, &ptr, NULL, NULL) != napi_ok || (tt != napi_float32_array && tt != napi_uint16_array)) {
            napi_throw_type_error(env, NULL, "AOV plane: a Float32Array or a Uint16Array of half bits expected");
            return 0;
        }
        if (n == 0 || len == 0 || len % n) {
            napi_throw_range_error(env, NULL, "AOV plane: length is no multiple of rows * width");
            return 0;
        }
        planes[i].data = ptr;
        planes[i].type = tt == napi_uint16_array ? RFX_PLANE_F16 : RFX_PLANE_F32;
        planes[i].channels = (int)(len / n);
    }
    return 1;
}
/* stageAov(ctx, planes, row0, rows): rfx_stage_aov (rfx.h "streamed AOV frames"); the arrays — ideally views of hostAlloc() memory — must stay
 * alive and unchanged like stageUpload's.  aovStageBytes(ctx, planes, row0, rows) -> the bytes that call copies (0: it would be refused) */
static napi_value aov_call(napi_env env, napi_callback_info info, int stage) {
    napi_value a[4], out;
    int32_t row0, rows;
    rfx_aov_frame f;
    if (!get_args(env, info, 4, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[2], &row0) || !get_int(env, a[3], &rows)) return NULL;
    if (!read_aov_frame(env, c, a[1], rows, &f)) return NULL;
    if (!stage) {
        NAPI_CALL(env, napi_create_double(env, (double)rfx_aov_stage_bytes(c, &f, row0, rows), &out));
        return out;
    }
    int rc = rfx_stage_aov(c, &f, row0, rows);
    if (rc) return throw_rfx(env, c, "rfx_stage_aov", rc);
    return NULL;
}
/* setAovConventions(ctx, kinds, floats): rfx_set_aov_conventions (rfx.h "AOV conventions").  kinds: an Int32Array [depth_kind, velocity_kind,
 * normal_space, perspective, has_background_position]; floats: a Float32Array of 87 in the struct's order — velocity_scale[2], near_, far_, the
 * five matrices, background_position[3].  kinds null / undefined: back to the default. */
static napi_value n_set_aov_conventions(napi_env env, napi_callback_info info) {
    napi_value a[3];
    if (!get_args(env, info, 3, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    napi_valuetype vt = napi_undefined;
    napi_typeof(env, a[1], &vt);
    if (vt == napi_null || vt == napi_undefined) {
        int rc = rfx_set_aov_conventions(c, NULL);
        if (rc) return throw_rfx(env, c, "rfx_set_aov_conventions", rc);
        return NULL;
    }
    napi_typedarray_type tk, tf;
    size_t nk, nf;
    void *pk, *pf;
    if (napi_get_typedarray_info(env, a[1], &tk, &nk, &pk, NULL, NULL) != napi_ok || tk != napi_int32_array || nk != 5 ||
        napi_get_typedarray_info(env, a[2], &tf, &nf, &pf, NULL, NULL) != napi_ok || tf != napi_float32_array || nf != 87) {
        napi_throw_type_error(env, NULL, "setAovConventions: an Int32Array of 5 and a Float32Array of 87 expected");
        return NULL;
    }
    const int32_t *k = (const int32_t *)pk;
    const float *f = (const float *)pf;
    rfx_aov_conventions q;
    memset(&q, 0, sizeof q);
    q.depth_kind = k[0]; q.velocity_kind = k[1]; q.normal_space = k[2]; q.perspective = k[3]; q.has_background_position = k[4];
    q.velocity_scale[0] = f[0]; q.velocity_scale[1] = f[1];
    q.near_ = f[2]; q.far_ = f[3];
    memcpy(q.velocityMatrix, f + 4, 64); memcpy(q.prevVelocityMatrix, f + 20, 64); memcpy(q.projectionMatrix, f + 36, 64);
    memcpy(q.projectionMatrixInverse, f + 52, 64); memcpy(q.cameraMatrixWorld, f + 68, 64);
    memcpy(q.background_position, f + 84, 12);
    int rc = rfx_set_aov_conventions(c, &q);
    if (rc) return throw_rfx(env, c, "rfx_set_aov_conventions", rc);
    return NULL;
}
static napi_value n_stage_aov(napi_env env, napi_callback_info info) { return aov_call(env, info, 1); }
static napi_value n_aov_stage_bytes(napi_env env, napi_callback_info info) { return aov_call(env, info, 0); }
/* An EXR frame descriptor (rfx.h "streamed EXR frames") from what imageio.exrAovLayout returns: `bytes` the file (a Uint8Array / Buffer, ideally over
 * hostAlloc() memory), `parts` an Int32Array [parts, then per part: compression, channels, then per channel: pixel type, plane, component],
 * `chunks` a Uint8Array of rfx_exr_chunk records.  The descriptor is consumed by the call: its tables are copies in one block, *hold, which the
 * caller frees.  Returns 0 after throwing. */
static int read_exr_frame(napi_env env, napi_value bytes, napi_value parts, napi_value chunks, size_t record, rfx_exr_frame *f, void **hold) {
    napi_typedarray_type tb, tp, tc;
    size_t nb, np, nc;
    void *pb, *pp, *pc;
    *hold = NULL;
    if (napi_get_typedarray_info(env, bytes, &tb, &nb, &pb, NULL, NULL) != napi_ok || tb != napi_uint8_array ||
        napi_get_typedarray_info(env, parts, &tp, &np, &pp, NULL, NULL) != napi_ok || tp != napi_int32_array ||
        napi_get_typedarray_info(env, chunks, &tc, &nc, &pc, NULL, NULL) != napi_ok || tc != napi_uint8_array) {
        napi_throw_type_error(env, NULL, "EXR frame: (Uint8Array file bytes, Int32Array parts, Uint8Array chunk records) expected");
        return 0;
    }
    const int32_t *w = (const int32_t *)pp;
    size_t nparts = np ? (size_t)w[0] : 0, at = 1, nchan = 0;
    int ok = np >= 1 && w[0] > 0 && nc % record == 0 && nc > 0;
    for (size_t k = 0; ok && k < nparts; k++) {  /* walk the list once: it must end where the array ends */
        if (at + 2 > np || w[at + 1] <= 0 || at + 2 + 3 * (size_t)w[at + 1] > np) { ok = 0; break; }
        nchan += (size_t)w[at + 1];
        at += 2 + 3 * (size_t)w[at + 1];
    }
    if (!ok || at != np) { napi_throw_range_error(env, NULL, "EXR frame: the part list or the chunk records are malformed"); return 0; }
    const size_t parts_b = nparts * sizeof(rfx_exr_part), chans_b = nchan * sizeof(rfx_exr_channel);
    char *block = (char *)malloc(nc + parts_b + chans_b);  /* chunk records first: they hold 64-bit fields */
    if (!block) { napi_throw_error(env, NULL, "EXR frame: out of memory"); return 0; }
    memcpy(block, pc, nc);
    rfx_exr_part *P = (rfx_exr_part *)(block + nc);
    rfx_exr_channel *C = (rfx_exr_channel *)(block + nc + parts_b);
    at = 1;
    for (size_t k = 0; k < nparts; k++) {
        P[k].compression = w[at]; P[k].channels = w[at + 1]; P[k].channel = C;
        for (int32_t i = 0; i < w[at + 1]; i++, C++) { C->pixel_type = w[at + 2 + 3 * i]; C->plane = w[at + 3 + 3 * i]; C->component = w[at + 4 + 3 * i]; }
        at += 2 + 3 * (size_t)w[at + 1];
    }
    f->data = pb; f->bytes = nb; f->parts = (int)nparts; f->chunks = (int)(nc / record);
    f->part = P; f->chunk = (const rfx_exr_chunk *)block;
    *hold = block;
    return 1;
}
/* stageExrAov(ctx, bytes, parts, chunks, row0, rows): rfx_stage_exr_aov; `bytes` must stay alive and unchanged like stageUpload's planes.
 * exrAovStageBytes(...) -> the bytes that call copies (0: it would be refused).  exrAovStatus(ctx) -> [bad chunks, first bad chunk, code] */
static napi_value exr_aov_call(napi_env env, napi_callback_info info, int stage) {
    napi_value a[6], out = NULL;
    int32_t row0, rows;
    rfx_exr_frame f;
    void *hold;
    if (!get_args(env, info, 6, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[4], &row0) || !get_int(env, a[5], &rows)) return NULL;
    if (!read_exr_frame(env, a[1], a[2], a[3], sizeof(rfx_exr_chunk), &f, &hold)) return NULL;
    if (!stage) {
        const size_t n = rfx_exr_aov_stage_bytes(c, &f, row0, rows);
        free(hold);
        NAPI_CALL(env, napi_create_double(env, (double)n, &out));
        return out;
    }
    int rc = rfx_stage_exr_aov(c, &f, row0, rows);
    free(hold);
    if (rc) return throw_rfx(env, c, "rfx_stage_exr_aov", rc);
    return NULL;
}
static napi_value n_stage_exr_aov(napi_env env, napi_callback_info info) { return exr_aov_call(env, info, 1); }
static napi_value n_exr_aov_stage_bytes(napi_env env, napi_callback_info info) { return exr_aov_call(env, info, 0); }
/* stageExrBlocks / exrBlocksStageBytes(ctx, bytes, parts, blocks, row0, rows): rfx_stage_exr_blocks / rfx_exr_blocks_stage_bytes (rfx.h "EXR
 * blocks") — the same arguments, `blocks` a Uint8Array of rfx_exr_block records (imageio.exrAovLayout(..., { forms: "blocks" })) */
static napi_value exr_blocks_call(napi_env env, napi_callback_info info, int stage, int piz) {
    napi_value a[6], out = NULL;
    int32_t row0, rows;
    rfx_exr_frame f;
    void *hold;
    if (!get_args(env, info, 6, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[4], &row0) || !get_int(env, a[5], &rows)) return NULL;
    if (!read_exr_frame(env, a[1], a[2], a[3], sizeof(rfx_exr_block), &f, &hold)) return NULL;
    const rfx_exr_block_frame b = {f.data, f.bytes, f.parts, f.chunks, f.part, (const rfx_exr_block *)hold};  /* (the records lead the block) */
    if (!stage) {
        const size_t n = piz ? rfx_exr_blocks_piz_stage_bytes(c, &b, row0, rows) : rfx_exr_blocks_stage_bytes(c, &b, row0, rows);
        free(hold);
        NAPI_CALL(env, napi_create_double(env, (double)n, &out));
        return out;
    }
    int rc = piz ? rfx_stage_exr_blocks_piz(c, &b, row0, rows) : rfx_stage_exr_blocks(c, &b, row0, rows);
    free(hold);
    if (rc) return throw_rfx(env, c, piz ? "rfx_stage_exr_blocks_piz" : "rfx_stage_exr_blocks", rc);
    return NULL;
}
static napi_value n_stage_exr_blocks(napi_env env, napi_callback_info info) { return exr_blocks_call(env, info, 1, 0); }
static napi_value n_exr_blocks_stage_bytes(napi_env env, napi_callback_info info) { return exr_blocks_call(env, info, 0, 0); }
/* stageExrBlocksPiz / exrBlocksPizStageBytes: the same through rfx_stage_exr_blocks_piz / rfx_exr_blocks_piz_stage_bytes (rfx.h "EXR blocks with
 * PIZ": a part's compression may also be 4) */
static napi_value n_stage_exr_blocks_piz(napi_env env, napi_callback_info info) { return exr_blocks_call(env, info, 1, 1); }
static napi_value n_exr_blocks_piz_stage_bytes(napi_env env, napi_callback_info info) { return exr_blocks_call(env, info, 0, 1); }
static napi_value n_exr_aov_status(napi_env env, napi_callback_info info) {
    napi_value a[1], out, v;
    int s[3] = {0, -1, 0};
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    int rc = rfx_exr_aov_status(c, &s[0], &s[1], &s[2]);
    if (rc) return throw_rfx(env, c, "rfx_exr_aov_status", rc);
    NAPI_CALL(env, napi_create_array_with_length(env, 3, &out));
    for (uint32_t i = 0; i < 3; i++) {
        NAPI_CALL(env, napi_create_int32(env, s[i], &v));
        NAPI_CALL(env, napi_set_element(env, out, i, v));
    }
    return out;
}
static napi_value n_upload(napi_env env, napi_callback_info info) { return xfer(env, info, 1); }
static napi_value n_download(napi_env env, napi_callback_info info) { return xfer(env, info, 0); }

static napi_value n_clear(napi_env env, napi_callback_info info) {
    napi_value a[2];
    int32_t tex;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex)) return NULL;
    int rc = rfx_clear(c, (rfx_tex)tex);
    if (rc) return throw_rfx(env, c, "rfx_clear", rc);
    return NULL;
}

static const float *f32_prop(napi_env env, napi_value obj, const char *name, size_t want, int optional, int *ok) {
    napi_value v;
    bool has = false;
    napi_valuetype vt = napi_undefined;
    if (napi_has_named_property(env, obj, name, &has) == napi_ok && has && napi_get_named_property(env, obj, name, &v) == napi_ok) napi_typeof(env, v, &vt);
    if (!has || vt == napi_null || vt == napi_undefined) {
        if (!optional) { napi_throw_type_error(env, NULL, "AOV plane missing"); *ok = 0; }
        return NULL;
    }
    napi_typedarray_type tt;
    size_t len;
    void *ptr;
    if (napi_get_typedarray_info(env, v, &tt, &len, &ptr, NULL, NULL) != napi_ok || tt != napi_float32_array || len != want) {
        napi_throw_type_error(env, NULL, "AOV plane: Float32Array of rows * width * channels expected");
        *ok = 0;
        return NULL;
    }
    return (const float *)ptr;
}

/* packGBuffer(ctx, {diffuse, normal, roughness, metalness, emissive, depth?}, row0, rows) / packVelocity(ctx, {velocity, normal, depth}, row0, rows) */
static napi_value n_pack(napi_env env, napi_callback_info info, int velocity) {
    napi_value a[4];
    int32_t row0, rows, W = 0;
    if (!get_args(env, info, 4, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[2], &row0) || !get_int(env, a[3], &rows)) return NULL;
    rfx_get_geometry(c, &W, NULL, NULL, NULL, NULL);
    const size_t n = (size_t)rows * (size_t)W;
    int ok = 1, rc;
    if (velocity) {
        rfx_aov_velocity v = {f32_prop(env, a[1], "velocity", 2 * n, 0, &ok), f32_prop(env, a[1], "normal", 3 * n, 0, &ok), f32_prop(env, a[1], "depth", n, 0, &ok)};
        if (!ok) return NULL;
        rc = rfx_pack_velocity(c, &v, row0, rows);
    } else {
        rfx_aov_gbuffer g = {f32_prop(env, a[1], "diffuse", 4 * n, 0, &ok), f32_prop(env, a[1], "normal", 3 * n, 0, &ok), f32_prop(env, a[1], "roughness", n, 0, &ok),
                             f32_prop(env, a[1], "metalness", n, 0, &ok), f32_prop(env, a[1], "emissive", 3 * n, 0, &ok), f32_prop(env, a[1], "depth", n, 1, &ok)};
        if (!ok) return NULL;
        rc = rfx_pack_gbuffer(c, &g, row0, rows);
    }
    if (rc) return throw_rfx(env, c, velocity ? "rfx_pack_velocity" : "rfx_pack_gbuffer", rc);
    return NULL;
}
static napi_value n_pack_gbuffer(napi_env env, napi_callback_info info) { return n_pack(env, info, 0); }
static napi_value n_pack_velocity(napi_env env, napi_callback_info info) { return n_pack(env, info, 1); }

/* setEnvironment(ctx, Float32Array | null, width, height, halfFloatType, halfStoreRTZ) — scene.environment (rfx_set_environment) */
static napi_value n_set_environment(napi_env env, napi_callback_info info) {
    napi_value a[6];
    if (!get_args(env, info, 6, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    napi_valuetype vt;
    napi_typeof(env, a[1], &vt);
    int32_t w = 0, h = 0, half = 1, rtz = 1;
    const float *data = NULL;
    if (vt != napi_null && vt != napi_undefined) {
        napi_typedarray_type tt;
        size_t len;
        void *ptr;
        if (napi_get_typedarray_info(env, a[1], &tt, &len, &ptr, NULL, NULL) != napi_ok || tt != napi_float32_array) {
            napi_throw_type_error(env, NULL, "setEnvironment: Float32Array or null expected");
            return NULL;
        }
        if (!get_int(env, a[2], &w) || !get_int(env, a[3], &h) || !get_int(env, a[4], &half) || !get_int(env, a[5], &rtz)) return NULL;
        if ((size_t)w * (size_t)h * 4 != len) {
            napi_throw_range_error(env, NULL, "setEnvironment: data length != width * height * 4");
            return NULL;
        }
        data = (const float *)ptr;
    }
    int rc = rfx_set_environment(c, data, w, h, half, rtz);
    if (rc) return throw_rfx(env, c, "rfx_set_environment", rc);
    return NULL;
}

/* cubeToEquirect(ctx, Float32Array faces[6 * size * size * 4], size, generateMipmaps, Float32Array out[width * height * 4], width, height):
 * rfx_cube_to_equirect (CubeToEquirectEnvPass's draw + read-back) */
static napi_value n_cube_to_equirect(napi_env env, napi_callback_info info) {
    napi_value a[7];
    if (!get_args(env, info, 7, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    int32_t size, mips, w, h;
    if (!get_int(env, a[2], &size) || !get_int(env, a[3], &mips) || !get_int(env, a[5], &w) || !get_int(env, a[6], &h)) return NULL;
    napi_typedarray_type tt;
    size_t len_in, len_out;
    void *pin, *pout;
    if (napi_get_typedarray_info(env, a[1], &tt, &len_in, &pin, NULL, NULL) != napi_ok || tt != napi_float32_array ||
        napi_get_typedarray_info(env, a[4], &tt, &len_out, &pout, NULL, NULL) != napi_ok || tt != napi_float32_array) {
        napi_throw_type_error(env, NULL, "cubeToEquirect: Float32Array faces and Float32Array target expected");
        return NULL;
    }
    if (size < 1 || w < 1 || h < 1 || (size_t)6 * (size_t)size * (size_t)size * 4 != len_in || (size_t)w * (size_t)h * 4 != len_out) {
        napi_throw_range_error(env, NULL, "cubeToEquirect: faces length != 6 * size * size * 4 or target length != width * height * 4");
        return NULL;
    }
    int rc = rfx_cube_to_equirect(c, (const float *)pin, size, mips, (float *)pout, w, h);
    if (rc) return throw_rfx(env, c, "rfx_cube_to_equirect", rc);
    return NULL;
}

/* setEnvironmentImportance(ctx, Float32Array marginal, Float32Array conditional, totalSumWhole, totalSumDecimal) */
static napi_value n_set_environment_importance(napi_env env, napi_callback_info info) {
    napi_value a[5];
    if (!get_args(env, info, 5, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    const float *tab[2];
    size_t count[2];
    for (int k = 0; k < 2; k++) {
        napi_typedarray_type tt;
        size_t len;
        void *ptr;
        if (napi_get_typedarray_info(env, a[1 + k], &tt, &len, &ptr, NULL, NULL) != napi_ok || tt != napi_float32_array) {
            napi_throw_type_error(env, NULL, "setEnvironmentImportance: Float32Array expected");
            return NULL;
        }
        tab[k] = (const float *)ptr;
        count[k] = len;  /* the library checks them against the environment's size before it copies */
    }
    double whole = 0, dec = 0;
    if (napi_get_value_double(env, a[3], &whole) != napi_ok || napi_get_value_double(env, a[4], &dec) != napi_ok) {
        napi_throw_type_error(env, NULL, "setEnvironmentImportance: totalSumWhole / totalSumDecimal must be numbers");
        return NULL;
    }
    int rc = rfx_set_environment_importance(c, tab[0], count[0], tab[1], count[1], (float)whole, (float)dec);
    if (rc) return throw_rfx(env, c, "rfx_set_environment_importance", rc);
    return NULL;
}

/* ---- the environment kept on the device (include/rfx.h): stream-ordered, no read-back
 * setEnvironmentCube(ctx, Float32Array faces[6 * size * size * 4], size, generateMipmaps, width, height): rfx_set_environment_cube */
static napi_value n_set_environment_cube(napi_env env, napi_callback_info info) {
    napi_value a[6];
    if (!get_args(env, info, 6, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    int32_t size, mips, w, h;
    if (!get_int(env, a[2], &size) || !get_int(env, a[3], &mips) || !get_int(env, a[4], &w) || !get_int(env, a[5], &h)) return NULL;
    napi_typedarray_type tt;
    size_t len;
    void *ptr;
    if (napi_get_typedarray_info(env, a[1], &tt, &len, &ptr, NULL, NULL) != napi_ok || tt != napi_float32_array) {
        napi_throw_type_error(env, NULL, "setEnvironmentCube: Float32Array faces expected");
        return NULL;
    }
    if (size < 1 || (size_t)6 * (size_t)size * (size_t)size * 4 != len) {
        napi_throw_range_error(env, NULL, "setEnvironmentCube: faces length != 6 * size * size * 4");
        return NULL;
    }
    int rc = rfx_set_environment_cube(c, (const float *)ptr, size, mips, w, h);
    if (rc) return throw_rfx(env, c, "rfx_set_environment_cube", rc);
    return NULL;
}
/* buildEnvironmentImportance(ctx, flipY): rfx_build_environment_importance (K10) */
static napi_value n_build_environment_importance(napi_env env, napi_callback_info info) {
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    int32_t flip = 0;
    if (!c || !get_int(env, a[1], &flip)) return NULL;
    int rc = rfx_build_environment_importance(c, flip);
    if (rc) return throw_rfx(env, c, "rfx_build_environment_importance", rc);
    return NULL;
}
/* downloadEnvironmentImportance(ctx, Float32Array marginal[height], Float32Array conditional[width * height]) -> {totalSumValue, whole, decimal}
 * (the caller sizes the arrays for the environment it set: the library copies height and width * height floats) */
static napi_value n_download_environment_importance(napi_env env, napi_callback_info info) {
    napi_value a[5], out, v;
    if (!get_args(env, info, 5, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    int32_t w, h;
    if (!c || !get_int(env, a[3], &w) || !get_int(env, a[4], &h)) return NULL;
    float *tab[2];
    for (int k = 0; k < 2; k++) {
        napi_typedarray_type tt;
        size_t len;
        void *ptr;
        if (napi_get_typedarray_info(env, a[1 + k], &tt, &len, &ptr, NULL, NULL) != napi_ok || tt != napi_float32_array) {
            napi_throw_type_error(env, NULL, "downloadEnvironmentImportance: Float32Array expected");
            return NULL;
        }
        if (w < 1 || h < 1 || len != (k ? (size_t)w * (size_t)h : (size_t)h)) {
            napi_throw_range_error(env, NULL, "downloadEnvironmentImportance: marginal must hold height floats and conditional width * height");
            return NULL;
        }
        tab[k] = (float *)ptr;
    }
    int levels = 0;
    int rc = rfx_download_environment(c, 0, NULL, &levels);  /* the size the caller states must be the held environment's: 1 + log2(max edge) levels */
    int want = 1;
    for (int m = w > h ? w : h; m > 1; m >>= 1) want++;
    if (!rc && levels != want) {
        napi_throw_range_error(env, NULL, "downloadEnvironmentImportance: width / height are not the held environment's");
        return NULL;
    }
    double total = 0;
    float whole = 0, dec = 0;
    if (!rc) rc = rfx_download_environment_importance(c, tab[0], tab[1], &total, &whole, &dec);
    if (rc) return throw_rfx(env, c, "rfx_download_environment_importance", rc);
    NAPI_CALL(env, napi_create_object(env, &out));
    NAPI_CALL(env, napi_create_double(env, total, &v));
    NAPI_CALL(env, napi_set_named_property(env, out, "totalSumValue", v));
    NAPI_CALL(env, napi_create_double(env, whole, &v));
    NAPI_CALL(env, napi_set_named_property(env, out, "whole", v));
    NAPI_CALL(env, napi_create_double(env, dec, &v));
    NAPI_CALL(env, napi_set_named_property(env, out, "decimal", v));
    return out;
}

/* ssgiMarch / ssgiTrace / ssgiShade(ctx, {camera, steps, refineSteps, mode, useDirectLight, missedRays, importanceSampling,
 *                 rayDistance, thickness, envBlur, blueNoiseIndex, historySource, resolutionScale, useEnvMap}) */
static napi_value ssgi_stage(napi_env env, napi_callback_info info, int stage) {
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_ssgi_params p;
    memset(&p, 0, sizeof p);
    if (!read_camera(env, a[1], "camera", &p.camera)) return NULL;
    p.steps = (int32_t)prop_num(env, a[1], "steps", 20);
    p.refineSteps = (int32_t)prop_num(env, a[1], "refineSteps", 5);
    p.mode = (int32_t)prop_num(env, a[1], "mode", 0);
    p.useDirectLight = (int32_t)prop_num(env, a[1], "useDirectLight", 0);
    p.missedRays = (int32_t)prop_num(env, a[1], "missedRays", 0);
    p.importanceSampling = (int32_t)prop_num(env, a[1], "importanceSampling", 0);
    p.useEnvMap = (int32_t)prop_num(env, a[1], "useEnvMap", 0);
    p.rayDistance = (float)prop_num(env, a[1], "rayDistance", 10);
    p.thickness = (float)prop_num(env, a[1], "thickness", 10);
    p.envBlur = (float)prop_num(env, a[1], "envBlur", 0.5);
    p.blueNoiseIndex = (int32_t)prop_num(env, a[1], "blueNoiseIndex", 0);
    p.historySource = (int32_t)prop_num(env, a[1], "historySource", 0);
    p.resolutionScale = (float)prop_num(env, a[1], "resolutionScale", 1);
    int rc = stage == 0 ? rfx_ssgi_march(c, &p) : (stage == 1 ? rfx_ssgi_trace(c, &p) : rfx_ssgi_shade(c, &p));
    if (rc) return throw_rfx(env, c, stage == 0 ? "rfx_ssgi_march" : (stage == 1 ? "rfx_ssgi_trace" : "rfx_ssgi_shade"), rc);
    return NULL;
}
static napi_value n_ssgi(napi_env env, napi_callback_info info) { return ssgi_stage(env, info, 0); }
static napi_value n_ssgi_trace(napi_env env, napi_callback_info info) { return ssgi_stage(env, info, 1); }
static napi_value n_ssgi_shade(napi_env env, napi_callback_info info) { return ssgi_stage(env, info, 2); }

/* temporalReproject(ctx, {camera, prevCamera, textureCount, inputType, reprojectSpecular[2], neighborhoodClamp[2],
 *                         logTransform, fullAccumulate, confidencePower, neighborhoodClampIntensity, maxBlend, keepData,
 *                         historySource, targetHalf, halfStoreRTZ}) */
static napi_value n_temporal(napi_env env, napi_callback_info info) {
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_temporal_params p;
    memset(&p, 0, sizeof p);
    if (!read_camera(env, a[1], "camera", &p.camera) || !read_camera(env, a[1], "prevCamera", &p.prevCamera)) return NULL;
    p.textureCount = (int32_t)prop_num(env, a[1], "textureCount", 2);
    p.inputType = (int32_t)prop_num(env, a[1], "inputType", 0);
    prop_bool2(env, a[1], "reprojectSpecular", p.reprojectSpecular);
    prop_bool2(env, a[1], "neighborhoodClamp", p.neighborhoodClamp);
    p.logTransform = (int32_t)prop_num(env, a[1], "logTransform", 0);
    p.fullAccumulate = (int32_t)prop_num(env, a[1], "fullAccumulate", 0);
    p.confidencePower = (float)prop_num(env, a[1], "confidencePower", 0.75);
    p.neighborhoodClampIntensity = (float)prop_num(env, a[1], "neighborhoodClampIntensity", 1);
    p.maxBlend = (float)prop_num(env, a[1], "maxBlend", 1);
    p.keepData = (float)prop_num(env, a[1], "keepData", 1);
    p.historySource = (int32_t)prop_num(env, a[1], "historySource", 0);
    p.targetHalf = (int32_t)prop_num(env, a[1], "targetHalf", 0);
    p.halfStoreRTZ = (int32_t)prop_num(env, a[1], "halfStoreRTZ", 1);
    p.inputWidth = (int32_t)prop_num(env, a[1], "inputWidth", 0);
    p.inputHeight = (int32_t)prop_num(env, a[1], "inputHeight", 0);
    int rc = rfx_temporal_reproject(c, &p);
    if (rc) return throw_rfx(env, c, "rfx_temporal_reproject", rc);
    return NULL;
}

/* copyFramebuffer(ctx, dstTex) — renderer.copyFramebufferToTexture of TemporalReprojectPass.js:198-201 */
/* setRowWindow(ctx, y0, y1): rfx_set_row_window (y1 <= y0 resets) */
static napi_value n_set_row_window(napi_env env, napi_callback_info info) {
    napi_value a[3];
    int32_t y0, y1;
    if (!get_args(env, info, 3, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &y0) || !get_int(env, a[2], &y1)) return NULL;
    int rc = rfx_set_row_window(c, y0, y1);
    if (rc) return throw_rfx(env, c, "rfx_set_row_window", rc);
    return NULL;
}

/* setUvModel(ctx, model): rfx_set_uv_model (0 = RFX_UV_IDEAL, 1 = RFX_UV_REFERENCE_GL) */
static napi_value n_set_uv_model(napi_env env, napi_callback_info info) {
    napi_value a[2];
    int32_t m;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &m)) return NULL;
    int rc = rfx_set_uv_model(c, m);
    if (rc) return throw_rfx(env, c, "rfx_set_uv_model", rc);
    return NULL;
}

/* ---- row-tiled runs (rfx.h "row-tiled runs"): one Node process per GPU */
/* splitRows(height, nranks, rank) -> [tile_y0, tile_rows] */
static napi_value n_split_rows(napi_env env, napi_callback_info info) {
    napi_value a[3], arr, v;
    int32_t h, n, r;
    int y0 = 0, rows = 0;
    if (!get_args(env, info, 3, a) || !get_int(env, a[0], &h) || !get_int(env, a[1], &n) || !get_int(env, a[2], &r)) return NULL;
    if (rfx_split_rows(h, n, r, &y0, &rows) != RFX_OK) {
        napi_throw_range_error(env, NULL, "splitRows: height cannot be cut into that many tiles of at least 2 rows");
        return NULL;
    }
    NAPI_CALL(env, napi_create_array_with_length(env, 2, &arr));
    NAPI_CALL(env, napi_create_int32(env, y0, &v));
    napi_set_element(env, arr, 0, v);
    NAPI_CALL(env, napi_create_int32(env, rows, &v));
    napi_set_element(env, arr, 1, v);
    return arr;
}
/* commUniqueId() -> Buffer(128) (ncclGetUniqueId; rank 0 hands it to the other processes, e.g. through a file) */
static napi_value n_comm_unique_id(napi_env env, napi_callback_info info) {
    char id[128];
    napi_value buf;
    void *data = NULL;
    int rc = rfx_comm_unique_id(id);
    if (rc) {
        napi_throw_error(env, NULL, "rfx_comm_unique_id failed: RCCL not loadable on this host or no device");
        return NULL;
    }
    NAPI_CALL(env, napi_create_buffer_copy(env, sizeof id, id, &data, &buf));
    return buf;
}
/* commInit(ctx, Buffer id128, rank, nranks) */
static napi_value n_comm_init(napi_env env, napi_callback_info info) {
    napi_value a[4];
    int32_t rank, n;
    void *data = NULL;
    size_t len = 0;
    if (!get_args(env, info, 4, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[2], &rank) || !get_int(env, a[3], &n)) return NULL;
    if (napi_get_buffer_info(env, a[1], &data, &len) != napi_ok || len != 128) {
        napi_throw_type_error(env, NULL, "commInit: the unique id is a 128-byte Buffer");
        return NULL;
    }
    int rc = rfx_comm_init(c, data, rank, n);
    if (rc) return throw_rfx(env, c, "rfx_comm_init", rc);
    return NULL;
}
/* haloExchange(ctx, tex, upRank, downRank) — -1 = no such neighbour */
static napi_value n_halo_exchange(napi_env env, napi_callback_info info) {
    napi_value a[4];
    int32_t tex, up, down;
    if (!get_args(env, info, 4, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex) || !get_int(env, a[2], &up) || !get_int(env, a[3], &down)) return NULL;
    int rc = rfx_halo_exchange(c, (rfx_tex)tex, NULL, up, down);
    if (rc) return throw_rfx(env, c, "rfx_halo_exchange", rc);
    return NULL;
}
/* allgatherHistory(ctx, tex) */
static napi_value n_allgather_history(napi_env env, napi_callback_info info) {
    napi_value a[2];
    int32_t tex;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex)) return NULL;
    int rc = rfx_allgather_history(c, (rfx_tex)tex, NULL);
    if (rc) return throw_rfx(env, c, "rfx_allgather_history", rc);
    return NULL;
}
/* gatherHistoryRows(ctx, tex) -> bytes this rank receives (rfx_gather_history_rows: between ssgiTrace and ssgiShade) */
static napi_value n_gather_history_rows(napi_env env, napi_callback_info info) {
    napi_value a[2], out;
    int32_t tex;
    size_t got = 0;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex)) return NULL;
    int rc = rfx_gather_history_rows(c, (rfx_tex)tex, NULL, &got);
    if (rc) return throw_rfx(env, c, "rfx_gather_history_rows", rc);
    napi_create_double(env, (double)got, &out);
    return out;
}
/* The device-driven history gather (include/rfx.h rfx_peer_*: the consumer's own kernel loads the column blocks its rays read out of the
 * peers' planes through HIP IPC mappings).  peerExport(ctx, tex) -> Buffer of RFX_PEER_BLOB_BYTES; peerOpen(ctx, tex, Buffer of nranks blobs in
 * rank order, rank, nranks); peerGatherHistory(ctx, tex) -> bytes the PREVIOUS call pulled; peerClose(ctx) */
static napi_value n_peer_export(napi_env env, napi_callback_info info) {
    napi_value a[2], buf;
    int32_t tex;
    char blob[RFX_PEER_BLOB_BYTES];
    void *data = NULL;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex)) return NULL;
    int rc = rfx_peer_export(c, (rfx_tex)tex, blob);
    if (rc) return throw_rfx(env, c, "rfx_peer_export", rc);
    NAPI_CALL(env, napi_create_buffer_copy(env, sizeof blob, blob, &data, &buf));
    return buf;
}
static napi_value n_peer_open(napi_env env, napi_callback_info info) {
    napi_value a[5];
    int32_t tex, rank, n;
    void *data = NULL;
    size_t len = 0;
    if (!get_args(env, info, 5, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex) || !get_int(env, a[3], &rank) || !get_int(env, a[4], &n)) return NULL;
    if (n < 1 || napi_get_buffer_info(env, a[2], &data, &len) != napi_ok || len != (size_t)n * RFX_PEER_BLOB_BYTES) {
        napi_throw_type_error(env, NULL, "peerOpen: the blobs are one Buffer of nranks * RFX_PEER_BLOB_BYTES bytes, in rank order");
        return NULL;
    }
    int rc = rfx_peer_open(c, (rfx_tex)tex, data, rank, n);
    if (rc) return throw_rfx(env, c, "rfx_peer_open", rc);
    return NULL;
}
static napi_value n_peer_gather_history(napi_env env, napi_callback_info info) {
    napi_value a[2], out;
    int32_t tex;
    size_t got = 0;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex)) return NULL;
    int rc = rfx_peer_gather_history(c, (rfx_tex)tex, &got);
    if (rc) return throw_rfx(env, c, "rfx_peer_gather_history", rc);
    napi_create_double(env, (double)got, &out);
    return out;
}
static napi_value n_peer_close(napi_env env, napi_callback_info info) {
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    int rc = rfx_peer_close(c);
    if (rc) return throw_rfx(env, c, "rfx_peer_close", rc);
    return NULL;
}
/* ssgiHitMask(ctx, Uint32Array of frame-height entries): rfx_ssgi_hit_mask (after ssgiTrace; blocks until the trace has finished) */
static napi_value n_ssgi_hit_mask(napi_env env, napi_callback_info info) {
    napi_value a[2], ab;
    napi_typedarray_type type;
    size_t len = 0, off = 0;
    void *data = NULL;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    if (napi_get_typedarray_info(env, a[1], &type, &len, &data, &ab, &off) != napi_ok || type != napi_uint32_array) {
        napi_throw_type_error(env, NULL, "ssgiHitMask: a Uint32Array with one entry per frame row");
        return NULL;
    }
    int rc = rfx_ssgi_hit_mask(c, (unsigned int *)data, (int)len);
    if (rc) return throw_rfx(env, c, "rfx_ssgi_hit_mask", rc);
    return NULL;
}
/* commWait(ctx) / commDestroy(ctx) */
static napi_value n_comm_wait(napi_env env, napi_callback_info info) {
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    int rc = rfx_comm_wait(c);
    if (rc) return throw_rfx(env, c, "rfx_comm_wait", rc);
    return NULL;
}
static napi_value n_comm_destroy(napi_env env, napi_callback_info info) {
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_comm_destroy(c);
    return NULL;
}

static napi_value n_copy_framebuffer(napi_env env, napi_callback_info info) {
    napi_value a[2];
    int32_t tex;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex)) return NULL;
    int rc = rfx_copy_framebuffer(c, (rfx_tex)tex);
    if (rc) return throw_rfx(env, c, "rfx_copy_framebuffer", rc);
    return NULL;
}

/* poissonDenoise(ctx, {radius, phi, lumaPhi, depthPhi, normalPhi, roughnessPhi, specularPhi, textureCount,
 *                      isTextureSpecular[2], blueNoiseIndex, inputIsTemporal, writeToB, halfStoreRTZ}) */
static napi_value n_denoise(napi_env env, napi_callback_info info) {
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_denoise_params p;
    memset(&p, 0, sizeof p);
    p.radius = (float)prop_num(env, a[1], "radius", 3);
    p.phi = (float)prop_num(env, a[1], "phi", 0.5);
    p.lumaPhi = (float)prop_num(env, a[1], "lumaPhi", 5);
    p.depthPhi = (float)prop_num(env, a[1], "depthPhi", 2);
    p.normalPhi = (float)prop_num(env, a[1], "normalPhi", 3.25);
    p.roughnessPhi = (float)prop_num(env, a[1], "roughnessPhi", 0.0 / 0.0);
    p.specularPhi = (float)prop_num(env, a[1], "specularPhi", 0.0 / 0.0);
    p.textureCount = (int32_t)prop_num(env, a[1], "textureCount", 2);
    prop_bool2(env, a[1], "isTextureSpecular", p.isTextureSpecular);
    p.blueNoiseIndex = (int32_t)prop_num(env, a[1], "blueNoiseIndex", 0);
    p.inputIsTemporal = (int32_t)prop_num(env, a[1], "inputIsTemporal", 1);
    p.writeToB = (int32_t)prop_num(env, a[1], "writeToB", 0);
    p.halfStoreRTZ = (int32_t)prop_num(env, a[1], "halfStoreRTZ", 0);
    int rc = rfx_poisson_denoise(c, &p);
    if (rc) return throw_rfx(env, c, "rfx_poisson_denoise", rc);
    return NULL;
}

/* compose(ctx, {camera, inputType}) */
static napi_value n_compose(napi_env env, napi_callback_info info) {
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_compose_params p;
    memset(&p, 0, sizeof p);
    if (!read_camera(env, a[1], "camera", &p.camera)) return NULL;
    p.inputType = (int32_t)prop_num(env, a[1], "inputType", 0);
    p.giSource = (int32_t)prop_num(env, a[1], "giSource", 0);
    p.writeHistoryRGB = (int32_t)prop_num(env, a[1], "writeHistoryRGB", 0);
    int rc = rfx_compose(c, &p);
    if (rc) return throw_rfx(env, c, "rfx_compose", rc);
    return NULL;
}

/* finalCompose(ctx, {camera, isDebug, inputSource, fogMode, fogColor[3], fogNear, fogFar, fogDensity}) — SSGIEffect's own fragment */
static napi_value n_final(napi_env env, napi_callback_info info) {
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_final_params p;
    memset(&p, 0, sizeof p);
    if (!read_camera(env, a[1], "camera", &p.camera)) return NULL;
    p.isDebug = (int32_t)prop_num(env, a[1], "isDebug", 0);
    p.inputSource = (int32_t)prop_num(env, a[1], "inputSource", 0);
    p.fogMode = (int32_t)prop_num(env, a[1], "fogMode", 0);
    napi_value fc;
    bool has = false;
    if (napi_has_named_property(env, a[1], "fogColor", &has) == napi_ok && has && napi_get_named_property(env, a[1], "fogColor", &fc) == napi_ok) {
        for (uint32_t k = 0; k < 3; k++) {
            napi_value e;
            double v = 0;
            if (napi_get_element(env, fc, k, &e) == napi_ok) napi_get_value_double(env, e, &v);
            p.fogColor[k] = (float)v;
        }
    }
    p.fogNear = (float)prop_num(env, a[1], "fogNear", 0);
    p.fogFar = (float)prop_num(env, a[1], "fogFar", 0);
    p.fogDensity = (float)prop_num(env, a[1], "fogDensity", 0);
    int rc = rfx_final_compose(c, &p);
    if (rc) return throw_rfx(env, c, "rfx_final_compose", rc);
    return NULL;
}

/* the uniforms object of the four motion-blur calls: {source, center, centerAlphaOne, samples, intensity, jitter, deltaTime, frame, resolution[2],
 * targetHalf, halfStoreRTZ} -> rfx_motion_blur_params.  Returns 0 (a type error is pending) when `resolution` is malformed. */
static int motion_blur_params(napi_env env, napi_value o, const char *who, rfx_motion_blur_params *p) {
    memset(p, 0, sizeof *p);
    p->source = (int32_t)prop_num(env, o, "source", RFX_TEX_FINAL);
    p->center = (int32_t)prop_num(env, o, "center", -1);
    p->centerAlphaOne = (int32_t)prop_num(env, o, "centerAlphaOne", 0);
    p->samples = (int32_t)prop_num(env, o, "samples", 16);
    p->intensity = (float)prop_num(env, o, "intensity", 1);
    p->jitter = (float)prop_num(env, o, "jitter", 1);
    p->deltaTime = (float)prop_num(env, o, "deltaTime", 0);
    p->frame = (int32_t)prop_num(env, o, "frame", 0);
    if (!prop_floats(env, o, "resolution", p->resolution, 2)) {
        char msg[96];
        snprintf(msg, sizeof msg, "%s: resolution must hold 2 numbers", who);
        napi_throw_type_error(env, NULL, msg);
        return 0;
    }
    p->targetHalf = (int32_t)prop_num(env, o, "targetHalf", 0);
    p->halfStoreRTZ = (int32_t)prop_num(env, o, "halfStoreRTZ", 1);
    return 1;
}
/* motionBlur(ctx, uniforms) — MotionBlurEffect's fragment (K6, rfx_motion_blur) -> RFX_TEX_MOTION_BLUR */
static napi_value n_motion_blur(napi_env env, napi_callback_info info) {
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_motion_blur_params p;
    if (!motion_blur_params(env, a[1], "motionBlur", &p)) return NULL;
    int rc = rfx_motion_blur(c, &p);
    if (rc) return throw_rfx(env, c, "rfx_motion_blur", rc);
    return NULL;
}
/* motionBlurStage(ctx, uniforms): rfx_motion_blur_stage (a row tile's rows of the source into RFX_TEX_BLUR_SOURCE; arms the tiled draw) */
static napi_value n_motion_blur_stage(napi_env env, napi_callback_info info) {
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_motion_blur_params p;
    if (!motion_blur_params(env, a[1], "motionBlurStage", &p)) return NULL;
    int rc = rfx_motion_blur_stage(c, &p);
    if (rc) return throw_rfx(env, c, "rfx_motion_blur_stage", rc);
    return NULL;
}
/* motionBlurReachMask(ctx, uniforms, Uint32Array of frame-height entries): rfx_motion_blur_reach_mask (blocks) */
static napi_value n_motion_blur_reach_mask(napi_env env, napi_callback_info info) {
    napi_value a[3], ab;
    napi_typedarray_type type;
    size_t len = 0, off = 0;
    void *data = NULL;
    if (!get_args(env, info, 3, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_motion_blur_params p;
    if (!motion_blur_params(env, a[1], "motionBlurReachMask", &p)) return NULL;
    if (napi_get_typedarray_info(env, a[2], &type, &len, &data, &ab, &off) != napi_ok || type != napi_uint32_array) {
        napi_throw_type_error(env, NULL, "motionBlurReachMask: a Uint32Array with one entry per frame row");
        return NULL;
    }
    int rc = rfx_motion_blur_reach_mask(c, &p, (unsigned int *)data, (int)len);
    if (rc) return throw_rfx(env, c, "rfx_motion_blur_reach_mask", rc);
    return NULL;
}
/* motionBlurGather(ctx, uniforms) -> bytes this rank receives (rfx_motion_blur_gather over the context's communicator; commWait before the draw) */
static napi_value n_motion_blur_gather(napi_env env, napi_callback_info info) {
    napi_value a[2], out;
    size_t got = 0;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_motion_blur_params p;
    if (!motion_blur_params(env, a[1], "motionBlurGather", &p)) return NULL;
    int rc = rfx_motion_blur_gather(c, &p, NULL, &got);
    if (rc) return throw_rfx(env, c, "rfx_motion_blur_gather", rc);
    napi_create_double(env, (double)got, &out);
    return out;
}

/* the params object of the export calls: {source, format, channels, tonemap, exposure} -> rfx_export_params (include/rfx.h) */
static void export_params(napi_env env, napi_value o, rfx_export_params *p) {
    memset(p, 0, sizeof *p);
    p->source = (int32_t)prop_num(env, o, "source", RFX_TEX_FINAL);
    p->format = (int32_t)prop_num(env, o, "format", RFX_EXPORT_U8_SRGB);
    p->channels = (int32_t)prop_num(env, o, "channels", 3);
    p->tonemap = (int32_t)prop_num(env, o, "tonemap", 0);
    p->exposure = (float)prop_num(env, o, "exposure", 1);
}
/* exportBytes(ctx, params) -> rfx_export_bytes (0: bad params) */
static napi_value n_export_bytes(napi_env env, napi_callback_info info) {
    napi_value a[2], out;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_export_params p;
    export_params(env, a[1], &p);
    NAPI_CALL(env, napi_create_double(env, (double)rfx_export_bytes(c, &p), &out));
    return out;
}
/* exportFrame(ctx, params, typedArray): rfx_export (blocks) / stageExport(ctx, params, typedArray) -> ticket: rfx_stage_export — the array,
 * ideally a view of hostAlloc() memory, must stay alive until exportWait(ctx, ticket) has returned.  The library checks the byte count. */
static napi_value export_into(napi_env env, napi_callback_info info, int staged) {
    napi_value a[3], ab, out;
    napi_typedarray_type type;
    size_t len = 0, off = 0;
    void *data = NULL;
    if (!get_args(env, info, 3, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_export_params p;
    export_params(env, a[1], &p);
    bool is_ta = false;
    napi_is_typedarray(env, a[2], &is_ta);
    if (!is_ta || napi_get_typedarray_info(env, a[2], &type, &len, &data, &ab, &off) != napi_ok || !data) {
        napi_throw_type_error(env, NULL, staged ? "stageExport: TypedArray expected" : "exportFrame: TypedArray expected");
        return NULL;
    }
    static const size_t esz[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
    int ticket = 0;
    int rc = staged ? rfx_stage_export(c, &p, data, len * esz[type], &ticket) : rfx_export(c, &p, data, len * esz[type]);
    if (rc) return throw_rfx(env, c, staged ? "rfx_stage_export" : "rfx_export", rc);
    if (!staged) return NULL;
    NAPI_CALL(env, napi_create_int32(env, ticket, &out));
    return out;
}
static napi_value n_export_frame(napi_env env, napi_callback_info info) { return export_into(env, info, 0); }
static napi_value n_stage_export(napi_env env, napi_callback_info info) { return export_into(env, info, 1); }
/* pngBound(ctx, params) -> rfx_png_bound (0: bad params or a format other than U8_SRGB) */
static napi_value n_png_bound(napi_env env, napi_callback_info info) {
    napi_value a[2], out;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_export_params p;
    export_params(env, a[1], &p);
    NAPI_CALL(env, napi_create_double(env, (double)rfx_png_bound(c, &p), &out));
    return out;
}
/* pngFrame(ctx, params, filter, Uint8Array): rfx_png (blocks) / stagePng(ctx, params, filter, Uint8Array) -> ticket: rfx_stage_png — the result
 * buffer of include/rfx.h "PNG fragments"; the array must stay alive until exportWait(ctx, ticket) has returned.  The library checks the byte count. */
/* pngFrameEx(ctx, params, filter, flags, Uint8Array) / stagePngEx(...) -> ticket: rfx_png_ex / rfx_stage_png_ex (rfx.h "Match form": flags =
 * RFX_ENCODE_MATCHES or 0) */
static napi_value png_into(napi_env env, napi_callback_info info, int staged, int ex) {
    napi_value a[5], ab, out;
    napi_typedarray_type type;
    size_t len = 0, off = 0;
    void *data = NULL;
    int32_t filter = 0, flags = 0;
    if (!get_args(env, info, ex ? 5 : 4, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[2], &filter) || (ex && !get_int(env, a[3], &flags))) return NULL;
    rfx_export_params p;
    export_params(env, a[1], &p);
    napi_value arr = a[ex ? 4 : 3];
    bool is_ta = false;
    napi_is_typedarray(env, arr, &is_ta);
    if (!is_ta || napi_get_typedarray_info(env, arr, &type, &len, &data, &ab, &off) != napi_ok || !data || type != napi_uint8_array) {
        napi_throw_type_error(env, NULL, staged ? "stagePng: Uint8Array expected" : "pngFrame: Uint8Array expected");
        return NULL;
    }
    int ticket = 0, rc;
    if (ex) {
        rc = staged ? rfx_stage_png_ex(c, &p, filter, (unsigned)flags, data, len, &ticket) : rfx_png_ex(c, &p, filter, (unsigned)flags, data, len);
        if (rc) return throw_rfx(env, c, staged ? "rfx_stage_png_ex" : "rfx_png_ex", rc);
    } else {
        rc = staged ? rfx_stage_png(c, &p, filter, data, len, &ticket) : rfx_png(c, &p, filter, data, len);
        if (rc) return throw_rfx(env, c, staged ? "rfx_stage_png" : "rfx_png", rc);
    }
    if (!staged) return NULL;
    NAPI_CALL(env, napi_create_int32(env, ticket, &out));
    return out;
}
static napi_value n_png_frame(napi_env env, napi_callback_info info) { return png_into(env, info, 0, 0); }
static napi_value n_stage_png(napi_env env, napi_callback_info info) { return png_into(env, info, 1, 0); }
static napi_value n_png_frame_ex(napi_env env, napi_callback_info info) { return png_into(env, info, 0, 1); }
static napi_value n_stage_png_ex(napi_env env, napi_callback_info info) { return png_into(env, info, 1, 1); }
/* exrBound(ctx, params) -> rfx_exr_bound (0: bad params or a format other than F16) */
static napi_value n_exr_bound(napi_env env, napi_callback_info info) {
    napi_value a[2], out;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    rfx_export_params p;
    export_params(env, a[1], &p);
    NAPI_CALL(env, napi_create_double(env, (double)rfx_exr_bound(c, &p), &out));
    return out;
}
/* exrFrame(ctx, params, Uint8Array): rfx_exr (blocks) / stageExr(ctx, params, Uint8Array) -> ticket: rfx_stage_exr — the result buffer of
 * include/rfx.h "EXR fragments"; the array must stay alive until exportWait(ctx, ticket) has returned.  The library checks the byte count. */
/* exrFrameEx(ctx, params, flags, Uint8Array) / stageExrEx(...) -> ticket: rfx_exr_ex / rfx_stage_exr_ex (rfx.h "Match form") */
static napi_value exr_into(napi_env env, napi_callback_info info, int staged, int ex) {
    napi_value a[4], ab, out;
    napi_typedarray_type type;
    size_t len = 0, off = 0;
    void *data = NULL;
    int32_t flags = 0;
    if (!get_args(env, info, ex ? 4 : 3, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || (ex && !get_int(env, a[2], &flags))) return NULL;
    rfx_export_params p;
    export_params(env, a[1], &p);
    napi_value arr = a[ex ? 3 : 2];
    bool is_ta = false;
    napi_is_typedarray(env, arr, &is_ta);
    if (!is_ta || napi_get_typedarray_info(env, arr, &type, &len, &data, &ab, &off) != napi_ok || !data || type != napi_uint8_array) {
        napi_throw_type_error(env, NULL, staged ? "stageExr: Uint8Array expected" : "exrFrame: Uint8Array expected");
        return NULL;
    }
    int ticket = 0, rc;
    if (ex) {
        rc = staged ? rfx_stage_exr_ex(c, &p, (unsigned)flags, data, len, &ticket) : rfx_exr_ex(c, &p, (unsigned)flags, data, len);
        if (rc) return throw_rfx(env, c, staged ? "rfx_stage_exr_ex" : "rfx_exr_ex", rc);
    } else {
        rc = staged ? rfx_stage_exr(c, &p, data, len, &ticket) : rfx_exr(c, &p, data, len);
        if (rc) return throw_rfx(env, c, staged ? "rfx_stage_exr" : "rfx_exr", rc);
    }
    if (!staged) return NULL;
    NAPI_CALL(env, napi_create_int32(env, ticket, &out));
    return out;
}
static napi_value n_exr_frame(napi_env env, napi_callback_info info) { return exr_into(env, info, 0, 0); }
static napi_value n_stage_exr(napi_env env, napi_callback_info info) { return exr_into(env, info, 1, 0); }
static napi_value n_exr_frame_ex(napi_env env, napi_callback_info info) { return exr_into(env, info, 0, 1); }
static napi_value n_stage_exr_ex(napi_env env, napi_callback_info info) { return exr_into(env, info, 1, 1); }
/* exportWait(ctx, ticket): rfx_export_wait */
static napi_value n_export_wait(napi_env env, napi_callback_info info) {
    napi_value a[2];
    int32_t ticket = 0;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &ticket)) return NULL;
    int rc = rfx_export_wait(c, ticket);
    if (rc) return throw_rfx(env, c, "rfx_export_wait", rc);
    return NULL;
}
/* constants() -> the header's values the JS side mirrors (js/Renderer.js EXPORT, PROF_KINDS): checked against each other by the tests */
static napi_value n_constants(napi_env env, napi_callback_info info) {
    (void)info;
    static const struct { const char *name; int v; } k[] = {
        {"EXPORT_F32", RFX_EXPORT_F32}, {"EXPORT_F16", RFX_EXPORT_F16}, {"EXPORT_U8_SRGB", RFX_EXPORT_U8_SRGB},
        {"PROF_K7", RFX_PROF_K7}, {"PROF_COUNT", RFX_PROF_COUNT}, {"TEX_COUNT", RFX_TEX_COUNT}, {"ABI_VERSION", RFX_ABI_VERSION},
    };
    napi_value out;
    NAPI_CALL(env, napi_create_object(env, &out));
    for (size_t i = 0; i < sizeof k / sizeof k[0]; i++) {
        napi_value v;
        NAPI_CALL(env, napi_create_int32(env, k[i].v, &v));
        NAPI_CALL(env, napi_set_named_property(env, out, k[i].name, v));
    }
    return out;
}

static napi_value n_sync(napi_env env, napi_callback_info info) {
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    int rc = rfx_sync(c);
    if (rc) return throw_rfx(env, c, "rfx_sync", rc);
    return NULL;
}

static napi_value n_halo_violations(napi_env env, napi_callback_info info) {
    napi_value a[1], out;
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    NAPI_CALL(env, napi_create_uint32(env, rfx_halo_violations(c), &out));
    return out;
}

/* timeBegin(ctx) / timeEnd(ctx) -> ms */
static napi_value n_time_begin(napi_env env, napi_callback_info info) {
    napi_value a[1];
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    int rc = rfx_time_begin(c);
    if (rc) return throw_rfx(env, c, "rfx_time_begin", rc);
    return NULL;
}
static napi_value n_time_end(napi_env env, napi_callback_info info) {
    napi_value a[1], out;
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    float ms = 0;
    int rc = rfx_time_end(c, &ms);
    if (rc) return throw_rfx(env, c, "rfx_time_end", rc);
    NAPI_CALL(env, napi_create_double(env, ms, &out));
    return out;
}

/* profile(ctx, enable) / profileRead(ctx) -> { ms, launches }: arrays of RFX_PROF_COUNT_ALL entries (rfx_profile, rfx_profile_read_n) */
static napi_value n_profile(napi_env env, napi_callback_info info) {
    napi_value a[2];
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    int32_t on = 0;
    NAPI_CALL(env, napi_get_value_int32(env, a[1], &on));
    int rc = rfx_profile(c, on);
    if (rc) return throw_rfx(env, c, "rfx_profile", rc);
    return NULL;
}
static napi_value n_profile_read(napi_env env, napi_callback_info info) {
    napi_value a[1], out, ms_arr, n_arr;
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    float ms[RFX_PROF_COUNT_ALL];
    int n[RFX_PROF_COUNT_ALL];
    int rc = rfx_profile_read_n(c, ms, n, RFX_PROF_COUNT_ALL);
    if (rc) return throw_rfx(env, c, "rfx_profile_read", rc);
    NAPI_CALL(env, napi_create_object(env, &out));
    NAPI_CALL(env, napi_create_array_with_length(env, RFX_PROF_COUNT_ALL, &ms_arr));
    NAPI_CALL(env, napi_create_array_with_length(env, RFX_PROF_COUNT_ALL, &n_arr));
    for (uint32_t i = 0; i < RFX_PROF_COUNT_ALL; i++) {
        napi_value v;
        NAPI_CALL(env, napi_create_double(env, ms[i], &v));
        NAPI_CALL(env, napi_set_element(env, ms_arr, i, v));
        NAPI_CALL(env, napi_create_int32(env, n[i], &v));
        NAPI_CALL(env, napi_set_element(env, n_arr, i, v));
    }
    NAPI_CALL(env, napi_set_named_property(env, out, "ms", ms_arr));
    NAPI_CALL(env, napi_set_named_property(env, out, "launches", n_arr));
    return out;
}

static napi_value init(napi_env env, napi_value exports) {
    static const struct { const char *name; napi_callback fn; } fns[] = {
        {"abiVersion", n_abi_version}, {"create", n_create}, {"heldRows", n_held_rows}, {"ssgiTargetRows", n_ssgi_target_rows}, {"upload", n_upload}, {"download", n_download},
        {"clear", n_clear}, {"setEnvironment", n_set_environment}, {"setEnvironmentImportance", n_set_environment_importance}, {"packGBuffer", n_pack_gbuffer}, {"packVelocity", n_pack_velocity}, {"ssgiMarch", n_ssgi}, {"ssgiTrace", n_ssgi_trace}, {"ssgiShade", n_ssgi_shade}, {"temporalReproject", n_temporal}, {"copyFramebuffer", n_copy_framebuffer}, {"poissonDenoise", n_denoise}, {"compose", n_compose}, {"finalCompose", n_final}, {"motionBlur", n_motion_blur},
        {"motionBlurStage", n_motion_blur_stage}, {"motionBlurReachMask", n_motion_blur_reach_mask}, {"motionBlurGather", n_motion_blur_gather},
        {"sync", n_sync}, {"setRowWindow", n_set_row_window}, {"setUvModel", n_set_uv_model}, {"cubeToEquirect", n_cube_to_equirect}, {"setEnvironmentCube", n_set_environment_cube}, {"buildEnvironmentImportance", n_build_environment_importance}, {"downloadEnvironmentImportance", n_download_environment_importance}, {"haloViolations", n_halo_violations}, {"timeBegin", n_time_begin}, {"timeEnd", n_time_end}, {"profile", n_profile}, {"profileRead", n_profile_read},
        {"stageUpload", n_stage_upload}, {"stageFlip", n_stage_flip}, {"hostAlloc", n_host_alloc}, {"stageAov", n_stage_aov}, {"setAovConventions", n_set_aov_conventions},{"aovStageBytes", n_aov_stage_bytes},
        {"stageExrAov", n_stage_exr_aov}, {"exrAovStageBytes", n_exr_aov_stage_bytes}, {"exrAovStatus", n_exr_aov_status},
        {"stageExrBlocks", n_stage_exr_blocks}, {"exrBlocksStageBytes", n_exr_blocks_stage_bytes},
        {"stageExrBlocksPiz", n_stage_exr_blocks_piz}, {"exrBlocksPizStageBytes", n_exr_blocks_piz_stage_bytes},
        {"exportBytes", n_export_bytes}, {"exportFrame", n_export_frame}, {"stageExport", n_stage_export}, {"exportWait", n_export_wait}, {"constants", n_constants},
        {"pngBound", n_png_bound}, {"pngFrame", n_png_frame}, {"stagePng", n_stage_png},
        {"exrBound", n_exr_bound}, {"exrFrame", n_exr_frame}, {"stageExr", n_stage_exr},
        {"pngFrameEx", n_png_frame_ex}, {"stagePngEx", n_stage_png_ex}, {"exrFrameEx", n_exr_frame_ex}, {"stageExrEx", n_stage_exr_ex},
        {"splitRows", n_split_rows}, {"commUniqueId", n_comm_unique_id}, {"commInit", n_comm_init}, {"haloExchange", n_halo_exchange},
        {"allgatherHistory", n_allgather_history}, {"gatherHistoryRows", n_gather_history_rows}, {"commWait", n_comm_wait}, {"commDestroy", n_comm_destroy},
        {"peerExport", n_peer_export}, {"peerOpen", n_peer_open}, {"peerGatherHistory", n_peer_gather_history}, {"peerClose", n_peer_close}, {"ssgiHitMask", n_ssgi_hit_mask},
    };
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
        napi_set_named_property(env, exports, fns[i].name, f);
    }
    return exports;
}

NAPI_MODULE(rfx_napi, init)
