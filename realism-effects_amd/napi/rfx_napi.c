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
#include <math.h>
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
/* the `data` pointer the function was created with (init): what the callbacks that serve several exports select by */
static void *call_data(napi_env env, napi_callback_info info) {
    void *data = NULL;
    napi_get_cb_info(env, info, NULL, NULL, NULL, &data);
    return data;
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

/* obj[name] = three numbers -> out[3]; missing: left as it is, an element that is no number: 0 */
static void prop_float3(napi_env env, napi_value obj, const char *name, float *out) {
    napi_value v;
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has || napi_get_named_property(env, obj, name, &v) != napi_ok) return;
    for (uint32_t k = 0; k < 3; k++) {
        napi_value e;
        double d = 0;
        if (napi_get_element(env, v, k, &e) == napi_ok) napi_get_value_double(env, e, &d);
        out[k] = (float)d;
    }
}

/* ---- the parameter objects of the draws and of the export calls: plain JS objects whose property names are the fields' (the reference's uniform /
 * define names), read by one reader from one table per struct of include/rfx.h: {field, kind, offset, default where the property is missing}.
 * An int or a float takes a number or a boolean; INT2 (a define bool[2]) a scalar for both or an array, default 0; FLOAT3 an array, default 0;
 * FLOAT2 and CAMERA are required.  -NAN (denoise): the quiet NaN with the sign bit set, what 0.0 / 0.0 evaluated at run time gives on the host.
 * A table lists every field of its struct, in the struct's order: table_that_misses_a_field() below, checked when the addon loads. */
typedef enum { F_INT, F_FLOAT, F_INT2, F_FLOAT2, F_FLOAT3, F_CAMERA } field_kind;
static const size_t FIELD_BYTES[] = {sizeof(int32_t), sizeof(float), 2 * sizeof(int32_t), 2 * sizeof(float), 3 * sizeof(float), sizeof(rfx_camera)};
typedef struct { const char *name; field_kind kind; size_t offset; double def; } field;
#define FIELD(S, name, kind, def) {#name, kind, offsetof(S, name), def}

#define S rfx_ssgi_params
static const field ssgi_fields[] = {
    FIELD(S, camera, F_CAMERA, 0), FIELD(S, steps, F_INT, 20), FIELD(S, refineSteps, F_INT, 5), FIELD(S, mode, F_INT, 0), FIELD(S, useDirectLight, F_INT, 0),
    FIELD(S, missedRays, F_INT, 0), FIELD(S, importanceSampling, F_INT, 0), FIELD(S, useEnvMap, F_INT, 0), FIELD(S, rayDistance, F_FLOAT, 10),
    FIELD(S, thickness, F_FLOAT, 10), FIELD(S, envBlur, F_FLOAT, 0.5), FIELD(S, blueNoiseIndex, F_INT, 0), FIELD(S, resolutionScale, F_FLOAT, 1),
    FIELD(S, historySource, F_INT, 0),
};
#undef S
#define S rfx_temporal_params
static const field temporal_fields[] = {
    FIELD(S, camera, F_CAMERA, 0), FIELD(S, prevCamera, F_CAMERA, 0), FIELD(S, textureCount, F_INT, 2), FIELD(S, inputType, F_INT, 0),
    FIELD(S, reprojectSpecular, F_INT2, 0), FIELD(S, neighborhoodClamp, F_INT2, 0), FIELD(S, logTransform, F_INT, 0), FIELD(S, fullAccumulate, F_INT, 0),
    FIELD(S, confidencePower, F_FLOAT, 0.75), FIELD(S, neighborhoodClampIntensity, F_FLOAT, 1), FIELD(S, maxBlend, F_FLOAT, 1), FIELD(S, keepData, F_FLOAT, 1),
    FIELD(S, historySource, F_INT, 0), FIELD(S, targetHalf, F_INT, 0), FIELD(S, halfStoreRTZ, F_INT, 1), FIELD(S, inputWidth, F_INT, 0),
    FIELD(S, inputHeight, F_INT, 0),
};
#undef S
#define S rfx_denoise_params
static const field denoise_fields[] = {
    FIELD(S, radius, F_FLOAT, 3), FIELD(S, phi, F_FLOAT, 0.5), FIELD(S, lumaPhi, F_FLOAT, 5), FIELD(S, depthPhi, F_FLOAT, 2), FIELD(S, normalPhi, F_FLOAT, 3.25),
    FIELD(S, roughnessPhi, F_FLOAT, -NAN), FIELD(S, specularPhi, F_FLOAT, -NAN), FIELD(S, textureCount, F_INT, 2),
    FIELD(S, isTextureSpecular, F_INT2, 0), FIELD(S, blueNoiseIndex, F_INT, 0), FIELD(S, inputIsTemporal, F_INT, 1), FIELD(S, writeToB, F_INT, 0),
    FIELD(S, halfStoreRTZ, F_INT, 0),
};
#undef S
#define S rfx_compose_params
static const field compose_fields[] = {
    FIELD(S, camera, F_CAMERA, 0), FIELD(S, inputType, F_INT, 0), FIELD(S, giSource, F_INT, 0), FIELD(S, writeHistoryRGB, F_INT, 0),
};
#undef S
#define S rfx_final_params
static const field final_fields[] = {
    FIELD(S, camera, F_CAMERA, 0), FIELD(S, isDebug, F_INT, 0), FIELD(S, inputSource, F_INT, 0), FIELD(S, fogMode, F_INT, 0), FIELD(S, fogColor, F_FLOAT3, 0),
    FIELD(S, fogNear, F_FLOAT, 0), FIELD(S, fogFar, F_FLOAT, 0), FIELD(S, fogDensity, F_FLOAT, 0),
};
#undef S
#define S rfx_motion_blur_params
static const field motion_blur_fields[] = {
    FIELD(S, source, F_INT, RFX_TEX_FINAL), FIELD(S, center, F_INT, -1), FIELD(S, centerAlphaOne, F_INT, 0), FIELD(S, samples, F_INT, 16),
    FIELD(S, intensity, F_FLOAT, 1), FIELD(S, jitter, F_FLOAT, 1), FIELD(S, deltaTime, F_FLOAT, 0), FIELD(S, frame, F_INT, 0), FIELD(S, resolution, F_FLOAT2, 0),
    FIELD(S, targetHalf, F_INT, 0), FIELD(S, halfStoreRTZ, F_INT, 1),
};
#undef S
#define S rfx_export_params
static const field export_fields[] = {
    FIELD(S, source, F_INT, RFX_TEX_FINAL), FIELD(S, format, F_INT, RFX_EXPORT_U8_SRGB), FIELD(S, channels, F_INT, 3), FIELD(S, tonemap, F_INT, 0),
    FIELD(S, exposure, F_FLOAT, 1),
};
#undef S

typedef enum { P_SSGI, P_TEMPORAL, P_DENOISE, P_COMPOSE, P_FINAL, P_MOTION_BLUR, P_EXPORT, P_COUNT } params_kind;
typedef union {
    rfx_ssgi_params ssgi; rfx_temporal_params temporal; rfx_denoise_params denoise; rfx_compose_params compose; rfx_final_params final;
    rfx_motion_blur_params motion_blur; rfx_export_params export_;
} any_params;
#define TABLE(name, fields, S) {name, fields, sizeof fields / sizeof fields[0], sizeof(S)}
static const struct { const char *name; const field *fields; size_t count, size; } PARAMS[P_COUNT] = {  /* name: paramBytes' `kind` */
    TABLE("ssgi", ssgi_fields, rfx_ssgi_params), TABLE("temporal", temporal_fields, rfx_temporal_params), TABLE("denoise", denoise_fields, rfx_denoise_params),
    TABLE("compose", compose_fields, rfx_compose_params), TABLE("final", final_fields, rfx_final_params),
    TABLE("motionBlur", motion_blur_fields, rfx_motion_blur_params), TABLE("export", export_fields, rfx_export_params),
};

/* NULL, or the name of a table whose fields do not tile its struct from offset 0 to sizeof: a field of rfx.h that a table forgets must stop the
 * addon from loading instead of reading as 0 (the structs hold 4-byte members only: no padding) */
static const char *table_that_misses_a_field(void) {
    for (int k = 0; k < P_COUNT; k++) {
        size_t at = 0;
        for (size_t i = 0; i < PARAMS[k].count; at += FIELD_BYTES[PARAMS[k].fields[i++].kind])
            if (PARAMS[k].fields[i].offset != at) return PARAMS[k].name;
        if (at != PARAMS[k].size) return PARAMS[k].name;
    }
    return NULL;
}

/* obj -> the struct of `kind` at `out`, as the call passes it to the C ABI.  Returns 0 (a type error is pending, naming `who`) when a required field
 * is missing or malformed. */
static int read_params(napi_env env, napi_value obj, params_kind kind, const char *who, void *out) {
    memset(out, 0, PARAMS[kind].size);
    for (size_t i = 0; i < PARAMS[kind].count; i++) {
        const field *f = &PARAMS[kind].fields[i];
        void *at = (char *)out + f->offset;
        switch (f->kind) {
        case F_INT: *(int32_t *)at = (int32_t)prop_num(env, obj, f->name, f->def); break;
        case F_FLOAT: *(float *)at = (float)prop_num(env, obj, f->name, f->def); break;
        case F_INT2: prop_bool2(env, obj, f->name, (int32_t *)at); break;
        case F_FLOAT3: prop_float3(env, obj, f->name, (float *)at); break;
        case F_CAMERA: if (!read_camera(env, obj, f->name, (rfx_camera *)at)) return 0; break;
        case F_FLOAT2:
            if (!prop_floats(env, obj, f->name, (float *)at, 2)) {
                char msg[96];
                snprintf(msg, sizeof msg, "%s: %s must hold 2 numbers", who, f->name);
                napi_throw_type_error(env, NULL, msg);
                return 0;
            }
            break;
        }
    }
    return 1;
}
static int kind_by_name(napi_env env, napi_value v) {
    char name[16] = "";
    size_t n = 0;
    if (napi_get_value_string_utf8(env, v, name, sizeof name, &n) == napi_ok)
        for (int k = 0; k < P_COUNT; k++) if (!strcmp(name, PARAMS[k].name)) return k;
    return -1;
}
/* paramBytes(kind, object) -> Buffer: the struct of "ssgi" | "temporal" | "denoise" | "compose" | "final" | "motionBlur" | "export" exactly as the
 * corresponding call passes it to the C ABI.  A test hook in the spirit of the library's rfx_internal_* plan exports: no context, no GPU; js/ does
 * not use it. */
static napi_value n_param_bytes(napi_env env, napi_callback_info info) {
    napi_value a[2], buf;
    any_params p;
    void *copy = NULL;
    if (!get_args(env, info, 2, a)) return NULL;
    const int kind = kind_by_name(env, a[0]);
    if (kind < 0) { napi_throw_range_error(env, NULL, "paramBytes: unknown kind"); return NULL; }
    if (!read_params(env, a[1], (params_kind)kind, "paramBytes", &p)) return NULL;
    NAPI_CALL(env, napi_create_buffer_copy(env, PARAMS[kind].size, &p, &copy, &buf));
    return buf;
}
/* the draws and the calls like them — (ctx, params object): read the struct of `kind`, call, throw on rc.  One row of EXPORTS each (DRAW) */
typedef struct { const char *js, *c_name; params_kind kind; int (*fn)(rfx_ctx *, const void *); } params_fn;
#define PARAMS_FN(fn, T) static int p_##fn(rfx_ctx *c, const void *p) { return fn(c, (const T *)p); }
PARAMS_FN(rfx_ssgi_march, rfx_ssgi_params) PARAMS_FN(rfx_ssgi_trace, rfx_ssgi_params) PARAMS_FN(rfx_ssgi_shade, rfx_ssgi_params)
PARAMS_FN(rfx_temporal_reproject, rfx_temporal_params) PARAMS_FN(rfx_poisson_denoise, rfx_denoise_params) PARAMS_FN(rfx_compose, rfx_compose_params)
PARAMS_FN(rfx_final_compose, rfx_final_params) PARAMS_FN(rfx_motion_blur, rfx_motion_blur_params) PARAMS_FN(rfx_motion_blur_stage, rfx_motion_blur_params)
static napi_value params_call(napi_env env, napi_callback_info info) {
    const params_fn *d = (const params_fn *)call_data(env, info);
    napi_value a[2];
    any_params p;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !read_params(env, a[1], d->kind, d->js, &p)) return NULL;
    int rc = d->fn(c, &p);
    if (rc) return throw_rfx(env, c, d->c_name, rc);
    return NULL;
}
/* ... and the calls whose arguments are (ctx, n integers): get them, call, throw on rc.  One row of EXPORTS each (INTS) */
typedef struct { const char *c_name; size_t n; int (*fn)(rfx_ctx *, const int32_t *v); } ints_fn;
#define INTS_FN(fn, call) static int i_##fn(rfx_ctx *c, const int32_t *v) { (void)v; return call; }
INTS_FN(rfx_stage_flip, rfx_stage_flip(c)) INTS_FN(rfx_clear, rfx_clear(c, (rfx_tex)v[0])) INTS_FN(rfx_copy_framebuffer, rfx_copy_framebuffer(c, (rfx_tex)v[0]))
INTS_FN(rfx_build_environment_importance, rfx_build_environment_importance(c, v[0])) INTS_FN(rfx_set_row_window, rfx_set_row_window(c, v[0], v[1]))
INTS_FN(rfx_set_uv_model, rfx_set_uv_model(c, v[0])) INTS_FN(rfx_export_wait, rfx_export_wait(c, v[0])) INTS_FN(rfx_sync, rfx_sync(c))
INTS_FN(rfx_time_begin, rfx_time_begin(c)) INTS_FN(rfx_halo_exchange, rfx_halo_exchange(c, (rfx_tex)v[0], NULL, v[1], v[2]))
INTS_FN(rfx_allgather_history, rfx_allgather_history(c, (rfx_tex)v[0], NULL)) INTS_FN(rfx_comm_wait, rfx_comm_wait(c)) INTS_FN(rfx_peer_close, rfx_peer_close(c))
INTS_FN(rfx_comm_destroy, (rfx_comm_destroy(c), RFX_OK))  /* (its result was never reported) */
static napi_value ints_call(napi_env env, napi_callback_info info) {
    const ints_fn *d = (const ints_fn *)call_data(env, info);
    napi_value a[4];
    int32_t v[3] = {0, 0, 0};
    if (!get_args(env, info, 1 + d->n, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    for (size_t i = 0; i < d->n; i++) if (!get_int(env, a[1 + i], &v[i])) return NULL;
    int rc = d->fn(c, v);
    if (rc) return throw_rfx(env, c, d->c_name, rc);
    return NULL;
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

/* [a, b] */
static napi_value int_pair(napi_env env, int a, int b) {
    napi_value arr, e;
    NAPI_CALL(env, napi_create_array_with_length(env, 2, &arr));
    napi_create_int32(env, a, &e); napi_set_element(env, arr, 0, e);
    napi_create_int32(env, b, &e); napi_set_element(env, arr, 1, e);
    return arr;
}
/* heldRows(ctx, tex) -> [row0, rows] */
static napi_value n_held_rows(napi_env env, napi_callback_info info) {
    napi_value a[2];
    int32_t tex;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[1], &tex)) return NULL;
    int r0 = 0, n = 0;
    int rc = rfx_tex_held_rows(c, (rfx_tex)tex, &r0, &n);
    if (rc) return throw_rfx(env, c, "rfx_tex_held_rows", rc);
    return int_pair(env, r0, n);
}

/* ssgiTargetRows(ctx, resolutionScale) -> [row0, rows]: rfx_ssgi_target_rows */
static napi_value n_ssgi_target_rows(napi_env env, napi_callback_info info) {
    napi_value a[2];
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
    return int_pair(env, r0, n);
}

/* download (XFER[0]) / upload (XFER[1]) / stageUpload (XFER[2]) (ctx, tex, typedArray, row0, rows).  stageUpload: asynchronous copy into the slot's
 * back buffer (rfx.h "streaming dumps"); the array — ideally a view of hostAlloc() memory — must stay alive and unchanged until the flip that
 * publishes it has been synced */
static const int XFER[3] = {0, 1, 2};
static napi_value xfer(napi_env env, napi_callback_info info) {
    const int up = *(const int *)call_data(env, info);
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
static const int AOV_BYTES = 0, AOV_STAGE = 1;
static napi_value aov_call(napi_env env, napi_callback_info info) {
    const int stage = *(const int *)call_data(env, info);
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
/* The calls on an EXR frame, (ctx, bytes, parts, records, row0, rows): stageExrAov -> rfx_stage_exr_aov, `records` a Uint8Array of rfx_exr_chunk;
 * stageExrBlocks -> rfx_stage_exr_blocks (rfx.h "EXR blocks"), `records` of rfx_exr_block (imageio.exrAovLayout(..., { forms: "blocks" }));
 * stageExrBlocksPiz -> rfx_stage_exr_blocks_piz (rfx.h "EXR blocks with PIZ": a part's compression may also be 4).  `bytes` must stay alive and
 * unchanged like stageUpload's planes.  exrAovStageBytes / exrBlocksStageBytes / exrBlocksPizStageBytes(...) -> the bytes that call copies (0: it
 * would be refused).  The two descriptors differ in the record type alone: a form has either the chunk functions or the block ones. */
typedef struct {
    const char *c_name;
    size_t record;
    int (*stage_chunks)(rfx_ctx *, const rfx_exr_frame *, int, int);
    size_t (*bytes_chunks)(const rfx_ctx *, const rfx_exr_frame *, int, int);
    int (*stage_blocks)(rfx_ctx *, const rfx_exr_block_frame *, int, int);
    size_t (*bytes_blocks)(const rfx_ctx *, const rfx_exr_block_frame *, int, int);
} exr_form;
static const exr_form EXR_CHUNKS = {"rfx_stage_exr_aov", sizeof(rfx_exr_chunk), rfx_stage_exr_aov, rfx_exr_aov_stage_bytes, NULL, NULL};
static const exr_form EXR_BLOCKS = {"rfx_stage_exr_blocks", sizeof(rfx_exr_block), NULL, NULL, rfx_stage_exr_blocks, rfx_exr_blocks_stage_bytes};
static const exr_form EXR_PIZ = {"rfx_stage_exr_blocks_piz", sizeof(rfx_exr_block), NULL, NULL, rfx_stage_exr_blocks_piz, rfx_exr_blocks_piz_stage_bytes};
typedef struct { const exr_form *form; int stage; } exr_fn;
static napi_value exr_frame_call(napi_env env, napi_callback_info info) {
    const exr_fn *d = (const exr_fn *)call_data(env, info);
    const exr_form *form = d->form;
    napi_value a[6], out = NULL;
    int32_t row0, rows;
    rfx_exr_frame f;
    void *hold;
    if (!get_args(env, info, 6, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !get_int(env, a[4], &row0) || !get_int(env, a[5], &rows)) return NULL;
    if (!read_exr_frame(env, a[1], a[2], a[3], form->record, &f, &hold)) return NULL;
    const rfx_exr_block_frame b = {f.data, f.bytes, f.parts, f.chunks, f.part, (const rfx_exr_block *)hold};  /* (the records lead the block) */
    if (!d->stage) {
        const size_t n = form->bytes_blocks ? form->bytes_blocks(c, &b, row0, rows) : form->bytes_chunks(c, &f, row0, rows);
        free(hold);
        NAPI_CALL(env, napi_create_double(env, (double)n, &out));
        return out;
    }
    int rc = form->stage_blocks ? form->stage_blocks(c, &b, row0, rows) : form->stage_chunks(c, &f, row0, rows);
    free(hold);
    if (rc) return throw_rfx(env, c, form->c_name, rc);
    return NULL;
}
/* exrAovStatus(ctx) -> [bad chunks, first bad chunk, code] */
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
static const int PACK_GBUFFER = 0, PACK_VELOCITY = 1;
static napi_value n_pack(napi_env env, napi_callback_info info) {
    const int velocity = *(const int *)call_data(env, info);
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
    if (!read_params(env, a[1], P_MOTION_BLUR, "motionBlurReachMask", &p)) return NULL;
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
    if (!read_params(env, a[1], P_MOTION_BLUR, "motionBlurGather", &p)) return NULL;
    int rc = rfx_motion_blur_gather(c, &p, NULL, &got);
    if (rc) return throw_rfx(env, c, "rfx_motion_blur_gather", rc);
    napi_create_double(env, (double)got, &out);
    return out;
}

/* ---- the export calls (rfx.h "streamed frame export", "PNG fragments", "EXR fragments", "Match form"): one descriptor per kind of payload.
 * exportBytes / pngBound / exrBound(ctx, params) -> the bytes of a result buffer (0: bad params, or a format other than the kind's).
 * exportFrame(ctx, params, typedArray): rfx_export (blocks) / stageExport(...) -> ticket: rfx_stage_export — the array, ideally a view of
 * hostAlloc() memory, must stay alive until exportWait(ctx, ticket) has returned.  pngFrame / stagePng(ctx, params, filter, Uint8Array) and
 * exrFrame / stageExr(ctx, params, Uint8Array): the same with the result buffer of "PNG fragments" / "EXR fragments".  pngFrameEx / stagePngEx(ctx,
 * params, filter, flags, Uint8Array) and exrFrameEx / stageExrEx(ctx, params, flags, Uint8Array): the _ex entry points (flags = RFX_ENCODE_MATCHES
 * or 0).  The library checks the byte count. */
typedef struct {
    int has_filter, want_u8;        /* a `filter` argument after params; the array must be a Uint8Array */
    const char *js[2];              /* [staged]: the names in the type errors */
    const char *c_name[4];          /* [staged + 2 * ex] */
    size_t (*bound)(const rfx_ctx *, const rfx_export_params *);
    int (*call)(rfx_ctx *, const rfx_export_params *, int filter, int ex, unsigned flags, void *data, size_t bytes, int *ticket);  /* ticket NULL: blocks */
} encode_kind;
static int export_fn(rfx_ctx *c, const rfx_export_params *p, int filter, int ex, unsigned flags, void *d, size_t n, int *t) {
    (void)filter; (void)ex; (void)flags;
    return t ? rfx_stage_export(c, p, d, n, t) : rfx_export(c, p, d, n);
}
static int png_fn(rfx_ctx *c, const rfx_export_params *p, int filter, int ex, unsigned flags, void *d, size_t n, int *t) {
    if (ex) return t ? rfx_stage_png_ex(c, p, filter, flags, d, n, t) : rfx_png_ex(c, p, filter, flags, d, n);
    return t ? rfx_stage_png(c, p, filter, d, n, t) : rfx_png(c, p, filter, d, n);
}
static int exr_fn_(rfx_ctx *c, const rfx_export_params *p, int filter, int ex, unsigned flags, void *d, size_t n, int *t) {
    (void)filter;
    if (ex) return t ? rfx_stage_exr_ex(c, p, flags, d, n, t) : rfx_exr_ex(c, p, flags, d, n);
    return t ? rfx_stage_exr(c, p, d, n, t) : rfx_exr(c, p, d, n);
}
static const encode_kind ENC_EXPORT = {0, 0, {"exportFrame: TypedArray expected", "stageExport: TypedArray expected"},
                                       {"rfx_export", "rfx_stage_export", NULL, NULL}, rfx_export_bytes, export_fn};
static const encode_kind ENC_PNG = {1, 1, {"pngFrame: Uint8Array expected", "stagePng: Uint8Array expected"},
                                    {"rfx_png", "rfx_stage_png", "rfx_png_ex", "rfx_stage_png_ex"}, rfx_png_bound, png_fn};
static const encode_kind ENC_EXR = {0, 1, {"exrFrame: Uint8Array expected", "stageExr: Uint8Array expected"},
                                    {"rfx_exr", "rfx_stage_exr", "rfx_exr_ex", "rfx_stage_exr_ex"}, rfx_exr_bound, exr_fn_};
static napi_value bound_call(napi_env env, napi_callback_info info) {
    const encode_kind *k = (const encode_kind *)call_data(env, info);
    napi_value a[2], out;
    rfx_export_params p;
    if (!get_args(env, info, 2, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || !read_params(env, a[1], P_EXPORT, "", &p)) return NULL;
    NAPI_CALL(env, napi_create_double(env, (double)k->bound(c, &p), &out));
    return out;
}
typedef struct { const encode_kind *kind; int staged, ex; } encode_fn;
static napi_value encode_call(napi_env env, napi_callback_info info) {
    const encode_fn *d = (const encode_fn *)call_data(env, info);
    const encode_kind *k = d->kind;
    napi_value a[5], ab, out;
    napi_typedarray_type type;
    size_t len = 0, off = 0, at = 2;
    void *data = NULL;
    int32_t filter = 0, flags = 0;
    rfx_export_params p;
    if (!get_args(env, info, 3 + k->has_filter + d->ex, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c || (k->has_filter && !get_int(env, a[at++], &filter)) || (d->ex && !get_int(env, a[at++], &flags))) return NULL;
    if (!read_params(env, a[1], P_EXPORT, "", &p)) return NULL;
    bool is_ta = false;
    napi_is_typedarray(env, a[at], &is_ta);
    if (!is_ta || napi_get_typedarray_info(env, a[at], &type, &len, &data, &ab, &off) != napi_ok || !data || (k->want_u8 && type != napi_uint8_array)) {
        napi_throw_type_error(env, NULL, k->js[d->staged]);
        return NULL;
    }
    static const size_t esz[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
    int ticket = 0;
    int rc = k->call(c, &p, filter, d->ex, (unsigned)flags, data, len * esz[type], d->staged ? &ticket : NULL);
    if (rc) return throw_rfx(env, c, k->c_name[d->staged + 2 * d->ex], rc);
    if (!d->staged) return NULL;
    NAPI_CALL(env, napi_create_int32(env, ticket, &out));
    return out;
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

static napi_value n_halo_violations(napi_env env, napi_callback_info info) {
    napi_value a[1], out;
    if (!get_args(env, info, 1, a)) return NULL;
    rfx_ctx *c = get_ctx(env, a[0]);
    if (!c) return NULL;
    NAPI_CALL(env, napi_create_uint32(env, rfx_halo_violations(c), &out));
    return out;
}

/* timeEnd(ctx) -> ms since timeBegin(ctx) */
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

/* profile(ctx, enable) / profileRead(ctx) -> { ms, launches }: arrays of RFX_PROF_COUNT_ALL entries (rfx_profile, rfx_profile_read_n).
 * (profile is no INTS row: an `enable` that is no number throws here, where ints_call returns without a word) */
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

/* What the addon exports: the JS name, the callback, and for a callback that serves several names what this one selects (call_data).  DRAW,
 * INTS, ENCODE and EXR rows are whole functions: (ctx, params object), (ctx, n integers), the export calls, the calls on an EXR frame. */
#define DRAW(js, fn, kind) {js, params_call, &(const params_fn){js, #fn, kind, p_##fn}}
#define INTS(js, fn, n) {js, ints_call, &(const ints_fn){#fn, n, i_##fn}}
#define ENCODE(js, kind, staged, ex) {js, encode_call, &(const encode_fn){&kind, staged, ex}}
#define EXR(js, form, stage) {js, exr_frame_call, &(const exr_fn){&form, stage}}
static const struct { const char *name; napi_callback fn; const void *data; } EXPORTS[] = {
    {"abiVersion", n_abi_version, NULL}, {"create", n_create, NULL}, {"constants", n_constants, NULL}, {"paramBytes", n_param_bytes, NULL},
    {"heldRows", n_held_rows, NULL}, {"ssgiTargetRows", n_ssgi_target_rows, NULL},
    {"download", xfer, &XFER[0]}, {"upload", xfer, &XFER[1]}, {"stageUpload", xfer, &XFER[2]}, {"hostAlloc", n_host_alloc, NULL},
    INTS("stageFlip", rfx_stage_flip, 0), INTS("clear", rfx_clear, 1),
    {"stageAov", aov_call, &AOV_STAGE}, {"aovStageBytes", aov_call, &AOV_BYTES}, {"setAovConventions", n_set_aov_conventions, NULL},
    EXR("stageExrAov", EXR_CHUNKS, 1), EXR("exrAovStageBytes", EXR_CHUNKS, 0), EXR("stageExrBlocks", EXR_BLOCKS, 1), EXR("exrBlocksStageBytes", EXR_BLOCKS, 0),
    EXR("stageExrBlocksPiz", EXR_PIZ, 1), EXR("exrBlocksPizStageBytes", EXR_PIZ, 0), {"exrAovStatus", n_exr_aov_status, NULL},
    {"packGBuffer", n_pack, &PACK_GBUFFER}, {"packVelocity", n_pack, &PACK_VELOCITY},
    {"setEnvironment", n_set_environment, NULL}, {"setEnvironmentImportance", n_set_environment_importance, NULL}, {"cubeToEquirect", n_cube_to_equirect, NULL},
    {"setEnvironmentCube", n_set_environment_cube, NULL}, INTS("buildEnvironmentImportance", rfx_build_environment_importance, 1),
    {"downloadEnvironmentImportance", n_download_environment_importance, NULL},
    /* the draws: ssgiMarch in one launch, or as ssgiTrace + ssgiShade (only the second reads last frame's composed GI); copyFramebuffer(ctx, dstTex) is
     * renderer.copyFramebufferToTexture of TemporalReprojectPass.js:198-201; finalCompose SSGIEffect's own fragment; motionBlur MotionBlurEffect's (K6) ->
     * RFX_TEX_MOTION_BLUR; motionBlurStage a row tile's rows of the source into RFX_TEX_BLUR_SOURCE (arms the tiled draw) */
    DRAW("ssgiMarch", rfx_ssgi_march, P_SSGI), DRAW("ssgiTrace", rfx_ssgi_trace, P_SSGI), DRAW("ssgiShade", rfx_ssgi_shade, P_SSGI),
    DRAW("temporalReproject", rfx_temporal_reproject, P_TEMPORAL), INTS("copyFramebuffer", rfx_copy_framebuffer, 1),
    DRAW("poissonDenoise", rfx_poisson_denoise, P_DENOISE), DRAW("compose", rfx_compose, P_COMPOSE), DRAW("finalCompose", rfx_final_compose, P_FINAL),
    DRAW("motionBlur", rfx_motion_blur, P_MOTION_BLUR), DRAW("motionBlurStage", rfx_motion_blur_stage, P_MOTION_BLUR),
    {"motionBlurReachMask", n_motion_blur_reach_mask, NULL}, {"motionBlurGather", n_motion_blur_gather, NULL},
    /* setRowWindow(ctx, y0, y1): y1 <= y0 resets; setUvModel(ctx, model): 0 = RFX_UV_IDEAL, 1 = RFX_UV_REFERENCE_GL */
    INTS("setRowWindow", rfx_set_row_window, 2), INTS("setUvModel", rfx_set_uv_model, 1), INTS("sync", rfx_sync, 0),
    {"haloViolations", n_halo_violations, NULL}, INTS("timeBegin", rfx_time_begin, 0), {"timeEnd", n_time_end, NULL},
    {"profile", n_profile, NULL}, {"profileRead", n_profile_read, NULL},
    {"exportBytes", bound_call, &ENC_EXPORT}, ENCODE("exportFrame", ENC_EXPORT, 0, 0), ENCODE("stageExport", ENC_EXPORT, 1, 0), INTS("exportWait", rfx_export_wait, 1),
    {"pngBound", bound_call, &ENC_PNG}, ENCODE("pngFrame", ENC_PNG, 0, 0), ENCODE("stagePng", ENC_PNG, 1, 0),
    ENCODE("pngFrameEx", ENC_PNG, 0, 1), ENCODE("stagePngEx", ENC_PNG, 1, 1),
    {"exrBound", bound_call, &ENC_EXR}, ENCODE("exrFrame", ENC_EXR, 0, 0), ENCODE("stageExr", ENC_EXR, 1, 0),
    ENCODE("exrFrameEx", ENC_EXR, 0, 1), ENCODE("stageExrEx", ENC_EXR, 1, 1),
    /* row-tiled runs: haloExchange(ctx, tex, upRank, downRank) — -1 = no such neighbour */
    {"splitRows", n_split_rows, NULL}, {"commUniqueId", n_comm_unique_id, NULL}, {"commInit", n_comm_init, NULL}, INTS("haloExchange", rfx_halo_exchange, 3),
    INTS("allgatherHistory", rfx_allgather_history, 1), {"gatherHistoryRows", n_gather_history_rows, NULL}, INTS("commWait", rfx_comm_wait, 0),
    INTS("commDestroy", rfx_comm_destroy, 0), {"peerExport", n_peer_export, NULL}, {"peerOpen", n_peer_open, NULL},
    {"peerGatherHistory", n_peer_gather_history, NULL}, INTS("peerClose", rfx_peer_close, 0), {"ssgiHitMask", n_ssgi_hit_mask, NULL},
};

static napi_value init(napi_env env, napi_value exports) {
    const char *bad = table_that_misses_a_field();
    if (bad) {
        char msg[128];
        snprintf(msg, sizeof msg, "rfx_napi: the field table of \"%s\" does not cover its struct in include/rfx.h", bad);
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    for (size_t i = 0; i < sizeof EXPORTS / sizeof EXPORTS[0]; i++) {
        napi_value f;
        if (napi_create_function(env, EXPORTS[i].name, NAPI_AUTO_LENGTH, EXPORTS[i].fn, (void *)EXPORTS[i].data, &f) != napi_ok) return NULL;
        napi_set_named_property(env, exports, EXPORTS[i].name, f);
    }
    return exports;
}

NAPI_MODULE(rfx_napi, init)
