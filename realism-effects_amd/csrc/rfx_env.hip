// rfx_env.hip — the C ABI's one-off inputs: the importer's blocking packers (rfx_pack_gbuffer / rfx_pack_velocity, kernels in k0_import.hip), and
// scene.environment — its mip chain (k1_ssgi.hip rfx_launch_env_mip), its importance tables, the cube-to-equirect pass (k0_cube.hip) — and the
// environment's stream-ordered updates, which keep all of that on the device (rfx_set_environment_cube, rfx_build_environment_importance: K10).
#include "rfx_host.h"

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

// the importance tables of an environment, and the environment with them
static void env_tables_release(rfx_ctx *c) {
    if (c->env_marginal) hipFree(c->env_marginal);
    if (c->env_conditional) hipFree(c->env_conditional);
    c->env_marginal = c->env_conditional = nullptr;
    c->env_tab_cap[0] = c->env_tab_cap[1] = 0;
    c->env_tables_set = c->env_sums_on_device = false;
}
static void env_release(rfx_ctx *c) {
    if (c->env) hipFree(c->env);
    c->env = nullptr; c->env_w = c->env_h = c->env_levels = 0;
    c->env_cap = 0;
    env_tables_release(c);
}
// the mip chain of a width x height map: the levels' offsets in texels; returns the chain's texels
static size_t env_chain(int width, int height, unsigned int off[16], int *levels) {
    size_t total = 0;
    *levels = 0;
    for (int w = width, h = height;; w = w > 1 ? w >> 1 : 1, h = h > 1 ? h >> 1 : 1) {
        off[(*levels)++] = (unsigned int)total;
        total += (size_t)w * h;
        if (w == 1 && h == 1) break;
    }
    return total;
}
// levels 1 .. of the chain in c->env from level 0
static hipError_t env_mips(rfx_ctx *c, int width, int height, const unsigned int *off, int levels, bool to_half, bool rtz) {
    hipError_t e = hipSuccess;
    for (int l = 1, w = width, h = height; l < levels && e == hipSuccess; l++) {
        const int dw = w > 1 ? w >> 1 : 1, dh = h > 1 ? h >> 1 : 1;
        e = rfx_launch_env_mip(c->env + off[l - 1], c->env + off[l], w, h, dw, dh, to_half, rtz, c->stream);
        w = dw; h = dh;
    }
    return e;
}
// an area of the stream-ordered environment updates grows: the one wait of that path (draws queued on the stream may still read the area that goes)
static int env_grow(rfx_ctx *c, void **area, size_t *cap, size_t need, const char *what) {
    if (*cap >= need) return RFX_OK;
    if (*area) HIPCHK(c, hipStreamSynchronize(c->stream));
    return grow_idle(c, area, cap, need, what);
}

extern "C" {

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
    unsigned int off[16];
    const size_t total = env_chain(width, height, off, &levels);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    env_release(c);  // (the tables of the previous map too: a new one needs its own)
    hipError_t e = hipMalloc((void **)&c->env, total * sizeof(float4));
    if (e != hipSuccess) return fail(c, RFX_ENOMEM, "hipMalloc(environment)", e);
    c->env_cap = total * sizeof(float4);
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
    if (e == hipSuccess) e = env_mips(c, width, height, off, levels, halfFloatType != 0, halfStoreRTZ != 0);
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
    c->env_tab_cap[0] = (size_t)c->env_h * sizeof(float); c->env_tab_cap[1] = (size_t)c->env_w * c->env_h * sizeof(float);
    e = hipMemcpyAsync(c->env_marginal, marginal, (size_t)c->env_h * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->env_conditional, conditional, (size_t)c->env_w * c->env_h * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {  // tables with undefined contents must not pass the importanceSampling validation
        env_tables_release(c);
        return fail(c, RFX_EDEVICE, "rfx_set_environment_importance: copying the tables", e);
    }
    c->env_sum_whole = totalSumWhole; c->env_sum_decimal = totalSumDecimal;
    c->env_tables_set = true;
    return RFX_OK;
}

// ---- the stream-ordered updates: nothing below waits for the stream, frees or allocates when the sizes are those of the previous call
int rfx_set_environment_cube(rfx_ctx *c, const float *faces, int size, int generateMipmaps, int width, int height) {
    if (!c || !faces) return RFX_EINVAL;
    if (size < 1 || size > 8192) return fail(c, RFX_EINVAL, "rfx_set_environment_cube: face size must be 1..8192");
    if (width < 1 || height < 1 || width > 16384 || height > 16384 || (width & (width - 1)) || (height & (height - 1)))
        return fail(c, RFX_EINVAL, "rfx_set_environment_cube: width and height must be powers of two <= 16384");
    RFX_ENTER(c);
    int cube_levels = 1, levels = 0;
    size_t nchain = (size_t)6 * size * size;
    if (generateMipmaps)
        for (int s = size >> 1; s >= 1; s >>= 1) { nchain += (size_t)6 * s * s; cube_levels++; }
    unsigned int off[16];
    const size_t total = env_chain(width, height, off, &levels);
    int rc;
    if ((rc = env_grow(c, &c->env_cube, &c->env_cube_cap, nchain * sizeof(float4), "rfx_set_environment_cube: hipMalloc(cube chain)"))) return rc;
    if ((rc = env_grow(c, &c->env_stage, &c->env_stage_cap, (size_t)width * height * sizeof(float4), "rfx_set_environment_cube: hipMalloc(equirect staging)"))) return rc;
    if (c->env_cap < total * sizeof(float4)) {  // the held environment goes with its buffer
        void *chain = c->env;
        c->env = nullptr; c->env_w = c->env_h = c->env_levels = 0;
        rc = env_grow(c, &chain, &c->env_cap, total * sizeof(float4), "rfx_set_environment_cube: hipMalloc(environment)");
        c->env = (float4 *)chain;
        if (rc) return rc;
    }
    if (!c->ev_env_copied) HIPCHK(c, hipEventCreateWithFlags(&c->ev_env_copied, hipEventDisableTiming));
    c->env_tables_set = false;  // a new map needs its own tables (their buffers stay)
    hipError_t e = hipMemcpyAsync(c->env_cube, faces, (size_t)6 * size * size * sizeof(float4), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipEventRecord(c->ev_env_copied, c->stream);
    float4 *stage = (float4 *)c->env_stage;
    if (e == hipSuccess) e = rfx_launch_cube_to_equirect((float4 *)c->env_cube, size, cube_levels, stage, width, height, rfx_uv_planes(c->uv_model, width, height), c->stream);
    // as rfx_set_environment(equirect, width, height, 0, 0): level 0 = the FloatType texels, then the chain
    if (e == hipSuccess) e = rfx_launch_env_mip(stage, c->env, width, height, width, height, false, false, c->stream);
    if (e == hipSuccess) e = env_mips(c, width, height, off, levels, false, false);
    if (e == hipSuccess) e = hipEventSynchronize(c->ev_env_copied);  // the caller may reuse `faces` as soon as we return
    if (e != hipSuccess) {
        c->env_w = c->env_h = c->env_levels = 0;  // no environment: a half-built chain is not drawn from
        hipStreamSynchronize(c->stream);
        env_release(c);
        return fail(c, RFX_EDEVICE, "rfx_set_environment_cube", e);
    }
    c->env_w = width; c->env_h = height; c->env_levels = levels;
    memcpy(c->env_off, off, sizeof off);
    return RFX_OK;
}

int rfx_build_environment_importance(rfx_ctx *c, int flipY) {
    if (!c) return RFX_EINVAL;
    if (!c->env) return fail(c, RFX_ESTATE, "rfx_build_environment_importance: no environment set");
    RFX_ENTER(c);
    const size_t nm = (size_t)c->env_h * sizeof(float), nc = (size_t)c->env_w * c->env_h * sizeof(float);
    int rc;
    c->env_tables_set = false;
    if ((rc = env_grow(c, (void **)&c->env_marginal, &c->env_tab_cap[0], nm, "rfx_build_environment_importance: hipMalloc(marginalWeights)"))) return rc;
    if ((rc = env_grow(c, (void **)&c->env_conditional, &c->env_tab_cap[1], nc, "rfx_build_environment_importance: hipMalloc(conditionalWeights)"))) return rc;
    if ((rc = env_grow(c, &c->env_k10, &c->env_k10_cap, rfx_env_tables_scratch_bytes(c->env_h), "rfx_build_environment_importance: hipMalloc(K10 scratch)"))) return rc;
    hipError_t e = rfx_launch_env_tables(c->env, c->env_w, c->env_h, flipY != 0, c->env_marginal, c->env_conditional, c->env_k10, c->stream);
    if (e != hipSuccess) return fail(c, RFX_EDEVICE, "rfx_build_environment_importance", e);
    c->env_tables_set = c->env_sums_on_device = true;
    return RFX_OK;
}

int rfx_download_environment_importance(rfx_ctx *c, float *marginal, float *conditional, double *totalSumValue, float *whole, float *decimal) {
    if (!c) return RFX_EINVAL;
    if (!c->env || !c->env_tables_set) return fail(c, RFX_ESTATE, "rfx_download_environment_importance: no importance tables set");
    RFX_ENTER(c);
    struct { double total; float whole, decimal; } s = {(double)c->env_sum_whole + (double)c->env_sum_decimal, c->env_sum_whole, c->env_sum_decimal};
    if (marginal) HIPCHK(c, hipMemcpyAsync(marginal, c->env_marginal, (size_t)c->env_h * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (conditional) HIPCHK(c, hipMemcpyAsync(conditional, c->env_conditional, (size_t)c->env_w * c->env_h * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (c->env_sums_on_device) HIPCHK(c, hipMemcpyAsync(&s, c->env_k10, sizeof s, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (totalSumValue) *totalSumValue = s.total;
    if (whole) *whole = s.whole;
    if (decimal) *decimal = s.decimal;
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

}  // extern "C"
