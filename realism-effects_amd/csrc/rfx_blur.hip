// rfx_blur.hip — the C ABI's K6: rfx_motion_blur and, for row-tiled contexts, its reach mask / stage (the gather is in rfx_comm.hip; the kernels
// in k6_motion_blur.hip)
#include "rfx_host.h"

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

extern "C" {

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

}  // extern "C"
