/*
 * rfx.h — C ABI of librfx_hip.so: the MI355X-native SSGI hot path
 * (SSGI ray-march -> TemporalReprojectPass -> PoissonDenoisePass -> DenoiserComposePass).
 *
 * Drop-in boundary.  In the reference every pass is a postprocessing `Pass` whose only
 * device-side operation is
 *      renderer.setRenderTarget(rt); renderer.render(this.scene, this.camera)
 * with the arithmetic defined by the pass's `fullscreenMaterial` (GLSL + uniforms + defines):
 *      src/ssgi/pass/SSGIPass.js:93-94                          -> rfx_ssgi_march
 *      src/temporal-reproject/TemporalReprojectPass.js:192-193  -> rfx_temporal_reproject
 *      src/denoise/pass/PoissonDenoisePass.js:146-147           -> rfx_poisson_denoise
 *      src/denoise/pass/DenoiserComposePass.js:133-134          -> rfx_compose
 * plus the one non-draw device operation on the path,
 *      renderer.copyFramebufferToTexture(...)  TemporalReprojectPass.js:198-201  -> rfx_copy_framebuffer
 *      (the pass's own history when no override textures are set: TRAAEffect, src/traa/TRAAEffect.js:52-75).
 * Each entry point below replaces exactly one of those calls.  The `*_params` structs
 * carry what the material's `uniforms` (run-time values) and `defines` (shader variants)
 * carried; textures are addressed by slot id (`rfx_tex`), the analogue of the
 * `WebGLRenderTarget.texture` objects the passes share by reference (Denoiser.js:45,51).
 *
 * Conventions
 *   - plain C, no exceptions: every call returns 0 (RFX_OK) or a negative RFX_E* code;
 *     rfx_last_error(ctx) gives the message (the reference signals nothing, GL errors only
 *     surface on the console).
 *   - images are row-major, row 0 = BOTTOM (GL / `vUv` convention), tightly packed.
 *   - matrices are column-major float[16], i.e. three.js `Matrix4.elements`.
 *   - one context per device; calls enqueue on the context's HIP stream and return;
 *     rfx_sync() blocks.  A context may own only a horizontal band ("tile") of the frame:
 *     rows [tile_y0, tile_y0 + tile_rows) are written, textures additionally hold
 *     `halo_rows` rows above and below (clipped to the frame) for the gathers
 *     (SURVEY.md §8e).  Row indices in every call are FRAME rows.
 *   - device buffers are owned by the library unless bound with rfx_bind_external().
 *   - threading: a context is driven by ONE host thread at a time (the reference drives its passes from the JS main thread); different contexts
 *     may be driven from different threads.  The only state the library shares between contexts are per-device caches of launch constants
 *     (the occupancy figure K1's persistent grid is sized with, the dynamic-LDS attribute of K3's kernels) and the RCCL binding: two threads that
 *     first use a kernel specialisation at the same moment both compute and store the SAME value — an unsynchronised but idempotent write.
 */
#ifndef RFX_H
#define RFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFX_ABI_VERSION 21

enum {
    RFX_OK = 0,
    RFX_EINVAL = -1,   /* bad argument / unsupported option combination */
    RFX_ENOMEM = -2,   /* device allocation failed */
    RFX_EDEVICE = -3,  /* HIP runtime error (no device, launch failure, ...) */
    RFX_ESTATE = -4,   /* texture not uploaded / wrong size */
    RFX_EUNSUPPORTED = -5
};

/* Texture slots.  Formats follow SURVEY.md Appendix B (the reference's render-target formats,
 * which parity dictates for every intermediate). */
typedef enum rfx_tex {
    RFX_TEX_DEPTH = 0,      /* R32F      GBufferPass depth texture (GBufferPass.js:42-44)           */
    RFX_TEX_GBUFFER,        /* RGBA32F   packed material (gbuffer_packing.glsl:166-178)             */
    RFX_TEX_VELOCITY,       /* RGBA32F   VelocityDepthNormalPass output (…Material.js:76-83,186-188)*/
    RFX_TEX_DIRECT_LIGHT,   /* RGBA32F   composer input buffer = direct lighting (SSGIEffect.js:396)*/
    RFX_TEX_BLUE_NOISE,     /* RGBA8 128x128, repeat (BlueNoiseUtils.js:9-15), already flipY'd      */
    RFX_TEX_SSGI,           /* RGBA32F   K1 out: 8 halfs {diffuse.rgb,roughness | specular.rgb,rayLength} */
    RFX_TEX_TEMPORAL0,      /* RGBA32F   K2 out 0 (diffuse), .a = age                               */
    RFX_TEX_TEMPORAL1,      /* RGBA32F   K2 out 1 (specular)                                        */
    RFX_TEX_DENOISE_A0,     /* RGBA16F   K3 ping-pong target A                                      */
    RFX_TEX_DENOISE_A1,
    RFX_TEX_DENOISE_B0,     /* RGBA16F   K3 ping-pong target B = K2 history = K4 input              */
    RFX_TEX_DENOISE_B1,
    RFX_TEX_COMPOSE,        /* RGBA32F   K4 out = next frame's K1 `accumulatedTexture`              */
    RFX_TEX_FBCOPY_F16,     /* RGBA16F linear   TemporalReprojectPass.framebufferTexture (:137-142) when the pass's    */
    RFX_TEX_FBCOPY_F32,     /* RGBA32F linear   input / render target is HalfFloatType resp. FloatType (:66,139-140)   */
    RFX_TEX_FINAL,          /* RGBA32F   SSGIEffect's own fragment (ssgi_compose.frag mainImage): the effect's output colour */
    RFX_TEX_COMPOSE_RGB,    /* RGB32F    .rgb of RFX_TEX_COMPOSE as 12-byte texels, held whole: the part of `accumulatedTexture` K1 reads,
                               kept beside it (rfx_compose_params.writeHistoryRGB) so that a row-tiled run all-gathers 12 B/px, not 16 */
    RFX_TEX_EFFECT_INPUT,   /* RGBA32F   (ABI 20) a host-filled effect input buffer: what an EffectPass reads as `inputBuffer` when it
                               does not come out of an earlier draw (a downloaded frame, TRAA's input plane ...); rfx_motion_blur */
    RFX_TEX_MOTION_BLUR,    /* RGBA32F   (ABI 20) MotionBlurEffect's output colour (rfx_motion_blur)                              */
    RFX_TEX_BLUR_SOURCE,    /* RGBA32F   (ABI 21) the plane a ROW-TILED rfx_motion_blur takes its taps from, held WHOLE like RFX_TEX_COMPOSE (frame
                               row y at y * W): the tile's own rows of the source (rfx_motion_blur_stage) plus the foreign texels the streaks
                               reach (rfx_motion_blur_gather, or rfx_upload by a host with its own transport).  Allocated on first use: a
                               whole-frame context and a run without motion blur never pay for it.  Not checkpoint state: rewritten before
                               every draw that reads it */
    RFX_TEX_COUNT
} rfx_tex;

/* What the passes read from `this._camera` each frame. */
typedef struct rfx_camera {
    float projectionMatrix[16];
    float projectionMatrixInverse[16];
    float matrixWorld[16];        /* cameraMatrixWorld */
    float matrixWorldInverse[16]; /* viewMatrix        */
    float position[3];            /* cameraPos (TemporalReprojectPass.js:98) */
    float near_, far_;
    int32_t isPerspective;        /* camera.isPerspectiveCamera -> the PERSPECTIVE_CAMERA define of every pass (1), else the orthographic depth -> view-Z variants (0) */
} rfx_camera;

/* K1 — SSGIMaterial uniforms/defines (src/ssgi/material/SSGIMaterial.js:15-51,
 * SSGIPass.js:38-40,82-91, SSGIEffect.js:143-151,203-226,254-258). */
typedef struct rfx_ssgi_params {
    rfx_camera camera;
    int32_t steps;            /* #define steps        (default 20) */
    int32_t refineSteps;      /* #define refineSteps  (default 5)  */
    int32_t mode;             /* #define mode: 0 = MODE_SSGI (two packed vec4 of halfs), 1 = MODE_SSR (raw vec4: specular GI, packHalf2x16(rayLength, roughness)) */
    int32_t useDirectLight;   /* #define useDirectLight */
    int32_t missedRays;       /* #define missedRays   */
    int32_t importanceSampling; /* #define importanceSampling (env-map MIS, ssgi.frag:197-216): needs useEnvMap and the tables of
                                 rfx_set_environment_importance                                                              */
    int32_t useEnvMap;        /* #define USE_ENVMAP: the context holds scene.environment (rfx_set_environment); missed rays and
                                 the screen-border fade take its colour instead of black (getEnvColor, ssgi.frag:311-346)   */
    float rayDistance;        /* uniform rayDistance = options.distance */
    float thickness;
    float envBlur;            /* uniform envBlur: mip = envBlur * maxEnvMapMipLevel (ssgi.frag:322); unused without USE_ENVMAP */
    int32_t blueNoiseIndex;   /* uniform blueNoiseIndex (BlueNoiseUtils.js:24-32 recurrence, host side) */
    float resolutionScale;    /* SSGIPass.setSize (SSGIPass.js:52-57): the pass renders into a (W*s) x (H*s) target and `resolution` is that size;
                                 0 is read as 1.  W*s and H*s must be whole numbers (RFX_EINVAL otherwise).  The target's texels are
                                 stored row-major at the start of RFX_TEX_SSGI (pitch W*s): every row on a whole-frame context, the
                                 rows rfx_ssgi_target_rows names on a row tile (see there for the layout and the halo rule).         */
    int32_t historySource;    /* uniform accumulatedTexture = ssgiEffect.denoiser.texture (SSGIPass.js:89, Denoiser.js:67-78):
                                 0  denoiseMode "full" / "full_temporal": K4's output, RFX_TEX_COMPOSE;
                                 1  "temporal": K2's texture[0], RFX_TEX_TEMPORAL0 (whole-frame contexts only);
                                 2  "denoised": the getter returns an ARRAY of textures, which three binds as its empty
                                    texture -> every history fetch reads (0,0,0,0);
                                 3  as 0, read from RFX_TEX_COMPOSE_RGB (same values: rfx_compose_params.writeHistoryRGB)    */
} rfx_ssgi_params;

/* K2 — TemporalReprojectMaterial uniforms/defines (TemporalReprojectPass.js:76-117,162-214). */
typedef struct rfx_temporal_params {
    rfx_camera camera;
    rfx_camera prevCamera;        /* prevViewMatrix, prevCameraMatrixWorld, prevProjectionMatrix(+Inverse), prevCameraPos */
    int32_t textureCount;         /* 2 (diffuseSpecular) or 1 */
    int32_t inputType;            /* 0 DIFFUSE_SPECULAR, 1 DIFFUSE, 2 SPECULAR */
    int32_t reprojectSpecular[2]; /* define bool[] */
    int32_t neighborhoodClamp[2]; /* define bool[]; accepted, the shader never reads it (Appendix D-6) */
    int32_t logTransform;
    int32_t fullAccumulate;       /* uniform: option && !didCameraMove */
    float confidencePower;        /* define, toPrecision(5) */
    float neighborhoodClampIntensity;
    float maxBlend;
    float keepData;               /* 0 for the first frame after reset(), else 1 */
    int32_t historySource;        /* which textures `accumulatedTexture[i]` are (TemporalReprojectPass.js:148-151):
                                     0  overrideAccumulatedTextures = K3's target B, RFX_TEX_DENOISE_B0/B1 (Denoiser.js:51);
                                     1  the pass's own framebuffer copy RFX_TEX_FBCOPY_F16 (render-target type HalfFloatType);
                                     2  the same, RFX_TEX_FBCOPY_F32 (FloatType).  With two textures (denoiseMode
                                        "full_temporal" / "temporal") BOTH read the one copy, which holds colour attachment 0
                                        = texture 0: copyFramebufferToTexture reads the framebuffer's read buffer.            */
    int32_t targetHalf;           /* render target type = type of the input texture (:63-68): 0 FloatType — texels stored as
                                     computed; 1 HalfFloatType — every output channel is rounded to half precision on store
                                     (RFX_TEX_TEMPORAL* then hold half-representable floats)                                 */
    int32_t halfStoreRTZ;         /* rounding of that store: 1 truncate (llvmpipe, parity with the oracle), 0 nearest-even    */
    int32_t inputWidth, inputHeight; /* size of `inputTexture` when it is smaller than the frame (K1 drawn with resolutionScale < 1:
                                     the pass samples it NEAREST at full-resolution vUv, TemporalReprojectPass.js:118); 0 = frame size */
} rfx_temporal_params;

/* K3 — PoissonDenoisePass uniforms/defines (PoissonDenoisePass.js:43-71, SSGIEffect.js:175-190). */
typedef struct rfx_denoise_params {
    float radius, phi, lumaPhi, depthPhi, normalPhi, roughnessPhi, specularPhi;
    int32_t textureCount;          /* 2 or 1 */
    int32_t isTextureSpecular[2];  /* define bool[2] */
    int32_t blueNoiseIndex;        /* advances once per draw */
    int32_t inputIsTemporal;       /* 1: inputs = RFX_TEX_TEMPORAL* (RGBA32F, nearest) — pass 0;
                                      0: inputs = the other ping-pong target (RGBA16F, linear)   */
    int32_t writeToB;              /* 0: render into A (even pass index), 1: into B (odd)       */
    int32_t halfStoreRTZ;          /* 1: RGBA16F stores truncate like llvmpipe's colour-buffer
                                         store (parity with the oracle); 0: round-to-nearest-even
                                         like GPU ROPs                                          */
} rfx_denoise_params;

/* K4 — DenoiserComposePass uniforms/defines (DenoiserComposePass.js:87-110). */
typedef struct rfx_compose_params {
    rfx_camera camera;
    int32_t inputType; /* 0 TYPE_DIFFUSE_SPECULAR; 2 TYPE_SPECULAR (diffuse component = sceneTexture = RFX_TEX_DIRECT_LIGHT, specular GI = B0) */
    int32_t giSource;  /* composerInputTextures (Denoiser.js:53): 0 the denoise pass's textures, RFX_TEX_DENOISE_B0/B1 (RGBA16F);
                          1 denoiseMode "full_temporal": K2's textures, RFX_TEX_TEMPORAL0/1 (RGBA32F, nearest) */
    int32_t writeHistoryRGB; /* 1: also keep RFX_TEX_COMPOSE_RGB = .rgb of every tile texel of RFX_TEX_COMPOSE (discarded background
                                fragments copy what the target holds), for rfx_ssgi_params.historySource 3 */
} rfx_compose_params;

/* SSGIEffect's own fragment — FinalSSGIMaterial uniforms/defines (SSGIEffect.js:34-66,404-417; src/ssgi/shader/ssgi_compose.frag). */
typedef struct rfx_final_params {
    rfx_camera camera;     /* cameraNear / cameraFar / PERSPECTIVE_CAMERA (only read when fog is on) */
    int32_t isDebug;       /* uniform isDebug: output = inputTexture texel, unmodified */
    int32_t inputSource;   /* uniform inputTexture = outputTexture[0] ?? outputTexture = denoiser.texture (SSGIEffect.js:139,402):
                              0 RFX_TEX_COMPOSE ("full", "full_temporal"); 1 RFX_TEX_TEMPORAL0 ("temporal"); 2 RFX_TEX_DENOISE_B0 ("denoised") */
    int32_t fogMode;       /* 0: scene.fog unset; 1: THREE.Fog (USE_FOG); 2: THREE.FogExp2 (USE_FOG + FOG_EXP2) */
    float fogColor[3];
    float fogNear, fogFar; /* fogMode 1 */
    float fogDensity;      /* fogMode 2 */
} rfx_final_params;

/* K6 — MotionBlurEffect (ABI 20): src/motion-blur/MotionBlurEffect.js:14-66,85-101 (uniforms / defines) and the effect's mainImage,
 * src/motion-blur/shader/motion_blur.frag:11-45, with the blue noise of src/utils/shader/blue_noise.glsl:37-45.  Per fragment:
 *   v = velocityTexture(vUv).xy (NEAREST, RFX_TEX_VELOCITY); dot(v, v) > 1e-9 is false (NaN included): output = inputColor.  Else
 *   v *= intensity; jitterOffset = jitter * v * blueNoise(vUv, frame).xy; frameSpeed = 0.01 / deltaTime;
 *   start = max(0, vUv + (jitterOffset - v * 0.5) * frameSpeed), end = min(1, vUv + (jitterOffset + v * 0.5) * frameSpeed);
 *   rgb = (inputColor.rgb + sum_{i=0..samples} inputTexture(mix(start, end, i / samples)).rgb) / (samples + 2)  (LINEAR taps);
 *   alpha = inputColor.a.
 * `inputColor` is what postprocessing's EffectMaterial hands the effect's mainImage: in the effect's own EffectPass the LINEAR fetch of the
 * pass's input buffer at vUv (the same slot as the taps); in the reference's README form EffectPass(camera, traaEffect, motionBlurEffect),
 * TRAA's output, traa_compose.frag: the NEAREST texel of RFX_TEX_TEMPORAL0 (TemporalReprojectPass.js:66-67) with alpha 1, while the taps
 * read the pass's input buffer (the plane TRAA's K2 took as its input: RFX_TEX_SSGI in both hosts).  Writes RFX_TEX_MOTION_BLUR.
 * A streak can reach anywhere on screen: a row-tiled context draws only after rfx_motion_blur_stage or rfx_motion_blur_gather armed it for
 * `source` (below), and gets RFX_EUNSUPPORTED otherwise.  Honours rfx_set_row_window and rfx_set_uv_model.  RFX_ESTATE when a host-filled input (RFX_TEX_VELOCITY, RFX_TEX_BLUE_NOISE, RFX_TEX_DIRECT_LIGHT, RFX_TEX_EFFECT_INPUT)
 * was never uploaded, packed, staged or bound, or a drawn one (RFX_TEX_FINAL, RFX_TEX_TEMPORAL0, RFX_TEX_SSGI) holds nothing yet. */
typedef struct rfx_motion_blur_params {
    int32_t source;         /* the taps' `inputTexture`: RFX_TEX_FINAL, RFX_TEX_TEMPORAL0, RFX_TEX_DIRECT_LIGHT, RFX_TEX_SSGI or RFX_TEX_EFFECT_INPUT
                               (each read as RGBA32F) */
    int32_t center;         /* the slot `inputColor` comes from.  -1: the effect's own EffectPass, the LINEAR fetch of `source` at vUv (a
                               `source` of RFX_TEX_TEMPORAL0 then stands for the buffer TRAA's own EffectPass wrote: pass centerAlphaOne 1).
                               An explicit slot is read with the reference's filter: NEAREST for RFX_TEX_TEMPORAL0 (TRAA's NearestFilter
                               target, the README form), LINEAR at vUv for the others */
    int32_t centerAlphaOne; /* 1: inputColor.a = 1 (traa_compose.frag:6 wrote it); 0: the centre's own alpha */
    int32_t samples;        /* #define samples, in [1, 65536] (default 16; fixed at construction, MotionBlurEffect.js:37-40) */
    float intensity;        /* uniform intensity (default 1) */
    float jitter;           /* uniform jitter (default 1) */
    float deltaTime;        /* uniform deltaTime: the host passes max(1/1000, deltaTime) (:89); finite and > 0 */
    int32_t frame;          /* uniform frame: renderer.info.render.frame % 4096 (:91); blueNoise's index, 0 = the unshifted table */
    float resolution[2];    /* uniform resolution: window.innerWidth / innerHeight (:94): the blue-noise pixel grid; finite, in (0, 65536] */
    int32_t targetHalf;     /* 1: the composer's buffers are HalfFloatType: the output is rounded to half precision on store */
    int32_t halfStoreRTZ;   /* rounding of that store: 1 truncate (llvmpipe), 0 nearest-even */
} rfx_motion_blur_params;

/* K7 — streamed frame export: the importer run in reverse.  The context's tile rows [tile_y0, tile_y0 + tile_rows) of an RGBA32F slot
 * are encoded ON THE DEVICE into a tightly packed interleaved stream — frame row order, row 0 = bottom, no pitch padding, no flip: the order
 * rfx_download uses — and only the encoded bytes cross PCIe: 3 B/px for a display image instead of the 16 B/px of rfx_download.
 *   RFX_EXPORT_F32      4 B per element: the source's bits, unchanged
 *   RFX_EXPORT_F16      2 B: IEEE binary16, round to nearest even; overflow -> +-inf, NaN stays NaN, subnormal halfs are produced
 *   RFX_EXPORT_U8_SRGB  1 B: the display encoding of rfx_amd/imageio.py tonemap(linear, operator, exposure) (js/imageio.js mirrors it), in fp32:
 *                       NaN -> 0, +inf -> 65504, -inf -> 0, clip to [0, 65504], times `exposure`; operator 0 "linear" / 1 "aces" (three's
 *                       ACESFilmicToneMapping: / 0.6, input matrix, rational fit, output matrix); NaN -> 0, inf -> 1, clip to [0, 1]; the sRGB
 *                       transfer function (branch at 0.0031308); (s * 255 + 0.5) truncated.  A fourth channel is alpha: NaN -> 0, clip to
 *                       [0, 1], (a * 255 + 0.5) truncated — no operator, no transfer function.
 * rfx_set_row_window does not apply: an export always covers the tile rows. */
enum { RFX_EXPORT_F32 = 0, RFX_EXPORT_F16 = 1, RFX_EXPORT_U8_SRGB = 2 };
typedef struct rfx_export_params {
    int32_t source;    /* RFX_TEX_FINAL, RFX_TEX_MOTION_BLUR, RFX_TEX_COMPOSE, RFX_TEX_TEMPORAL0, RFX_TEX_DIRECT_LIGHT or RFX_TEX_EFFECT_INPUT */
    int32_t format;    /* RFX_EXPORT_F32 / _F16 / _U8_SRGB */
    int32_t channels;  /* 3 (.rgb) or 4 (.rgba) */
    int32_t tonemap;   /* U8_SRGB only: 0 linear, 1 ACES filmic; must be 0 otherwise */
    float exposure;    /* U8_SRGB only: finite, >= 0.  Otherwise not given: 0 (a zeroed struct) or 1 (the hosts' default) */
} rfx_export_params;

typedef struct rfx_ctx rfx_ctx;

/* ---- lifetime (Pass ctor / setSize / dispose) */
int rfx_abi_version(void);
rfx_ctx *rfx_create(int device, int width, int height, int tile_y0, int tile_rows, int halo_rows);
void rfx_destroy(rfx_ctx *);
const char *rfx_last_error(const rfx_ctx *);
/* Geometry the context was created with (any out pointer may be NULL). */
int rfx_get_geometry(const rfx_ctx *, int *width, int *height, int *tile_y0, int *tile_rows, int *halo_rows);
/* Run the context's kernels on a caller-provided hipStream_t (e.g. a stream the framework also uses for its
 * collectives, so that they are ordered against the kernels); NULL restores the context's own stream.  The legacy
 * default stream has handle 0 == NULL and therefore cannot be selected: create a stream.  Switching drains the
 * stream used so far (its uploads and zero-fills must not race kernels on the new one): set it once, not per frame. */
int rfx_set_stream(rfx_ctx *, void *hip_stream);
/* Restrict the rows the following draws PRODUCE to frame rows [y0, y1) (intersected with what each draw would produce anyway);
 * y1 <= y0 resets.  Every pixel's result is independent of how the rows are split over launches, so a row-tiled run can draw the
 * interior of its tile while the halo rows of the input are still being exchanged, then the two boundary strips (rfx_amd/tiling.py).
 * Draws whose window is empty return RFX_OK without launching.  Ignored by rfx_ssgi_* with resolutionScale != 1, on whole-frame and
 * row-tiled contexts alike: the smaller target is always drawn whole (rfx_ssgi_target_rows), and rfx_temporal_reproject under a window
 * reads target rows that draw has left regardless. */
int rfx_set_row_window(rfx_ctx *, int y0, int y1);
/* Which vUv the draws' fragments see (every full-screen pass of the reference reads its inputs at the interpolated varying vUv,
 * src/utils/shader/basic.vert; e.g. ssgi.frag:107, temporal_reproject.frag:118, poisson_denoise.frag:128, DenoiserComposePass.js:58).
 *   RFX_UV_REFERENCE_GL  (default since ABI 15) the value the rasteriser of the reference's GL (Mesa llvmpipe, the oracle of the parity
 *                        tests) interpolates, bit for bit: three's full-screen triangle is clipped into two triangles along the frame
 *                        diagonal, each with its own fp32 plane equations (up to 2^-24 from the ideal value, different on either side of
 *                        the diagonal).  With it the NEAREST taps of the denoiser and every LINEAR fetch at vUv land where the
 *                        reference's land: what is left between the two implementations is transcendental rounding alone.
 *   RFX_UV_IDEAL         (i + 0.5) / n, correctly rounded: the value the shader authors mean, and what a GL that does not clip the
 *                        triangle is closest to.  Costs two IEEE divisions per fragment instead of an fma.
 * Applies to every following draw; row-tiled contexts evaluate the whole frame's planes. */
enum { RFX_UV_IDEAL = 0, RFX_UV_REFERENCE_GL = 1 };
int rfx_set_uv_model(rfx_ctx *, int model);
/* (ABI 17-18 had rfx_set_compose_fold: the compose draw made inside the last denoise launch from the texel just stored — an approximation of
 * the reference's LINEAR fetch.  Removed in ABI 19: an exact fold needs a second launch for the tile-edge pixels and saves at most 0.008 ms of
 * a 1.25 ms 4K frame before its LDS exchange is paid for (profiles/r06_k4/exact_fold_bounds.txt), and the library keeps ONE parity contract:
 * one launch per draw, exactly the reference's fetches.) */

/* ---- textures.  `row0`/`rows` are FRAME rows of the band being transferred; the band must lie
 * inside the rows the context holds: [max(0,tile_y0-halo), min(H,tile_y0+tile_rows+halo)).
 * Read-only full-frame inputs of K1 (depth, compose history) are always held whole. */
size_t rfx_tex_texel_bytes(rfx_tex id);
int rfx_tex_held_rows(const rfx_ctx *, rfx_tex id, int *row0, int *rows);
int rfx_upload(rfx_ctx *, rfx_tex id, const void *host, int row0, int rows);
int rfx_download(rfx_ctx *, rfx_tex id, void *host, int row0, int rows);
int rfx_clear(rfx_ctx *, rfx_tex id); /* zero-fill (render targets start zeroed) */
/* Device pointer of the first HELD row of a slot (for halo exchange / zero-copy interop).  Work the caller enqueues on the buffer must be
 * ordered against the context's draw stream (rfx_set_stream).  Taking RFX_TEX_DEPTH's pointer also moves K1's depth pre-pass from its own
 * stream into the draw stream for the rest of the context's life, exactly as rfx_bind_external(RFX_TEX_DEPTH) does. */
void *rfx_tex_device_ptr(rfx_ctx *, rfx_tex id);
/* Use caller-owned device memory (held-rows x width x texel bytes) for a slot. */
int rfx_bind_external(rfx_ctx *, rfx_tex id, void *device_ptr);

/* ---- importer: engine-side attribute planes (AOVs) instead of pre-packed dumps.  The two calls stand where the raster passes' fragment
 * epilogues pack their render targets (GBufferMaterial.js:84-89 `packGBuffer(diffuseColor, worldNormal, roughnessFactor, metalnessFactor,
 * totalEmissiveRadiance)`; VelocityDepthNormalMaterial.js:76-83,186-188 `vec4(vel.xy, packNormal(worldNormal), fragCoordZ)`) and fill rows
 * [row0, row0+rows) of RFX_TEX_GBUFFER / RFX_TEX_VELOCITY on the device (encode side of gbuffer_packing.glsl).  Planes are host pointers to
 * `rows` x width tightly packed float32 texels, row 0 of the band first (bottom up).  Texels with depth == 1 keep the passes' clear colour
 * (0, 0, 0, 1) (GBufferPass.js:103-105). */
typedef struct rfx_aov_gbuffer {
    const float *diffuse;    /* RGBA  diffuseColor (material colour x map, alpha)                     */
    const float *normal;     /* xyz   WORLD-space normal (normalised by the producer; re-scaled by the oct encoder) */
    const float *roughness;  /* 1     roughnessFactor                                                 */
    const float *metalness;  /* 1     metalnessFactor                                                 */
    const float *emissive;   /* rgb   totalEmissiveRadiance                                           */
    const float *depth;      /* 1     gl_FragCoord.z, 1.0 = not covered; may be NULL (every texel covered) */
} rfx_aov_gbuffer;
typedef struct rfx_aov_velocity {
    const float *velocity;   /* xy    uv-space motion: pos1 - pos0 with pos = clip.xy / clip.w * .5 + .5 (VelocityDepthNormalMaterial.js:76-80) */
    const float *normal;     /* xyz   WORLD-space normal                                              */
    const float *depth;      /* 1     gl_FragCoord.z, 1.0 = not covered                               */
} rfx_aov_velocity;
int rfx_pack_gbuffer(rfx_ctx *, const rfx_aov_gbuffer *, int row0, int rows);
int rfx_pack_velocity(rfx_ctx *, const rfx_aov_velocity *, int row0, int rows);

/* ---- scene.environment (SSGIEffect.keepEnvMapUpdated, SSGIEffect.js:309-362): an equirectangular HDR map.  The effect
 * turns its mipmaps on (`generateMipmaps`, LinearMipMapLinearFilter / LinearFilter, :323-328) and K1 samples it with
 * textureLod(map, equirectDirectionToUv(dir), envBlur * maxEnvMapMipLevel).  rfx_set_environment takes the base level as
 * width x height RGBA float32 texels (row 0 = bottom, v = 0), rounds them to half precision when the texture's type is
 * HalfFloatType (`halfFloatType`, what RGBELoader produces), and builds the mip chain the way glGenerateMipmap does on
 * the oracle's GL: every level the 2x2 bilinear-centre average of the one above, lerp(.5, lerp(.5,a,b), lerp(.5,c,d)), stored
 * in the texture's type (half: `halfStoreRTZ` 1 truncates like llvmpipe, 0 rounds to nearest even).  width and height must
 * be powers of two (wrap: ClampToEdge, three's default for a DataTexture).  maxEnvMapMipLevel = floor(log2(max(w,h))) + 1
 * (src/ssgi/utils/Utils.js:30-34).  rfx_set_environment(ctx, NULL, 0, 0, 0, 0) removes it. */
int rfx_set_environment(rfx_ctx *, const float *rgba, int width, int height, int halfFloatType, int halfStoreRTZ);
/* The two inverse-CDF tables and the luminance sum that EquirectHdrInfoUniform.updateFrom computes on the CPU (a Web Worker in the
 * reference, src/ssgi/utils/EquirectHdrInfoUniform.js:148-245,365-400) for `sampleEquirectProbability` (ssgi_utils.frag:210-225):
 * `marginalWeights` (height floats: an height x 1 NEAREST texture), `conditionalWeights` (width x height floats, row-major), and
 * totalSumValue split as the reference splits it (`~~total` and the rest).  Sizes are those of the environment set before. */
int rfx_set_environment_importance(rfx_ctx *, const float *marginalWeights, size_t marginalCount, const float *conditionalWeights,
                                   size_t conditionalCount, float totalSumWhole, float totalSumDecimal);  /* counts in floats: RFX_EINVAL unless height / width*height */
/* Read mip level `level` of the environment back (max(w>>level,1) x max(h>>level,1) RGBA float32); *levels (may be NULL) receives the
 * number of levels.  For inspection and for checking the chain against the driver's. */
int rfx_download_environment(rfx_ctx *, int level, float *rgba, int *levels);
/* CubeToEquirectEnvPass.generateEquirectEnvMap's draw + read-back (src/ssgi/pass/CubeToEquirectEnvPass.js:21-42,78-85; called from
 * SSGIEffect.js:316-321 when scene.environment is a CubeTexture): `faces_rgba` = the six faces +X -X +Y -Y +Z -Z, each size x size RGBA
 * float32 (linear values), row j = t as handed to glTexImage2D; `equirect_rgba` receives width x height RGBA float32 texels (the pass's
 * FloatType render target as readRenderTargetPixels returns it: row 0 = bottom) — the DataTexture the effect then treats like any
 * equirectangular environment: hand it to rfx_set_environment(…, halfFloatType = 0) and build the importance tables from it.
 * generateMipmaps = 0: the cube is sampled LINEAR, seamless, at level 0 (minFilter LinearFilter: HDRCubeTextureLoader's set-up);
 * 1: three's CubeTexture default, LinearMipmapLinearFilter over the chain glGenerateMipmap builds (any size since round 6: an odd level is
 * reduced by the GL's bilinear blit, an even one by the 2x2 average it degenerates to), with the implicit level of detail of `textureCube`
 * (the pass minifies near the face edges: levels 0-2 take part). */
int rfx_cube_to_equirect(rfx_ctx *, const float *faces_rgba, int size, int generateMipmaps, float *equirect_rgba, int width, int height);
/* ---- the environment kept on the device (additive to ABI 21: a host checks for the symbols; the version number stands).  For an
 * environment that changes during a sequence — a CubeCamera probe, an animated sky — the three calls above cost two uploads, a read-back,
 * the table build on the host and four waits per change.  The two calls below are STREAM-ORDERED on the context's stream instead: a draw
 * queued before them reads the old environment, one queued after them the new one.  They do not synchronise the stream, and they neither
 * allocate nor free device memory when the sizes are those of the previous call (the context owns the chain, the cube's chain, the staging,
 * the tables and K10's scratch, and grows them on demand).  They mix freely with the blocking calls above, which behave as before.
 *
 * rfx_set_environment_cube = rfx_cube_to_equirect followed by rfx_set_environment(equirect, width, height, 0, 0) with the equirectangular
 * map never leaving the device: every level is byte-identical to the two-call form.  The rules are those two calls': size 1..8192, width
 * and height powers of two <= 16384 (RFX_EINVAL).  Its one wait is on an event behind the copy of `faces_rgba`, which the caller may reuse
 * on return.  Like rfx_set_environment it invalidates the importance tables: importanceSampling is refused until a build (or
 * rfx_set_environment_importance) has run.
 *
 * rfx_build_environment_importance runs K10 (csrc/k10_env_tables.hip) on level 0 of the held environment — whichever call set it — and sets
 * the two tables and the two sums: bit for bit what rfx_amd/envmap.py build_importance (js/envmap.js buildImportance) computes from the same
 * texels for every finite input.  `flipY`: the texture's flipY, i.e. the worker's lossy "un-flip" of the reversed rows is reproduced.
 * RFX_ESTATE when no environment is set.
 *
 * rfx_download_environment_importance reads the tables back for inspection (any pointer may be NULL; synchronises): marginal (height floats),
 * conditional (width x height), totalSumValue and its two parts.  RFX_ESTATE when no tables are set. */
int rfx_set_environment_cube(rfx_ctx *, const float *faces_rgba, int size, int generateMipmaps, int width, int height);
int rfx_build_environment_importance(rfx_ctx *, int flipY);
int rfx_download_environment_importance(rfx_ctx *, float *marginal, float *conditional, double *totalSumValue, float *whole, float *decimal);

/* ---- the four draws (+ the framebuffer copy and the effect's own fragment) */
int rfx_ssgi_march(rfx_ctx *, const rfx_ssgi_params *);
/* The same draw in two launches, for a row-tiled run: rfx_ssgi_trace runs the fragment up to the end of RayMarch/BinarySearch
 * (ssgi.frag:441-503) and keeps the rays' end state in context scratch (32 B per pixel); rfx_ssgi_shade finishes the fragment
 * (doSample's shading :385-439 and the output packing) from it.  Only the shading reads `accumulatedTexture` (RFX_TEX_COMPOSE or
 * RFX_TEX_TEMPORAL0, historySource) — gathered anywhere on screen — so the all-gather that refreshes it between frames may still be in
 * flight during the trace and has to have landed only before the shade (rfx_amd/tiling.py).  Same params for both calls; the
 * result in RFX_TEX_SSGI is bit-identical to rfx_ssgi_march's.  rfx_ssgi_shade without a pending trace: RFX_ESTATE. */
int rfx_ssgi_trace(rfx_ctx *, const rfx_ssgi_params *);
int rfx_ssgi_shade(rfx_ctx *, const rfx_ssgi_params *);
/* resolutionScale != 1 on a row tile (added to ABI 21 without a new version number: one more entry point and three refusals fewer, nothing an
 * existing caller sees differently; a host checks for the symbol).  rfx_temporal_reproject reads the (W*s) x (H*s) target NEAREST at the full-resolution vUv:
 * frame row gy takes target row iy(gy) = nearest(vUv.y(gy) * H*s).  Its neighbourhood reads +-2 frame rows around the tile, so a tile
 * context draws exactly the target rows [row0, row0 + rows) that the frame rows [tile_y0 - e, tile_y0 + tile_rows + e), e = min(halo_rows, 2),
 * clipped to the frame, map to — under the context's vUv model — and stores them from the START of RFX_TEX_SSGI with pitch W*s: the
 * whole-frame layout shifted by row0.  Neighbouring tiles draw overlapping target rows redundantly (a fragment depends on its own
 * coordinates and the per-draw blue-noise shift only: the overlap is bit-identical).  The trace -> shade hand-over, rfx_ssgi_hit_mask,
 * rfx_gather_history_rows and rfx_peer_gather_history follow the same rows.
 * Halo rule: a fragment of target row j fetches the G-buffer and the direct light of frame row nearest(vUv.y(j) * H) through the held band.
 * That row lies within ceil(1 / (2 s)) rows of a frame row that maps to j, so the band must hold 2 + ceil(1 / (2 s)) rows around the tile
 * (rfx_amd/tiling.py required_halo(resolution_scale=s)); a fetch outside the band is clamped and counted by rfx_halo_violations.  A tile whose
 * target rows do not fit the slot (held rows * W texels) is refused with RFX_EINVAL.
 * rfx_ssgi_target_rows reports row0 / rows for a scale: 0, H*s on a whole-frame context; the held band of RFX_TEX_SSGI at scale 1 (or 0).
 * W*s or H*s not whole: RFX_EINVAL.  A host downloads a tile's target rows as the first rows * W*s texels of the slot. */
int rfx_ssgi_target_rows(rfx_ctx *, float resolutionScale, int *row0, int *rows);
int rfx_temporal_reproject(rfx_ctx *, const rfx_temporal_params *);
/* renderer.copyFramebufferToTexture(tmpVec2, this.framebufferTexture), TemporalReprojectPass.js:198-201: the tile rows of
 * the pass's render target RFX_TEX_TEMPORAL0 become the history the NEXT rfx_temporal_reproject samples (linear filter).
 * `dst` is RFX_TEX_FBCOPY_F16 (source texels must be half-representable, i.e. drawn with targetHalf = 1: the copy is then
 * exact, as in the reference where both sides have the same type) or RFX_TEX_FBCOPY_F32. */
int rfx_copy_framebuffer(rfx_ctx *, rfx_tex dst);
/* One PoissonDenoisePass draw. */
int rfx_poisson_denoise(rfx_ctx *, const rfx_denoise_params *);
int rfx_compose(rfx_ctx *, const rfx_compose_params *);
/* The effect's mainImage (src/ssgi/shader/ssgi_compose.frag:20-45), which postprocessing's EffectPass runs after
 * SSGIEffect.update(): background texels take the scene colour (RFX_TEX_DIRECT_LIGHT = the composer's input buffer),
 * the rest the composed GI (RFX_TEX_COMPOSE), fogged when the scene has fog; alpha 1.  Writes RFX_TEX_FINAL. */
int rfx_final_compose(rfx_ctx *, const rfx_final_params *);
/* MotionBlurEffect's mainImage (K6, ABI 20): see rfx_motion_blur_params.  Writes RFX_TEX_MOTION_BLUR.
 * On a ROW-TILED context (ABI 21) the draw produces the tile rows (row window honoured) once rfx_motion_blur_stage or rfx_motion_blur_gather has
 * armed it for p->source: the taps, and the `center == -1` fetch, read RFX_TEX_BLUR_SOURCE with whole-frame addressing; velocity, an explicit
 * centre slot and the output go through the band views like every other tiled draw.  The explicit centre of a row-tiled context is
 * RFX_TEX_TEMPORAL0 only (NEAREST: the pixel's own texel); any other slot is fetched LINEAR, its footprint leaves the rows the tile draws and no
 * mask names it: RFX_EUNSUPPORTED, from all four calls.  Arming lasts until the next stage or gather (a gather whose exchange fails disarms), so
 * a host may draw in row windows.  Not armed: RFX_EUNSUPPORTED (call rfx_motion_blur_stage or rfx_motion_blur_gather first); armed for another
 * source: RFX_ESTATE.  Bit-identical to the whole-frame context's rows when RFX_TEX_BLUR_SOURCE holds every texel rfx_motion_blur_reach_mask names. */
int rfx_motion_blur(rfx_ctx *, const rfx_motion_blur_params *);
/* Which texels of `source` will rfx_motion_blur with these params LOAD for the context's tile rows (intersected with the row window)?  Any
 * context, no communicator; blocks like rfx_ssgi_hit_mask and uses its format: `rows` must be the frame height, row_mask[y] gets bit b set when
 * a texel of frame row y in column block b (texel x is in block x * 32 / width) is loaded.  The mask encloses exactly the fetches of
 * motion_blur.frag:28-40 — all four texels of the LINEAR footprint of each of the samples + 1 taps at mix(startUv, endUv, i / samples), zero-weight
 * texels included (the kernel loads them and 0 * NaN is NaN) — and, when center == -1, the four texels of the LINEAR `inputColor` fetch at vUv.
 * A fragment that is not moved (dot(v, v) > 1e-9 false, NaN included) contributes its centre fetch only.  It is not a velocity BOUND: the
 * reduction (k6_motion_blur_reach) runs the draw's own streak set-up and tap addressing on the tile's velocity texels, the blue-noise table and
 * the uniforms, without the loads.  Validation and error codes are rfx_motion_blur's. */
int rfx_motion_blur_reach_mask(rfx_ctx *, const rfx_motion_blur_params *, unsigned int *row_mask, int rows);
/* Copy the context's tile rows of p->source into RFX_TEX_BLUR_SOURCE at their frame position (on the draw stream) and arm the tiled draw for
 * that source.  The piece a host with its own transport uses: it then fills the foreign texels the reach mask names with rfx_upload.  On a
 * whole-frame context: validates and returns (nothing to stage). */
int rfx_motion_blur_stage(rfx_ctx *, const rfx_motion_blur_params *);
/* Stage, reach mask, all-gather of the N masks, grouped ncclSend / ncclRecv of the named column blocks from their owners into
 * RFX_TEX_BLUR_SOURCE: the exchange of rfx_gather_history_rows on this plane.  Runs on the exchange stream, ordered after the draws enqueued so
 * far (the owners' rows of the source are current once their draw has executed); rfx_comm_wait orders the blur after it.  Waits on the host for
 * the N masks.  `bytes_received` (may be NULL): what this rank receives.  More than 64 ranks, no RCCL, no communicator: as
 * rfx_gather_history_rows. */
int rfx_motion_blur_gather(rfx_ctx *, const rfx_motion_blur_params *, void *ncclComm, size_t *bytes_received);

/* ---- streamed frame export (K7, rfx_export_params above): per-frame output of an offline run without a full-width blocking read-back.
 * Added to ABI 21 without a new version number, like rfx_ssgi_target_rows: four more entry points and one more profile kind, nothing an existing
 * call does differently; a host checks for the symbol.  (RFX_PROF_COUNT grew by one: a caller of rfx_profile_read sizes its arrays with the
 * RFX_PROF_COUNT of the header its library was built from.)
 * rfx_export_bytes: tile_rows * W * channels * element bytes; 0 on bad params.  `bytes` of the other calls must equal it.
 * rfx_stage_export enqueues the encode on the DRAW stream — ordered after every draw enqueued so far — into one of two internal device staging
 * buffers (not texture slots, not checkpoint state: allocated on first use, grown when a later call needs more, freed by rfx_destroy), then the
 * device-to-host copy on the context's DOWNLOAD stream (its own, so both PCIe directions run at once with rfx_stage_upload), which waits for an
 * event recorded after the kernel; it returns without waiting for either.  Tickets count up from 1 per context.
 *     draws(0); stage_export(A) -> 1;   loop: draws(n+1); stage_export(n+1 into the other buffer); export_wait(n); write frame n
 * Two orders hold: on the device, the encode of export n+2 waits for the copy of export n (they share a staging buffer); on the host,
 * rfx_stage_flip's rule — the call returns only once export n-2 has completed, so a host with two alternating pinned buffers never runs more
 * than two exports ahead.  `host` must stay valid until rfx_export_wait(ticket) returns.  Pinned memory (rfx_host_alloc) makes the copy
 * asynchronous; a pageable buffer is accepted and simply does not overlap.
 * rfx_export_wait returns when that export's bytes are in `host`: at once for a ticket that has retired, RFX_EINVAL for one never issued.
 * rfx_export = rfx_stage_export + rfx_export_wait (it takes a ticket of its own).  rfx_sync and rfx_destroy drain the download stream.
 * RFX_EINVAL: a source that is not one of the listed RGBA32F slots, a bad format / channel count / operator, an operator or exposure given with
 * a non-U8 format, bytes != rfx_export_bytes.  RFX_ESTATE: the source was never drawn, uploaded or bound (rfx_motion_blur's rule). */
size_t rfx_export_bytes(const rfx_ctx *, const rfx_export_params *);
int rfx_export(rfx_ctx *, const rfx_export_params *, void *host, size_t bytes);
int rfx_stage_export(rfx_ctx *, const rfx_export_params *, void *host, size_t bytes, int *ticket);
int rfx_export_wait(rfx_ctx *, int ticket);

/* ---- PNG fragments (K8): the U8_SRGB export leaves the device as a finished PNG data stream.  Additive to ABI 21 like the export: three
 * more entry points and one more profile kind (RFX_PROF_K8, read through rfx_profile_read_n); a host checks for the symbol.  K7 runs exactly as for rfx_stage_export, so the pixels in the
 * PNG are by construction the bytes rfx_export returns; K8 then encodes them on the DOWNLOAD stream, behind the "encoded" event, into a device
 * buffer of its own, and the device-to-host copy of the WHOLE bound follows.  (Copying only fragment_bytes would need the host to wait for the
 * header or the kernel to store into pinned memory; the downward PCIe direction is idle and the copy is already hidden, so it is left out.)
 *
 * THE FRAGMENT is the IDAT chunks of the context's tile rows and nothing else.
 *   Scanlines run top first: frame row tile_y0 + tile_rows - 1 down to tile_y0.  One scanline = one deflate chunk = one IDAT chunk:
 *       length (big-endian) | "IDAT" | payload | CRC-32("IDAT" + payload)
 *   Filter.  The scanline's FILTERED BYTES are the filter type byte followed by the n - 1 = W * channels residuals (n = 1 + W * channels).
 *     filter 0 (adaptive): the type with the smallest sum of |residual as int8| among None (0), Sub (1), Up (2), Paeth (4); a tie goes to the
 *     lowest type number.  The tile's FIRST scanline chooses between None and Sub only: its upper neighbour belongs to another tile (a
 *     whole-frame context is the one-tile case of the same rule).  filter 1..4 forces None, Sub, Up, Paeth; a forced Up or Paeth falls back
 *     to Sub on the tile's first scanline.  Avg is not offered.
 *   Payload: the smaller of two forms, a tie going to (a).  Both end on a byte boundary, so the payloads concatenate into one raw deflate stream.
 *     (a) one non-final dynamic-Huffman block of the n literals and the end-of-block symbol — no length / distance codes — then, after the
 *         three header bits 0 0 0 and padding to a byte, the empty non-final stored block 00 00 FF FF.  HLIT declares 257 codes, HDIST one
 *         distance code of length 0.  Size: ceil((block bits + 3) / 8) + 4.
 *     (b) ceil(n / 65535) non-final stored blocks (00 | LEN | ~LEN | bytes).  Size: n + 5 * ceil(n / 65535).
 *   THE CODE-LENGTH RULE (literal code: 257 symbols, limit 15, end-of-block counted once; code-length code: 19 symbols, limit 7):
 *     1. rank the symbols of non-zero frequency by (frequency descending, symbol number ascending);
 *     2. minimum-redundancy lengths by Moffat and Katajainen's in-place method over the frequencies in ascending order (the reverse of the
 *        ranking), where an internal node is taken before a leaf of equal weight;
 *     3. count the codes per length, a length above the limit counting at the limit; while the Kraft sum sum(count[i] << (limit - i)) exceeds
 *        1 << limit: take one code from count[limit], take one from the longest shorter length i that has one and add two to count[i + 1];
 *     4. hand the lengths out by rank, shortest first: the count[1] highest-ranked symbols get 1 bit, the next count[2] get 2, and so on;
 *     5. deflate's canonical codes from those lengths.
 *   The block header of (a): the 258 code lengths (257 literal / length codes, then the distance code's 0) as ONE sequence of run-length
 *     tokens — a run of r zeros: 18 (11..138) while r >= 11, then 17 (3..10) if r >= 3, else single 0s; a run of r equal non-zero lengths:
 *     the length once, then 16 (3..6) while 3 or more remain, then single lengths — coded with the code-length code built by the same rule
 *     from the tokens' frequencies; HCLEN = the last used entry of deflate's order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, at least 4.
 *     (A decoder accepts any valid header; this one is fixed so that the fragment is a pure function of the pixels — tests/png_device_ref.py
 *     restates it and the device's fragment equals it byte for byte.)
 * THE RESULT BUFFER (`host`, rfx_png_bound bytes): a 32-byte little-endian header, the fragment from offset 32, unspecified bytes after it.
 *       uint64 fragment_bytes | uint32 adler_a | uint32 adler_b | uint64 raw_bytes | 8 bytes of zero ("Match form" below counts its chunks in the first four)
 *   adler_a / adler_b: the stand-alone Adler-32 (initial value 1) of the tile's filtered bytes, low and high half; raw_bytes = tile_rows * n.
 * THE HOST'S WRAP: signature; IHDR; IDAT(78 01); the fragments, TOP TILE FIRST; IDAT(03 00 | Adler-32 big-endian) — the final empty block and
 *   the tiles' Adlers combined in that order as A = (A1 + A2 - 1) mod 65521, B = (B1 + B2 + len2 * (A1 - 1)) mod 65521; IEND.
 * rfx_png_bound = 32 + tile_rows * (12 + 5 * ceil(n / 65535) + n): every chunk in form (b).  0 on bad params or a format other than U8_SRGB.
 * `filter`: 0..4 as above.  Tickets come from rfx_stage_export's sequence and rfx_export_wait retires both kinds; the back pressure and the
 * two-buffer rule apply to the mixed sequence.  rfx_png = rfx_stage_png + rfx_export_wait.
 * RFX_EINVAL: what rfx_stage_export refuses, a format other than RFX_EXPORT_U8_SRGB, a filter outside 0..4, bytes != rfx_png_bound.
 * RFX_ESTATE: rfx_stage_export's rule. */
size_t rfx_png_bound(const rfx_ctx *, const rfx_export_params *);
int rfx_stage_png(rfx_ctx *, const rfx_export_params *, int filter, void *host, size_t bytes, int *ticket);
int rfx_png(rfx_ctx *, const rfx_export_params *, int filter, void *host, size_t bytes);

/* ---- EXR fragments (K8's second pre-transform): the F16 export leaves the device as finished OpenEXR ZIPS chunks.  Additive to ABI 21: three
 * more entry points, no new profile kind; a host checks for the symbol.  K7 runs exactly as for rfx_stage_export with RFX_EXPORT_F16 and 3 or 4
 * channels, so the samples in the file are by construction the halfs rfx_export returns; K8 then encodes them on the DOWNLOAD stream, behind the
 * "encoded" event, into the device buffer it uses for a PNG, and the device-to-host copy of the WHOLE bound follows (as for a PNG: copying only
 * fragment_bytes would need a host wait mid-stream; header.raw_bytes - header.fragment_bytes is what it would save).
 *
 * THE FRAGMENT is the scanline chunks of the context's tile rows and nothing else.
 *   Scanlines run top first: tile scanline s = 0 is frame row tile_y0 + tile_rows - 1; its EXR y is H - tile_y0 - tile_rows + s.
 *   One scanline = one chunk:   int32 y | int32 size | data   (little-endian)
 *   The scanline's RAW BLOCK, n = W * channels * 2 bytes: the channels in alphabetical order — A, B, G, R for 4 channels; B, G, R for 3 —
 *     each as W little-endian halfs.
 *   Its PREDICTED BYTES d: t = the even-indexed bytes of the raw block, then the odd-indexed ones; d[0] = t[0], d[i] = (t[i] - t[i-1] + 128) & 255
 *     (OpenEXR's ZIP / ZIPS / RLE pre-transform).
 *   data: form (a) when it is STRICTLY smaller than n bytes, else form (b); a reader tells them apart by size == n.
 *     (a) a complete zlib stream: 78 01; one FINAL dynamic-Huffman block (header bits 1 0 1) of the n literals d and the end-of-block symbol —
 *         no length / distance codes; HLIT declares 257 codes, HDIST one distance code of length 0 — padded to a byte; the Adler-32 of d,
 *         big-endian.  The code lengths follow THE CODE-LENGTH RULE and the block header the header-token rule of "PNG fragments" above, word for
 *         word: the data is a pure function of the halfs (tests/exr_device_ref.py restates it and the device's result equals it byte for byte).
 *         Size: 2 + ceil(block bits / 8) + 4.
 *     (b) the raw block itself, n bytes, unpredicted.
 *   There is no state across scanlines: the fragments of any row tiling, concatenated top tile first, are the whole frame's fragment.
 * THE RESULT BUFFER (`host`, rfx_exr_bound bytes): a 32-byte little-endian header, the fragment from offset 32, unspecified bytes after it.
 *       uint64 fragment_bytes | uint32 chunks | uint32 first_y | uint64 raw_bytes | uint32 raw_form_chunks | 4 bytes of zero ("Match form" below counts its chunks there)
 *   chunks = tile_rows; first_y = the y of the first chunk; raw_bytes = tile_rows * n; raw_form_chunks = the chunks in form (b).
 * THE HOST'S WRAP: magic and version; the attributes of a scanline file — channels (HALF, alphabetical), compression 2 (ZIPS), dataWindow,
 *   displayWindow, lineOrder 0 (increasing y), pixelAspectRatio, screenWindowCenter, screenWindowWidth; the offset table, built by walking the
 *   chunks' size fields; the fragments, TOP TILE FIRST.
 * rfx_exr_bound = 32 + tile_rows * (8 + n): every chunk in form (b).  0 on bad params or a format other than RFX_EXPORT_F16.
 * Tickets come from rfx_stage_export's sequence and rfx_export_wait retires all three kinds; the back pressure and the two-buffer rule apply to
 * the mixed sequence.  rfx_exr = rfx_stage_exr + rfx_export_wait.  The encode is timed under RFX_PROF_K8.
 * RFX_EINVAL: what rfx_stage_export refuses, a format other than RFX_EXPORT_F16, bytes != rfx_exr_bound.
 * RFX_ESTATE: rfx_stage_export's rule. */
size_t rfx_exr_bound(const rfx_ctx *, const rfx_export_params *);
int rfx_stage_exr(rfx_ctx *, const rfx_export_params *, void *host, size_t bytes, int *ticket);
int rfx_exr(rfx_ctx *, const rfx_export_params *, void *host, size_t bytes);

/* ---- Match form (K8 with run-length matches): both fragment kinds gain a third chunk form with LZ77 matches of distance 1.  Additive to ABI
 * 21: four more entry points, no new profile kind; a host checks for the symbol.  Opt-in per call: `flags` = 0 is rfx_stage_png / rfx_png /
 * rfx_stage_exr / rfx_exr byte for byte, RFX_ENCODE_MATCHES adds form (c) below; any other bit is RFX_EINVAL.  Everything else — K7, the
 * tickets, the back pressure, the two staging buffers, rfx_export_wait, RFX_PROF_K8, the bounds, the host's wrap — is the export's, over the
 * mixed sequence of all export kinds.  rfx_export_params keeps its layout.
 *
 *   THE BYTE SEQUENCE d[0, n) of a chunk is what the chunk codes without matches: the PNG scanline's filtered bytes, type byte first; the EXR
 *     scanline's predicted bytes.
 *   THE TOKEN RULE.  Position j >= 1 is REPEATING when d[j] == d[j - 1].  A maximal interval [s, e) of repeating positions is cut from s into
 *     pieces of 258 positions.  A piece of 3 or more positions is ONE MATCH: length = the piece, distance 1.  A last piece of 1 or 2 positions
 *     is literals, and so is every position that is not repeating.  A match never reaches before d[0]: no state crosses chunks, the fragments
 *     of any row tiling still concatenate to the whole frame's, and a PNG scanline still never looks at the previous scanline's bytes.
 *   FORM (c): one dynamic-Huffman block of those tokens and the end-of-block symbol.  The literal / length code covers 286 symbols, limit 15,
 *     the end-of-block symbol counted once, built by THE CODE-LENGTH RULE of "PNG fragments" from the tokens' frequencies (a match counts for
 *     its length symbol).  HLIT declares the codes up to the highest used symbol, at least 257.  HDIST declares one distance code, code 0, of
 *     length 1.  A match costs its length symbol, deflate's extra bits for the length, and the one distance bit 0 (distance code 0 has no extra
 *     bits).  The code-length sequence — the HLIT lengths, then that 1 — is tokenised by the header-token rule and coded by the code-length
 *     code rule of "PNG fragments", word for word.
 *     PNG: the block is non-final and followed by the empty stored block, exactly as form (a).  Size: ceil((block bits + 3) / 8) + 4.
 *     EXR: the block is FINAL inside 78 01 ... Adler-32 of d, exactly as form (a).  Size: 2 + ceil(block bits / 8) + 4.
 *   FORM CHOICE.  A chunk takes form (c) only when it contains at least one match AND (c) is STRICTLY smaller than what the chunk gets without
 *     matches — PNG: the smaller of (a) and (b); EXR: (a) when that is smaller than n, else n.  So no chunk is larger with matches than
 *     without, and a chunk without a match is byte-identical.  (tests/match_device_ref.py restates the form; the device's result equals it
 *     byte for byte.)
 *   THE RESULT BUFFER: uint32 match_form_chunks, the chunks in form (c), stands in bytes that are zero otherwise — PNG: the first four of the
 *     header's trailing 8 bytes (offset 24); EXR: the trailing 4 bytes (offset 28).  Zero with flags = 0.
 * RFX_EINVAL: a bit in `flags` other than RFX_ENCODE_MATCHES; what the call without _ex refuses. */
#define RFX_ENCODE_MATCHES 1u
int rfx_stage_png_ex(rfx_ctx *, const rfx_export_params *, int filter, unsigned flags, void *host, size_t bytes, int *ticket);
int rfx_png_ex(rfx_ctx *, const rfx_export_params *, int filter, unsigned flags, void *host, size_t bytes);
int rfx_stage_exr_ex(rfx_ctx *, const rfx_export_params *, unsigned flags, void *host, size_t bytes, int *ticket);
int rfx_exr_ex(rfx_ctx *, const rfx_export_params *, unsigned flags, void *host, size_t bytes);

int rfx_sync(rfx_ctx *);

/* ---- streaming dumps: host buffers that cross PCIe every frame (an offline run over a dumped sequence).  rfx_upload is synchronous
 * (the caller may free the plane on return).  The streaming form double-buffers the four input planes of the dump (depth, gbuffer,
 * velocity, direct light): rfx_stage_upload enqueues the copy of the NEXT frame's plane into the slot's back buffer on the context's
 * upload stream and returns; rfx_stage_flip makes everything staged since the last flip current — draws enqueued after it wait for
 * those copies, and copies staged after it wait for the draws enqueued before it (they overwrite the buffer those draws read).
 *     stage(frame 0); flip();   loop: stage(frame n+1); draws of frame n; flip()
 * `host` must stay valid and unchanged until the flip AFTER the one that publishes it has returned: rfx_stage_flip returns only when
 * the copies published by the previous flip have executed (host-side back pressure — a host with two alternating sets of pinned planes
 * can refill a set as soon as the next flip is back, and never runs more than two frames ahead of the device).  Pinned memory
 * (rfx_host_alloc = hipHostMalloc) is what makes the copy asynchronous; a pageable plane is accepted and simply does not overlap. */
void *rfx_host_alloc(size_t bytes);
void rfx_host_free(void *);
int rfx_stage_upload(rfx_ctx *, rfx_tex id, const void *host, int row0, int rows);
int rfx_stage_flip(rfx_ctx *);

/* ---- streamed AOV frames (additive to ABI 21: a host checks for the symbol): the importer's planes staged like a packed dump.
 * rfx_stage_aov is rfx_stage_upload for an engine's UNPACKED attribute planes: every needed plane crosses PCIe once, on the upload stream,
 * into a staging area the context owns (allocated on first use, grown when a later call needs more, freed by rfx_destroy; at most 84 bytes
 * per band pixel: 76 without a position plane, "AOV conventions" below), and one fused pack kernel behind the copies writes the BACK buffers of the dump's input slots, which rfx_stage_flip
 * publishes as ever.  Nothing is allocated, freed or synchronised per call.  Host-pointer lifetime and back pressure are rfx_stage_upload's:
 * a plane must stay valid and unchanged until the flip AFTER the one that publishes it has returned; pinned planes (rfx_host_alloc) make
 * the copies asynchronous, a pageable plane is accepted and simply does not overlap.
 * A plane is `rows` x width x channels tightly packed elements, row `row0` of the frame first (row 0 = bottom), float32 or IEEE half: an F16
 * element means (float)half, which is exact, so a half plane costs two bytes per element on the bus and gives the texels the widened plane
 * gives.  A plane that is not given has data == NULL.
 *   DEPTH         always written: the widened depth plane (required).
 *   GBUFFER       written iff diffuse, normal, roughness, metalness and emissive are ALL given (some of them: RFX_EINVAL): the texels
 *                 rfx_pack_gbuffer writes for those floats with the depth plane as coverage.  A 3-channel diffuse has alpha 1.
 *   VELOCITY      written iff velocity is given (normal is then required): rfx_pack_velocity's texels.
 *   DIRECT_LIGHT  written iff direct is given: the widened rgb(a); a 3-channel plane has alpha 1.
 * A slot that is not written keeps what rfx_stage_upload staged for it: the two forms mix within one batch.  NaN payloads are not specified.
 * Rows: the band must lie inside the rows DEPTH holds (the whole frame, on every context); each written slot receives band ∩ the rows it
 * holds, and a plane row no written row needs is not copied: rfx_aov_stage_bytes returns exactly the bytes the call copies host -> device
 * (0 on bad parameters).  RFX_EINVAL: a bad type or channel count, no depth, a partial G-buffer set, velocity without normal, a band outside
 * DEPTH's rows; RFX_ESTATE: a slot to be written is bound to an external buffer; RFX_ENOMEM: the staging area. */
typedef enum rfx_plane_type { RFX_PLANE_F32 = 0, RFX_PLANE_F16 = 1 } rfx_plane_type;
typedef struct rfx_plane { const void *data; int type; int channels; } rfx_plane;
typedef struct rfx_aov_frame {
    rfx_plane diffuse;    /* 3 or 4 (3: alpha = 1) */
    rfx_plane normal;     /* 3, world space */
    rfx_plane roughness;  /* 1 */
    rfx_plane metalness;  /* 1 */
    rfx_plane emissive;   /* 3 */
    rfx_plane velocity;   /* 2 */
    rfx_plane depth;      /* 1, required */
    rfx_plane direct;     /* 3 or 4 (3: alpha = 1) */
} rfx_aov_frame;
size_t rfx_aov_stage_bytes(const rfx_ctx *, const rfx_aov_frame *, int row0, int rows);
int rfx_stage_aov(rfx_ctx *, const rfx_aov_frame *, int row0, int rows);

/* ---- AOV conventions (additive to ABI 21: a host checks for the symbol): the planes as engines write them.
 * rfx_aov_frame's attributes are the reference's raster passes': depth = gl_FragCoord.z with 1.0 = not covered, velocity = the uv-space
 * pos1 - pos0 of VelocityDepthNormalMaterial.js:76-80, normal in world space.  A renderer writes a world position pass or a camera-space
 * depth, motion in pixels with its own sign and y direction (or none: a static scene under a moving camera), often camera-space normals.
 * rfx_set_aov_conventions says which of these the NEXT rfx_stage_aov / rfx_stage_exr_aov / rfx_stage_exr_blocks / rfx_stage_exr_blocks_piz
 * calls stage; the pack kernel converts per pixel, in fp32, on the staged planes.  The setting is context state, read at each of those calls
 * (set it per frame: the matrices change); NULL, or a struct whose three kinds are all 0, is the default: every call gives the bytes it gives
 * without the setting.  It is not checkpoint state; rfx_pack_gbuffer, rfx_pack_velocity and rfx_stage_upload never read it.
 *   depth_kind     FRAGCOORD: as above.  VIEW_Z: the 1-channel depth plane holds the positive distance along the camera axis, viewZ = -value.
 *                  POSITION: the depth plane has 3 channels, world x, y, z (an EXR descriptor maps P.X / P.Y / P.Z to components 0..2 of
 *                  RFX_EXR_PLANE_DEPTH).
 *   velocity_kind  UV: as above.  SCALED: the 2-channel plane times velocity_scale, e.g. (1/W, -1/H) for pixels, y down; a negated pair for the
 *                  other time direction.  CAMERAS: no velocity plane (one given: RFX_EINVAL); VELOCITY is written iff normal is given, the
 *                  motion is the point's own position through velocityMatrix and prevVelocityMatrix.
 *   normal_space   WORLD: as above.  VIEW: camera-space normals, turned by cameraMatrixWorld.
 * Matrices are float32, column-major (M[c][r] = m[4 c + r]), named as the reference names its uniforms: velocityMatrix / prevVelocityMatrix =
 * projectionMatrix x matrixWorldInverse of this and of the previous frame (VelocityDepthNormalMaterial.js:42-43 for an identity model matrix;
 * a host forms the product in float64 in three's multiplyMatrices element order, then rounds).  near_, far_, perspective: the camera's, read
 * where a FRAGCOORD depth is turned back into view Z (CAMERAS).  has_background_position: a texel whose position equals background_position
 * component-wise (==) is not covered (Blender writes 0, 0, 0 there).
 * ARITHMETIC.  IEEE binary32, uncontracted, in this order (tests/aov_convention_ref.py restates it):
 *   mul(M, p)_i = ((M[0][i] x + M[1][i] y) + M[2][i] z) + M[3][i]
 *   POSITION  new = mul(velocityMatrix, p); fragCoordZ = ((0.5f new.z) / new.w) + 0.5f (line 81's shape).  Covered iff x, y, z are finite, the
 *             texel is not the background position, new.w > 0 and 0 <= fragCoordZ < 1; else depth 1.0.
 *   VIEW_Z    cz = P[2][2] viewZ + P[3][2], cw = P[2][3] viewZ + P[3][3], the same quotient; P[0][2], P[0][3], P[1][2], P[1][3] must be 0
 *             (RFX_EINVAL).  Covered iff the value is finite and > 0 and 0 <= fragCoordZ < 1.
 *   CAMERAS   pos0 = (prev.xy / prev.w) 0.5f + 0.5f with prev = mul(prevVelocityMatrix, p), pos1 likewise from new, vel = pos1 - pos0 (lines
 *             76-79).  p is the position plane's texel under POSITION; else it is rebuilt from the texel's uv ((x + 0.5f) / W, (y + 0.5f) / H)
 *             and its view Z — perspectiveDepthToViewZ / orthographicDepthToViewZ of the depth under FRAGCOORD, -value under VIEW_Z — by
 *             getViewPosition (ssgi_utils.frag:17-24: clipW = P[2][3] viewZ + P[3][3]; v = Pinv x (((uv, viewZ) - 0.5f) 2.0f clipW, clipW) with
 *             all four terms of each row summed left to right; v.z = viewZ) and p = mul(cameraMatrixWorld, v).
 *   VIEW      n_i = (C[0][i] nx + C[1][i] ny) + C[2][i] nz, C = cameraMatrixWorld, then the oct encoder as ever.
 *   A texel that is not covered has the clear colour in GBUFFER and VELOCITY, as under the default.  Non-finite results of vel are "a
 *   non-finite value"; payload bits and subnormal intermediates are not specified.
 * ROWS AND BYTES.  rfx_aov_stage_bytes and its three EXR twins count the 3-channel plane; the staging area is at most 84 bytes per band pixel.
 * A bad EXR chunk or block still reads as not covered under every depth kind: a non-finite position or view Z is staged there, not 1.
 * RFX_EINVAL from rfx_set_aov_conventions: an unknown kind; a non-finite velocity_scale under SCALED; the four projection entries under VIEW_Z;
 * near_ >= far_ or a non-finite one where they are read (FRAGCOORD with CAMERAS).  From the staging calls: a depth plane that has not the
 * kind's channel count, a velocity plane under CAMERAS. */
enum { RFX_AOV_DEPTH_FRAGCOORD = 0, RFX_AOV_DEPTH_VIEW_Z = 1, RFX_AOV_DEPTH_POSITION = 2 };
enum { RFX_AOV_VELOCITY_UV = 0, RFX_AOV_VELOCITY_SCALED = 1, RFX_AOV_VELOCITY_CAMERAS = 2 };
enum { RFX_AOV_NORMAL_WORLD = 0, RFX_AOV_NORMAL_VIEW = 1 };
typedef struct rfx_aov_conventions {
    int32_t depth_kind, velocity_kind, normal_space;
    int32_t perspective;
    float velocity_scale[2];
    float near_, far_;
    float velocityMatrix[16], prevVelocityMatrix[16];
    float projectionMatrix[16], projectionMatrixInverse[16], cameraMatrixWorld[16];
    int32_t has_background_position;
    float background_position[3];
} rfx_aov_conventions;
int rfx_set_aov_conventions(rfx_ctx *, const rfx_aov_conventions *);   /* NULL: back to the default */

/* ---- device planes (additive to ABI 21: a host checks for the symbol): rfx_stage_aov for planes that already live in device memory.
 * A renderer on the same device (a HIP path tracer, a torch rasteriser) hands over the buffers it wrote, laid out as IT lays them out; the pack
 * kernel reads them where they are.  Nothing crosses PCIe, the staging area is not touched, and the LIBRARY allocates, frees and
 * host-synchronises nothing per call — the caller, though, has to make the planes complete first (ORDERING below: in this version that is a
 * synchronise of the producer's stream in the caller's frame loop).  In everything but where the bytes
 * come from the call IS rfx_stage_aov: the same slots under the same rules (DEPTH always; GBUFFER, VELOCITY, DIRECT_LIGHT where their planes are
 * given), the same back buffers published by rfx_stage_flip, the same row rule (DEPTH takes the whole band, the other slots band ∩ the rows they
 * hold), rfx_set_aov_conventions read the same way (POSITION: the depth plane has 3 channels; CAMERAS: no velocity plane), and it mixes within
 * one batch with rfx_stage_upload, rfx_stage_aov and the EXR calls.  The texels are, bit for bit, those rfx_stage_aov writes for the same
 * element values.
 * A PLANE is addressed by strides, in ELEMENTS (float32 or IEEE half, by `type`), of any sign, 0 allowed (a broadcast): the element of frame
 * column x, frame row y of the band and channel ch is data[x stride_x + (y - row0) stride_y + ch stride_c].  Row 0 is the frame's BOTTOM row and
 * stride_y steps to the row above: an image kept top-down has a negative stride_y and `data` at its last image row.  stride_c is not read for a
 * 1-channel plane.  data == NULL: the plane is not given.  Three layouts are read with vector loads, when `data` is aligned to four elements and
 * stride_y (and stride_c, planar) are multiples of four: INTERLEAVED (stride_c 1, stride_x = channels; any row pitch), PLANAR (stride_x 1; any
 * plane and row pitch); everything else — a mirrored or broadcast axis, a base or a pitch off that alignment — is read element by element.
 * When every plane a segment of the band reads is tight (interleaved, stride_y = width x channels) and 16-byte aligned, that segment is
 * packed by rfx_stage_aov's own kernel on the caller's pointers.
 * ORDERING.  producer_stream must be NULL in this version (anything else: RFX_EUNSUPPORTED; the parameter is where a hipStream_t the call
 * orders itself against will go): the planes are complete when the call is made — the producer's stream has been synchronised, or the upload
 * stream was made to wait by the caller's own means — and stay unchanged until the flip after the one that publishes them has returned
 * (rfx_stage_aov's rule).
 * Planes that overlap the context's own buffers (rfx_tex_device_ptr, a back buffer) are undefined.  The library does not ask the runtime what
 * kind of memory `data` is: an address the device cannot read faults there.
 * RFX_EINVAL: everything rfx_stage_aov refuses; a `data` not aligned to its element size; a plane whose extent — the sum over the three axes of
 * |stride| (count - 1), plus one, elements over the band — does not fit in 2^62 - 1 bytes.  RFX_ESTATE: a slot to be written is bound to an external
 * buffer.  Every check runs before anything is enqueued: a refused call leaves the batch as it was. */
typedef struct rfx_device_plane {
    const void *data;     /* device address of element (x = 0, frame row row0, channel 0); NULL: plane not given */
    int32_t type;         /* RFX_PLANE_F32 / RFX_PLANE_F16 */
    int32_t channels;     /* as rfx_plane */
    int64_t stride_x, stride_y, stride_c;  /* in ELEMENTS, any sign, 0 allowed (broadcast); stride_y steps to frame row + 1 (row 0 = bottom) */
} rfx_device_plane;
typedef struct rfx_aov_device_frame { rfx_device_plane diffuse, normal, roughness, metalness, emissive, velocity, depth, direct; } rfx_aov_device_frame;
int rfx_stage_aov_device(rfx_ctx *, const rfx_aov_device_frame *, int row0, int rows, void *producer_stream);
/* (producer_stream stays reserved.  A producer that must not host-synchronise orders the upload stream itself, before the call:
 * rfx_queue_wait_stream(ctx, RFX_QUEUE_UPLOAD, its stream) — "device images and stream ordering" below.) */

/* ---- device images and stream ordering (additive to ABI 21: a host checks for the symbols): the way OUT that stays on the device, and the
 * two calls that order a context's queues against a caller's stream without a host wait.
 * rfx_export_device is rfx_export into a buffer in device memory that the CALLER owns and lays out — a torch tensor a denoiser reads, a video
 * encoder's input surface, a viewer's texture.  It covers the context's tile rows [tile_y0, tile_y0 + tile_rows) of params->source and reads
 * rfx_export_params exactly as rfx_export does: the same sources, the same 8 format / channel / operator combinations, the same RFX_EINVAL and
 * RFX_ESTATE rules.  K7 encodes on the DRAW stream, after every draw enqueued so far, straight into the image: the element of column x, frame
 * row y and channel ch goes to data[x stride_x + (y - tile_y0) stride_y + ch stride_c], strides in ELEMENTS of params->format (4 / 2 / 1
 * bytes), of any sign; row 0 is the frame's BOTTOM row, so an image kept top-down has a negative stride_y and `data` at its last image row.
 * The elements are, bit for bit, those rfx_export returns for the same parameters.  No byte the image does not address is written: row
 * padding, plane padding and whatever lies before an offset base keep what they held.  The call takes no ticket, uses no staging buffer and no
 * download stream, allocates nothing and waits for nothing; it does not count in the tickets of rfx_stage_export and leaves their back
 * pressure alone.  rfx_set_row_window does not apply.  Several contexts of one process (row tiles on one device) may write their bands
 * into one frame-sized buffer.  The encode is timed under RFX_PROF_K7.
 * STORE FORMS (decided per call, uniform over the launch).  TIGHT — interleaved (stride_c 1, stride_x = channels), stride_y = width x channels,
 * `data` on a 4-byte boundary: rfx_export's own kernel on the caller's pointer.  INTERLEAVED — stride_c 1, stride_x = channels, `data` and the
 * row pitch in bytes multiples of 4: whole dwords, any row pitch.  PLANAR — stride_x 1, `data` aligned to four elements, stride_y and stride_c
 * multiples of four elements: one 16- / 8- / 4-byte store per channel and four pixels (F32 / F16 / U8).  Everything else — a misaligned base
 * or pitch, a mirrored x, scanline-planar (H, C, W) at a width that breaks the alignment — is written element by element.
 * RFX_EINVAL (every check runs before anything is enqueued, and rfx_last_error names the entry point): what rfx_export refuses; dst or
 * dst->data NULL; `data` not a multiple of the element size; an extent — (1 + the sum over the three axes of |stride| (count - 1)) elements —
 * beyond 2^62 - 1 bytes; strides that do not NEST.  A store image must not alias itself: of the axes whose count is above 1 (width, tile_rows,
 * channels), sorted by |stride|, the smallest |stride| must be >= 1 and every later one >= the one before it x that axis's count.  This admits
 * interleaved, planar (C, H, W), scanline-planar (H, C, W), any row or plane pitch, a top-down image, a mirrored axis; it refuses a 0 stride.
 * The rule is SUFFICIENT for an image without aliases, not necessary: some exotic alias-free layouts (interlocking combs) are refused too.
 * An image that overlaps the context's own buffers is undefined.  The library does not ask the runtime what kind of memory `data` is: an
 * address the device cannot write faults there.
 *
 * rfx_queue_wait_stream / rfx_stream_wait_queue: one hipEventRecord and one hipStreamWaitEvent each, on events the context owns (created at
 * the first use, destroyed by rfx_destroy).  The host never waits and nothing is allocated at a repeated call.  `queue`: RFX_QUEUE_DRAW —
 * whichever stream the context draws on at the call (rfx_set_stream) — or RFX_QUEUE_UPLOAD, the stream of the rfx_stage_* calls (created
 * here if no staged call has yet).  hip_stream NULL: RFX_EINVAL — the legacy default stream cannot be named, rfx_set_stream's rule.  An
 * unknown queue: RFX_EINVAL.  Only work enqueued BEFORE the call is ordered ("NOW").  The four uses:
 *   a producer, before rfx_stage_aov_device reads its planes:        rfx_queue_wait_stream(ctx, RFX_QUEUE_UPLOAD, producer)
 *   a producer, before it rewrites planes a staged call still reads: rfx_stream_wait_queue(ctx, RFX_QUEUE_UPLOAD, producer)
 *   a consumer whose image rfx_export_device is about to rewrite:    rfx_queue_wait_stream(ctx, RFX_QUEUE_DRAW, consumer)
 *   a consumer, before it reads the image:                           rfx_stream_wait_queue(ctx, RFX_QUEUE_DRAW, consumer) */
typedef struct rfx_device_image {
    void *data;                            /* device address of element (x = 0, frame row tile_y0, channel 0) */
    int64_t stride_x, stride_y, stride_c;  /* in ELEMENTS of params->format (4 / 2 / 1 bytes), any sign;
                                              stride_y steps to frame row + 1 (row 0 = bottom) */
} rfx_device_image;
int rfx_export_device(rfx_ctx *, const rfx_export_params *, const rfx_device_image *dst);

enum { RFX_QUEUE_DRAW = 0, RFX_QUEUE_UPLOAD = 1 };
int rfx_queue_wait_stream(rfx_ctx *, int queue, void *hip_stream);  /* the context's queue waits for what hip_stream holds NOW */
int rfx_stream_wait_queue(rfx_ctx *, int queue, void *hip_stream);  /* hip_stream waits for what the context's queue holds NOW */

/* ---- streamed EXR frames (additive to ABI 21: a host checks for the symbol): rfx_stage_aov for an AOV frame that is still a compressed OpenEXR
 * file.  The scanline chunks cross PCIe as they sit in the file, on the upload stream; K9 (csrc/k9_exr_import.hip) inflates them — one wave per
 * chunk, any RFC 1950 stream: stored, fixed and dynamic blocks, the Adler-32 checked —, undoes the predictor and the byte split, and scatters the
 * mapped channels into the typed staging planes rfx_stage_aov copies into; the same fused pack kernel then writes the back buffers.  The texels
 * are by construction the ones rfx_stage_aov writes for the planes a host decode of the file gives.  The host parses the header and the offset
 * table (a few KiB) and does no per-pixel work.
 * THE DESCRIPTOR.  `data` / `bytes`: the file (pinned memory makes the copies asynchronous).  Per part: its compression (OpenEXR's numbers: NONE 0,
 * ZIPS 2, ZIP 3) and its channels IN FILE ORDER, each with its pixel type (OpenEXR's: HALF 1, FLOAT 2) and the AOV plane (RFX_EXR_PLANE_*: the
 * index of the plane in rfx_aov_frame) and component it feeds, or plane RFX_EXR_SKIP: the channel is decoded with its chunk and dropped.  Per
 * chunk: its part, the file offset of the PACKED DATA (behind the chunk's y and size fields), the packed size, the first scanline y (0 = top) and
 * its rows.  Every part's data window is the frame (width x height of the context); a ZIP chunk has 16 rows but the last, the others one.
 * A chunk whose packed size equals rows x the part's bytes per scanline is the raw block (OpenEXR's rule) and is copied, as is every NONE chunk.
 * THE PLANES.  A plane exists when a channel maps to it; its components must be 0 .. n-1, each once, with n what rfx_stage_aov accepts (a
 * diffuse or direct plane without component 3 has three channels: alpha 1).  A plane whose channels are all HALF is staged as RFX_PLANE_F16, else
 * as RFX_PLANE_F32 with its halves widened.  The written-slot rules, the band rules, the host-pointer lifetime (`data`; the descriptor itself is
 * consumed by the call) and the back pressure are rfx_stage_aov's, word for word, for those planes.
 * THE BAND.  Only chunks with a scanline inside the band [row0, row0 + rows) (frame rows, 0 = bottom: scanline y is frame row height - 1 - y) are
 * copied and decoded, each with one copy of exactly its packed bytes; a ZIP chunk that straddles the band's edge is decoded whole and only its
 * rows inside the band are scattered.  Every scanline of the band must be covered by a chunk of every part that feeds a plane.
 * rfx_exr_aov_stage_bytes returns exactly the bytes the call copies host -> device: the packed bytes of those chunks (0 for a frame the call
 * would refuse).
 * STATUS.  A chunk that does not decode (any byte string is safe to send: reads are bounded by the packed size, writes by the raw size) makes
 * its rows read as not covered — depth 1, every other staged sample of it 0 — and is counted.  rfx_exr_aov_status blocks until the decode of the
 * most recent rfx_stage_exr_aov call has executed and reports the number of bad chunks, the first bad chunk's index in the descriptor's table
 * (-1: none) and its error code (csrc/k9_inflate.h K9_E_*; 0: none).  Any pointer may be NULL.  RFX_ESTATE before the first call.
 * Packed bytes, inflate scratch and status live in staging areas the context owns: allocated on first use, grown only when a later call needs
 * more (the one wait of this path), freed by rfx_destroy; nothing is allocated, freed or synchronised per call otherwise.
 * RFX_EINVAL: a UINT channel or another pixel type; a compression other than the three; a chunk outside the file bytes; a chunk whose part, y or
 * rows are inconsistent with the header (rows: 16 for ZIP but the last chunk, else 1; y a multiple of that; a packed size of 0 or of 2^30 or more,
 * or different from the raw size in a NONE part); two chunks of a part on one scanline; a band scanline no chunk of a mapped part covers; a component mapped
 * twice or missing; and what rfx_stage_aov refuses for the resulting planes (no depth, a partial G-buffer set, velocity without normal, a band
 * outside DEPTH's rows).  RFX_ESTATE, RFX_ENOMEM: rfx_stage_aov's. */
enum { RFX_EXR_NONE = 0, RFX_EXR_ZIPS = 2, RFX_EXR_ZIP = 3 };   /* rfx_exr_part.compression */
enum { RFX_EXR_HALF = 1, RFX_EXR_FLOAT = 2 };                    /* rfx_exr_channel.pixel_type */
enum { RFX_EXR_SKIP = -1, RFX_EXR_PLANE_DIFFUSE = 0, RFX_EXR_PLANE_NORMAL, RFX_EXR_PLANE_ROUGHNESS, RFX_EXR_PLANE_METALNESS, RFX_EXR_PLANE_EMISSIVE,
       RFX_EXR_PLANE_VELOCITY, RFX_EXR_PLANE_DEPTH, RFX_EXR_PLANE_DIRECT };
typedef struct rfx_exr_channel { int pixel_type; int plane; int component; } rfx_exr_channel;
typedef struct rfx_exr_part { int compression; int channels; const rfx_exr_channel *channel; } rfx_exr_part;
typedef struct rfx_exr_chunk { int part; int y; int rows; int reserved; unsigned long long offset; unsigned long long packed_bytes; } rfx_exr_chunk;
typedef struct rfx_exr_frame {
    const void *data; unsigned long long bytes;
    int parts; int chunks;
    const rfx_exr_part *part;
    const rfx_exr_chunk *chunk;
} rfx_exr_frame;
size_t rfx_exr_aov_stage_bytes(const rfx_ctx *, const rfx_exr_frame *, int row0, int rows);
int rfx_stage_exr_aov(rfx_ctx *, const rfx_exr_frame *, int row0, int rows);
int rfx_exr_aov_status(rfx_ctx *, int *bad_chunks, int *first_bad, int *code);

/* ---- EXR blocks (additive to ABI 21: a host checks for the symbol): the streamed EXR frames above for the file forms other writers choose — tiled
 * parts, RLE and PXR24 compression, a data window that is not the display window.  rfx_stage_exr_aov keeps its descriptor, checks and results; it
 * and rfx_stage_exr_blocks run one plan and the same kernels.
 * THE DESCRIPTOR.  rfx_exr_part and rfx_exr_channel as above.  A BLOCK is a rectangle of the frame: `x`, `y` its top-left texel (scanline 0 = top),
 * `cols` x `rows` texels, stored as OpenEXR stores a chunk — per row, every channel's `cols` samples, in file order —; `offset` / `packed_bytes`:
 * the PACKED DATA in the file bytes.  It serves a scanline chunk (x = 0, cols = width) and a tile alike: the library does not know which it is.
 * The frame (width x height of the context) is the parts' common data window.
 * COMPRESSIONS.  A part's compression is one of the five: NONE 0, RLE 1, ZIPS 2, ZIP 3, PXR24 5 (OpenEXR's numbers).
 * GEOMETRY.  A block lies inside the frame, cols >= 1, rows >= 1.  There is no per-compression row rule: the decoders need none.
 * SIZES.  The raw size rows x cols x bytes per texel is below 2^30; the packed size is 1 .. 2^30 - 1 and inside the file bytes; in a NONE part it
 * equals the raw size.  A block whose packed size equals its raw size is the raw block, whatever the compression (OpenEXR's rule) — for PXR24
 * with FLOAT channels that is whole 32-bit floats, while its zlib stream holds 3 bytes per FLOAT sample: the inflate must give exactly
 * rows x cols x (2 per HALF channel + 3 per FLOAT channel) bytes, not the raw size.
 * COVERAGE.  Within the band every texel of every part that feeds a plane lies in exactly one block of that part: two blocks on one texel, and a
 * texel without a block, are both refused (checked on the host by sorting the x-intervals of the band's rows).
 * THE BAND.  A block with a row inside the band is copied (one copy of exactly its packed bytes) and decoded whole; only its rows inside the band
 * are scattered.  rfx_exr_blocks_stage_bytes is the sum of the packed bytes of exactly those blocks (0 for a frame the call would refuse).
 * THE PLANES (components 0 .. n-1, F16 iff every channel is HALF, the missing alpha), the written-slot and band rules, the host-pointer lifetime
 * and the back pressure, the staging areas' ownership and growth: rfx_stage_exr_aov's, word for word.
 * STATUS.  Any byte string is safe to send: reads are bounded by the packed size, writes by the raw size.  A block that does not decode makes its
 * rectangle read as not covered (depth 1, every other staged sample of it 0) and is counted; rfx_exr_aov_status reports, for the most recent call
 * of either entry point, the bad blocks, the first one's index in the block table and its code (csrc/k9_inflate.h, csrc/k9_rle.h K9_E_*).
 * RFX_EINVAL: what the rules above exclude, and rfx_stage_exr_aov's cases for parts, channels, planes and the band.  No new profile kind. */
enum { RFX_EXR_RLE = 1, RFX_EXR_PXR24 = 5 };   /* beside NONE 0, ZIPS 2, ZIP 3: OpenEXR's own numbers */
typedef struct rfx_exr_block { int part; int x; int y; int cols; int rows; int reserved;
                               unsigned long long offset; unsigned long long packed_bytes; } rfx_exr_block;
typedef struct rfx_exr_block_frame { const void *data; unsigned long long bytes; int parts; int blocks;
                                     const rfx_exr_part *part; const rfx_exr_block *block; } rfx_exr_block_frame;
size_t rfx_exr_blocks_stage_bytes(const rfx_ctx *, const rfx_exr_block_frame *, int row0, int rows);
int    rfx_stage_exr_blocks(rfx_ctx *, const rfx_exr_block_frame *, int row0, int rows);

/* ---- EXR blocks with PIZ (additive to ABI 21: a host checks for the symbol): rfx_stage_exr_blocks for a file whose parts may also be PIZ-compressed
 * (4: the OpenEXR library's default).  The descriptor, the rules, the band arithmetic, the back pressure, the staging ownership and the results are
 * rfx_stage_exr_blocks', word for word, and both run one plan and the same kernels; the one difference: a part's compression may also be 4, in any
 * mix with the other five.  rfx_stage_exr_blocks and rfx_stage_exr_aov keep refusing it (RFX_EINVAL): a host opts in by calling these.
 * A PIZ BLOCK.  OpenEXR's scanline block of a PIZ part holds min(32, the rows left) rows, and a tile is a block, as now: there is still no row rule,
 * the library does not know which it is.  THE LIMIT: the wavelet of a block is decoded in cells of 64 x 64 words, each through all its levels on its
 * own, which holds while the largest power of two <= min(cols, rows) is at most 64: a block of a PIZ part whose cols AND rows are both 128 or more
 * is refused (RFX_EINVAL).  Scanline blocks of any width and tiles of up to 127 texels on their shorter side are taken.  The packed size equal to the raw size is the raw block, as for every compression.
 * THE DEVICE AREA grows by K9_PIZ_TABLE_BYTES (csrc/k9_piz.h: 257 KiB — the reverse lookup table, the sorted symbols) per PIZ block of the band that
 * is not stored raw (csrc/rfx_launch.h rfx_exr_piz_tables_for), under the growth rule of the staging areas.
 * STATUS.  rfx_exr_aov_status reports a bad PIZ block with csrc/k9_piz.h's K9_E_PIZ_* (15 .. 23); its rectangle reads as not covered. */
enum { RFX_EXR_PIZ = 4 };
size_t rfx_exr_blocks_piz_stage_bytes(const rfx_ctx *, const rfx_exr_block_frame *, int row0, int rows);
int    rfx_stage_exr_blocks_piz(rfx_ctx *, const rfx_exr_block_frame *, int row0, int rows);

/* ---- row-tiled runs: the exchanges, one process per GPU, RCCL over xGMI.  RCCL is bound at run time (a
 * single-GPU host needs none; a process that already maps an RCCL — e.g. torch's — shares it).
 * Tiles: rank r of n owns rfx_split_rows(height, n, r) — boundaries on even rows, the last tile takes the remainder.  The exchanges run on a second stream of the context: each call orders itself AFTER all draws
 * enqueued so far and returns; rfx_comm_wait orders all LATER draws after the exchanges issued so far.  In between the host may
 * enqueue draws that do not touch the rows in flight (the tile interior through rfx_set_row_window; rfx_ssgi_trace while the
 * composed GI is gathered), which is how their time is hidden.
 * Replaces nothing in the reference (it has no multi-GPU path); it is the halo step north_star / SURVEY.md §8e prescribe. */
int rfx_split_rows(int height, int nranks, int rank, int *tile_y0, int *tile_rows);
int rfx_comm_unique_id(void *id128);                                            /* ncclGetUniqueId: 128 bytes, rank 0 hands them to the others */
int rfx_comm_init(rfx_ctx *, const void *id128, int rank, int nranks);          /* ncclCommInitRank on the context's device (collective) */
int rfx_comm_destroy(rfx_ctx *);
/* ncclGroupStart; ncclSend/ncclRecv of halo_rows rows of texture `id` with the tile above (`up_rank`, higher frame rows) and
 * below (`down_rank`); ncclGroupEnd — -1 = no such neighbour.  `ncclComm` (an ncclComm_t) may be NULL: the context's own.
 * halo_rows taller than the split's tiles (many ranks, a fast camera: the band around a tile then reaches past its neighbours): every
 * tile whose rows lie inside this tile's band sends them directly, in the same group — that form needs rfx_comm_init on the context
 * (rank and size) and up / down = rank + 1 / rank - 1 (or -1). */
int rfx_halo_exchange(rfx_ctx *, rfx_tex id, void *ncclComm, int up_rank, int down_rank);
/* every rank's tile rows of RFX_TEX_COMPOSE or RFX_TEX_COMPOSE_RGB (held whole) to every rank, in place: next frame's K1 gathers
 * last frame's composed GI anywhere on screen.  ncclAllGather (equal tiles) or one ncclBroadcast per owner in a group (ragged). */
int rfx_allgather_history(rfx_ctx *, rfx_tex id, void *ncclComm);
/* The bounded form of that gather (ABI 15), called BETWEEN rfx_ssgi_trace and rfx_ssgi_shade: only the shading of a ray reads last
 * frame's composed GI, NEAREST at the ray's final uv (ssgi.frag:396-427), and after the trace those uvs are known.  The call reduces, on
 * the device, the ROW MASK of the history texels this tile's rays will read (ABI 16: one word per frame row, see rfx_ssgi_hit_mask; ABI 15
 * reduced one (min, max) row interval, which also moved every row between two needed ones), all-gathers the N masks, and moves with grouped
 * ncclSend / ncclRecv only the rows some rank needs from their owners (whose rows are current: K4 wrote them), in runs of consecutive
 * rows — instead of every rank receiving the other N - 1 tiles.  Bit-identical to the all-gather form.  It waits on the host for the N
 * masks (height words each; i.e. for the trace to finish); the row
 * transfers are asynchronous like the other exchanges (rfx_comm_wait before rfx_ssgi_shade).  `bytes_received` (may be NULL): what this
 * rank receives this frame.  A host uses EITHER this or rfx_allgather_history after K4. */
int rfx_gather_history_rows(rfx_ctx *, rfx_tex id, void *ncclComm, size_t *bytes_received);
/* The DEVICE-DRIVEN form of the bounded gather (ABI 19; csrc/rfx_peer.hip): no RCCL, no host wait, no packing.  xGMI lets a kernel load a
 * peer GPU's memory, so every rank exports the plane once (rfx_peer_export: RFX_PEER_BLOB_BYTES bytes holding HIP IPC handles of the plane and
 * of a small flag block; the host moves the N blobs to every rank by any means it has — they are plain bytes) and opens its peers'
 * (rfx_peer_open: `blobs` = the N blobs in rank order; the context's tile must be rfx_split_rows(height, nranks, rank)).  Then, per frame,
 * BETWEEN rfx_ssgi_trace and rfx_ssgi_shade and on EVERY rank, rfx_peer_gather_history enqueues on the exchange stream: a flag barrier through
 * the peers' mapped flag blocks ("every rank's compose draw of the previous frame has executed"), ONE kernel that walks this rank's own row
 * mask (rfx_ssgi_hit_mask's, already on the device) and copies the column blocks its rays will read straight out of their owners' planes, and
 * a second barrier ("every rank has pulled") that the next rfx_compose — which overwrites those rows — is ordered after.  The shade is ordered
 * after the pull by rfx_comm_wait, like the other exchanges.  Bit-identical to the all-gather form.  Nothing waits on the host:
 * `bytes_pulled_previous_call` (may be NULL) reports what the PREVIOUS call's kernel moved, and a peer that never reached a barrier (~2 s)
 * surfaces as RFX_EDEVICE from the next call instead of hanging the device.  The plane must be the library's own (not rfx_bind_external).
 * Contexts of one process (one per device, peer access enabled by the host) are recognised by the blob's process id and use each other's
 * addresses directly.  (Several contexts of one process on ONE device — a test set-up — work too, as long as their exchange streams sit on
 * different hardware queues: the barrier kernels of the ranks must be resident together, and the HIP runtime multiplexes a process's streams
 * onto GPU_MAX_HW_QUEUES (4) queues per device; with more streams than queues two barrier kernels can queue behind each other, and the call
 * after the bounded poll reports RFX_EDEVICE.  Set GPU_MAX_HW_QUEUES >= 4 x the contexts before the first HIP call.)  A host uses ONE of rfx_allgather_history / rfx_gather_history_rows / rfx_peer_gather_history. */
#define RFX_PEER_BLOB_BYTES 192
int rfx_peer_export(rfx_ctx *, rfx_tex id, void *blob);
int rfx_peer_open(rfx_ctx *, rfx_tex id, const void *blobs, int rank, int nranks);
int rfx_peer_gather_history(rfx_ctx *, rfx_tex id, size_t *bytes_pulled_previous_call);
int rfx_peer_close(rfx_ctx *);
/* The reduction on its own (any context, no communicator): after rfx_ssgi_trace, the inclusive range of history rows the shade of the
 * traced rows will read; row_hi < row_lo when it reads none (0x7fffffff, -1).  Blocks until the trace has finished.  A diagnostic: it is the
 * first and the last non-zero word of rfx_ssgi_hit_mask's mask, which it reads back whole (one word per frame row) to find them. */
int rfx_ssgi_hit_rows(rfx_ctx *, int *row_lo, int *row_hi);
/* ... and the mask form (ABI 16): row_mask[y], y in [0, height), gets bit b set when the shade of the traced rows reads a history texel of
 * frame row y in column block b (32 equal blocks across the frame: texel x is in block x * 32 / width); a row that is not read at all
 * gets 0.  `rows` must be the frame height.  Blocks until the trace has finished. */
int rfx_ssgi_hit_mask(rfx_ctx *, unsigned int *row_mask, int rows);
int rfx_comm_wait(rfx_ctx *);

/* Number of texel fetches that fell outside the rows a tile context holds since creation
 * (they are clamped into the band, i.e. the halo was too small for the frame's motion/radius).
 * 0 on a correct configuration; always 0 for a whole-frame context. */
unsigned int rfx_halo_violations(rfx_ctx *);

/* Timing helper: run `fn`-selected kernel `iters` times between two hipEvents on the context's
 * stream and return the mean milliseconds (used by bench.py for the roofline line). */
int rfx_time_begin(rfx_ctx *);
int rfx_time_end(rfx_ctx *, float *elapsed_ms);
/* Per-draw device timing INSIDE a frame loop (ABI 18; bench.py's `kernel_ms` and `roofline`).  rfx_profile(ctx, 1) resets the sums and makes every
 * draw entry point bracket the launches it makes with two hipEvents on the stream they run on (K1's depth pre-pass on its own stream, where it
 * overlaps the previous frame's later draws); rfx_profile(ctx, 0) stops.  rfx_profile_read waits for the recorded events and returns, per kind,
 * the summed milliseconds and the number of launches since the reset (arrays of RFX_PROF_COUNT entries; either may be NULL).  The events cost
 * a few microseconds per draw: the frame's own time (`value`) is measured without them.  At most 8192 launches are recorded per reset. */
enum { RFX_PROF_K1_PREPASS = 0, RFX_PROF_K1_MARCH, RFX_PROF_K2, RFX_PROF_K3_PASS0, RFX_PROF_K3_PASSN, RFX_PROF_K4, RFX_PROF_K5,
       RFX_PROF_K6, /* ABI 20: rfx_motion_blur */
       RFX_PROF_K6_REACH, /* ABI 21: the reach reduction of rfx_motion_blur_reach_mask / rfx_motion_blur_gather */
       RFX_PROF_K7, /* the encode of rfx_export / rfx_stage_export */
       RFX_PROF_COUNT };
/* Kinds added from here on do not grow RFX_PROF_COUNT: rfx_profile_read has no size argument and keeps filling exactly RFX_PROF_COUNT entries, so
 * a caller built against an earlier header is never overrun.  rfx_profile_read_n fills min(entries, RFX_PROF_COUNT_ALL) entries of each array
 * (the first RFX_PROF_COUNT are rfx_profile_read's) and is how the kinds below are read. */
enum { RFX_PROF_K8 = RFX_PROF_COUNT, /* the PNG encode of rfx_png / rfx_stage_png: its three launches on the download stream; the EXR encode of
                                       * rfx_exr / rfx_stage_exr (its four launches) is timed under this kind too */
       RFX_PROF_COUNT_ALL };
int rfx_profile(rfx_ctx *, int enable);
int rfx_profile_read(rfx_ctx *, float *ms_sum, int *launches);
int rfx_profile_read_n(rfx_ctx *, float *ms_sum, int *launches, int entries);

#ifdef __cplusplus
}
#endif
#endif /* RFX_H */
