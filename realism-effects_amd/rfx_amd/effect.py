"""Host-side mirror of the reference's operator interface for the hot path (Python flavour; the
Node flavour with the same surface lives in ../js).

Same class names, constructor signatures, option names, defaults and frame logic as the
reference's JS drivers; the device work each `render()` did through
`renderer.setRenderTarget(rt); renderer.render(scene, camera)` is one C-ABI call on a
`Context` (librfx_hip.so).  `scene` / `camera` are plain dumped-state objects (no three.js):

  camera  : rfx_amd.scene.Camera-like (projectionMatrix[Inverse], matrixWorld[Inverse], position,
            quaternion, near, far, isPerspectiveCamera) — updated by the caller every frame
  scene   : anything; only `scene.frame` (a dumped rfx_amd.scene.Frame) is read, by the
            raster shims (GBufferPass / VelocityDepthNormalPass) that stand where the
            reference rasterises
  renderer: an rfx_amd.context.Context (the device), passed to update()/render() like
            three's WebGLRenderer is.

Reference files mirrored (file:line in each class):
  src/ssgi/SSGIEffect.js, src/ssgi/SSGIOptions.js, src/ssgi/pass/SSGIPass.js,
  src/denoise/Denoiser.js, src/denoise/pass/PoissonDenoisePass.js,
  src/denoise/pass/DenoiserComposePass.js, src/temporal-reproject/TemporalReprojectPass.js,
  src/temporal-reproject/pass/VelocityDepthNormalPass.js, src/traa/TRAAEffect.js,
  src/utils/BlueNoiseUtils.js, src/utils/SceneUtils.js
"""
from __future__ import annotations

import math
import random

import numpy as np

from . import abi

# src/ssgi/SSGIOptions.js:26-48
defaultSSGIOptions = dict(
    mode="ssgi", distance=10, thickness=10, denoiseIterations=1, denoiseKernel=2, denoiseDiffuse=10, denoiseSpecular=10, radius=3,
    phi=0.5, lumaPhi=5, depthPhi=2, normalPhi=50, roughnessPhi=50, specularPhi=50, envBlur=0.5, importanceSampling=True, steps=20,
    refineSteps=5, resolutionScale=1, missedRays=False, outputTexture=None)

# src/temporal-reproject/TemporalReprojectPass.js:17-32
defaultTemporalReprojectPassOptions = dict(
    dilation=False, fullAccumulate=False, neighborhoodClamp=False, neighborhoodClampRadius=1, neighborhoodClampIntensity=1, maxBlend=1,
    logTransform=False, depthDistance=2, worldDistance=4, reprojectSpecular=False, renderTarget=None, copyTextures=True,
    confidencePower=0.75, inputType="diffuse")

# src/denoise/pass/PoissonDenoisePass.js:16-24
defaultPoissonBlurOptions = dict(iterations=1, radius=3, phi=0.5, lumaPhi=5, depthPhi=2, normalPhi=3.25, inputType="diffuseSpecular")

# src/denoise/Denoiser.js:6-11
defaultDenoiserOptions = dict(denoiseMode="full", inputType="diffuseSpecular", gBufferPass=None, velocityDepthNormalPass=None)

_INPUT_TYPES = ["diffuseSpecular", "diffuse", "specular"]
# three.js texture `type` constants the path distinguishes (three/src/constants.js)
UnsignedByteType, FloatType, HalfFloatType = 1009, 1015, 1016


def _texture_type(texture) -> int:
    """`texture.type` of an input texture: a three-style object/dict carrying `type`, or a bare slot id / None for the
    FloatType targets the SSGI chain passes around (SSGIPass.js:24)."""
    t = getattr(texture, "type", None)
    if t is None and isinstance(texture, dict):
        t = texture.get("type")
    return FloatType if t is None else int(t)


class StateError(ValueError):
    """A saved temporal state (rfx_amd.state) that does not fit the running effect; `field` names what differs."""

    def __init__(self, field, message):
        super().__init__("%s: %s" % (field, message))
        self.field = field


# Saved host state keeps every float as the hex of its little-endian IEEE bytes: bit for bit, and the same text from both hosts
def _hex32(values) -> str:
    return np.asarray(values, "<f4").tobytes().hex()


def _hex64(values) -> str:
    return np.asarray(values, "<f8").tobytes().hex()


def _unhex(text, dtype, count, field):
    try:
        a = np.frombuffer(bytes.fromhex(text), dtype)
    except (TypeError, ValueError):
        raise StateError(field, "not the hex of %s values" % np.dtype(dtype).name)
    if a.size != count:
        raise StateError(field, "%d values, expected %d" % (a.size, count))
    return a


_CAMERA_FIELDS = (("projectionMatrix", 16), ("projectionMatrixInverse", 16), ("matrixWorld", 16), ("matrixWorldInverse", 16), ("position", 3))


def _camera_state(c: abi.Camera) -> dict:
    """An abi.Camera (what the device is handed: float32) as saved state."""
    s = {name: _hex32(list(getattr(c, name))) for name, _ in _CAMERA_FIELDS}
    s.update(near=_hex32([c.near_]), far=_hex32([c.far_]), isPerspective=int(c.isPerspective))
    return s


def _camera_from_state(s, field) -> abi.Camera:
    c = abi.Camera()
    if not isinstance(s, dict):
        raise StateError(field, "missing")
    for name, n in _CAMERA_FIELDS:
        getattr(c, name)[:] = [float(x) for x in _unhex(s.get(name), "<f4", n, field + "." + name)]
    c.near_ = float(_unhex(s.get("near"), "<f4", 1, field + ".near")[0])
    c.far_ = float(_unhex(s.get("far"), "<f4", 1, field + ".far")[0])
    c.isPerspective = _state_int(s, "isPerspective", field)
    return c


def _state_int(s, key, field, allow_none=False):
    v = s.get(key) if isinstance(s, dict) else None
    if v is None and allow_none and isinstance(s, dict) and key in s:
        return None
    if isinstance(v, bool) or not isinstance(v, int):
        raise StateError(field + "." + key, "an integer is expected, got %r" % (v,))
    return v


def _state_dict(s, key, field):
    v = s.get(key) if isinstance(s, dict) else None
    if not isinstance(v, dict):
        raise StateError(field + "." + key, "missing")
    return v


# src/taa/TAAUtils.js:3 + src/temporal-reproject/utils/QuasirandomGenerator.js:12-27 (JS doubles)
def _generate_r2(count):
    g = 1.32471795724474602596090885447809
    a1, a2, base = 1.0 / g, 1.0 / (g * g), 1.1127756842787055
    return [[math.fmod(base + a1 * n, 1.0), math.fmod(base + a2 * n, 1.0)] for n in range(count)]


r2Sequence = [[a - 0.5, b - 0.5] for a, b in _generate_r2(256)]


def jitter(width, height, camera, frame, jitterScale=1):
    """src/taa/TAAUtils.js:5-11.  `camera.setViewOffset` is three's PerspectiveCamera method; the dumped-state camera of
    this host records the offset for the raster side (which renders the next dump with it) when it has one."""
    x, y = r2Sequence[frame % len(r2Sequence)]
    if hasattr(camera, "setViewOffset"):
        camera.setViewOffset(width, height, x * jitterScale, y * jitterScale, width, height)
    return x * jitterScale, y * jitterScale
HIGHEST_SIGNED_INT = 0x7FFFFFFF


class BlueNoiseIndex:
    """The `blueNoiseIndex` uniform getter of src/utils/BlueNoiseUtils.js:17-33: every READ (one
    per draw of the material) advances `(startIndex + idx + 1) % 0x7fffffff`; `startIndex` is
    random per material unless pinned for reproducible runs."""

    def __init__(self, start_index: int | None = None):
        self.start_index = int(start_index) if start_index is not None else int(math.floor(random.random() * HIGHEST_SIGNED_INT))
        self._idx = 0

    @property
    def value(self) -> int:
        self._idx = (self.start_index + self._idx + 1) % HIGHEST_SIGNED_INT
        return self._idx

    @value.setter
    def value(self, v: int):
        self._idx = int(v)

    def get_state(self) -> dict:
        return dict(startIndex=self.start_index, index=self._idx)

    def check_state(self, s, field):
        _state_int(s, "startIndex", field)
        _state_int(s, "index", field)

    def set_state(self, s):
        self.start_index, self._idx = int(s["startIndex"]), int(s["index"])


def didCameraMove(camera, last_position, last_quaternion) -> bool:
    """src/utils/SceneUtils.js:17-27."""
    p = np.asarray(camera.position, np.float64)
    if float(((p - last_position) ** 2).sum()) > 0.000001:
        return True
    q = np.asarray(getattr(camera, "quaternion", (0, 0, 0, 1)), np.float64)
    d = abs(float(np.clip(np.dot(q, last_quaternion), -1, 1)))
    return 2 * math.acos(d) > 0.001  # Quaternion.angleTo


def _upload_plane(renderer, tex, plane, static=False):
    """Hand one dumped full-frame plane to the device (the slot takes the band it holds).  The reference re-renders its raster passes
    every frame; so does this — every call uploads — unless the dump DECLARES itself unchanged (`scene.frame.static = True`): then a
    plane object that is already resident (same ndarray as last time) is not sent again.  Opt-in because identity says nothing about
    contents: a caller that refills a preallocated buffer in place (the normal per-frame dump loop) hands over the same object every
    frame with new texels in it."""
    cache = renderer.__dict__.setdefault("_resident_planes", {})
    if static == "resident" or (static and cache.get(tex) is plane):
        return  # "resident": the caller streamed the planes itself (Context.stage_frame / stage_flip)
    r0, n = renderer.held_rows(tex)
    if plane.shape[0] == n:  # the caller dumped exactly the band this tile holds
        renderer.upload(tex, plane, r0, n)
    else:
        renderer.upload(tex, plane[r0:r0 + n], r0, n)
    cache[tex] = plane


def _pack_planes(renderer, tex, aov, depth, pack, static=False):
    """Device-side packing of a dumped frame's attribute planes into `tex` (skipped only for a `static` frame's resident aov and for a frame
    the caller streamed itself — "resident": Context.stage_aov / stage_flip — like _upload_plane)."""
    cache = renderer.__dict__.setdefault("_resident_planes", {})
    if static == "resident" or (static and cache.get(tex) is aov):
        return
    r0, n = renderer.held_rows(tex)
    full = depth.shape[0] != n  # the caller dumped the whole frame: hand over the band this tile holds
    band = {k: (v[r0:r0 + n] if full else v) for k, v in aov.items()}
    pack(band, depth[r0:r0 + n] if full else depth, r0, n)
    cache[tex] = aov


class GBufferPass:
    """Stand-in for src/gbuffer/GBufferPass.js: the rasteriser is out of scope;
    `render` uploads the pre-dumped packed G-buffer + depth planes of `scene.frame`."""

    def __init__(self, scene, camera):
        self._scene, self._camera = scene, camera
        self.texture, self.depthTexture = abi.TEX_GBUFFER, abi.TEX_DEPTH

    def setSize(self, width, height):
        self.width, self.height = width, height

    def render(self, renderer):
        f = self._scene.frame
        _upload_plane(renderer, abi.TEX_DEPTH, f.depth, getattr(f, "static", False))
        if getattr(f, "gbuffer", None) is not None:
            _upload_plane(renderer, abi.TEX_GBUFFER, f.gbuffer, getattr(f, "static", False))
        else:  # an engine dump of UNPACKED attribute planes: the device packs them (rfx_pack_gbuffer = the pass's fragment epilogue)
            _pack_planes(renderer, abi.TEX_GBUFFER, f.aov, f.depth, renderer.pack_gbuffer, getattr(f, "static", False))

    def dispose(self):
        pass


class VelocityDepthNormalPass:
    """src/temporal-reproject/pass/VelocityDepthNormalPass.js:66 — kept as a loader shim: the
    class, its (scene, camera) signature and `texture`/`renderTarget` accessors survive, the
    raster work is replaced by uploading the dumped RGBA32F plane (format :186-188)."""

    def __init__(self, scene, camera):
        self._scene, self._camera = scene, camera
        self.renderTarget = self
        self.texture = abi.TEX_VELOCITY
        self.depthTexture = abi.TEX_VELOCITY
        self.lastVelocityTexture = None  # declared by the reference, never read by K2 (Appendix D-6)

    def setSize(self, width, height):
        self.width, self.height = width, height

    def render(self, renderer):
        f = self._scene.frame
        if getattr(f, "velocity", None) is not None:
            _upload_plane(renderer, abi.TEX_VELOCITY, f.velocity, getattr(f, "static", False))
        else:  # unpacked planes (uv-space velocity, world normal, depth): rfx_pack_velocity
            _pack_planes(renderer, abi.TEX_VELOCITY, f.aov, f.depth, renderer.pack_velocity, getattr(f, "static", False))

    def dispose(self):
        pass


class TemporalReprojectPass:
    """src/temporal-reproject/TemporalReprojectPass.js:38-225."""

    def __init__(self, scene, camera, velocityDepthNormalPass, texture, textureCount, options=None, half_store_rtz=True):
        self._scene, self._camera = scene, camera
        self.textureCount = textureCount
        o = dict(defaultTemporalReprojectPassOptions)
        o.update(options or {})
        self.options = o
        self.velocityDepthNormalPass = velocityDepthNormalPass
        self.frame = 0
        self.overrideAccumulatedTextures = []
        self.lastCameraTransform = dict(position=np.zeros(3), quaternion=np.array([0.0, 0, 0, 1]))
        # :63-68 the render target takes the TYPE of the input texture; :137-142 so does the framebuffer copy
        self.targetType = _texture_type(texture)
        if self.targetType not in (FloatType, HalfFloatType):
            raise ValueError("TemporalReprojectPass: input texture type %r — only FloatType / HalfFloatType targets are built" % (self.targetType,))
        it = _INPUT_TYPES.index(o["inputType"]) if o["inputType"] in _INPUT_TYPES else 1
        p = abi.TemporalParams(textureCount=textureCount, inputType=it, logTransform=1 if o["logTransform"] else 0,
                               confidencePower=float(o["confidencePower"]), neighborhoodClampIntensity=float(o["neighborhoodClampIntensity"]),
                               maxBlend=float(o["maxBlend"]), keepData=1.0, targetHalf=1 if self.targetType == HalfFloatType else 0,
                               halfStoreRTZ=1 if half_store_rtz else 0)
        for name in ("reprojectSpecular", "neighborhoodClamp"):  # :109-116 — arrays of (arrays of) bools; indices 0,1 matter
            v = o[name]
            v = list(v) if isinstance(v, (list, tuple)) else [v] * 2
            getattr(p, name)[:] = [1 if x else 0 for x in (v + v)[:2]]
        self.uniforms = p
        # :95-104 the ctor clones the current camera state into the prev* uniforms
        self._prev = abi.Camera.from_scene(camera)

    def setSize(self, width, height):
        self.width, self.height = width, height

    @property
    def texture(self):
        return abi.TEX_TEMPORAL0

    @property
    def framebufferTexture(self):
        """:137-142 — the slot the pass copies its target into when nothing overrides its history."""
        return abi.TEX_FBCOPY_F16 if self.targetType == HalfFloatType else abi.TEX_FBCOPY_F32

    def reset(self):
        self.uniforms.keepData = 0.0  # :158-160

    def render(self, renderer):
        self.frame = (self.frame + 1) % 4096
        cam = self._camera
        # :168-172,185-187 the pass draws with the UNJITTERED projection (view offset disabled while the uniforms are read)
        self.uniforms.camera = abi.Camera.from_scene(getattr(cam, "unjittered", cam))
        self.uniforms.prevCamera = self._prev
        moved = didCameraMove(cam, self.lastCameraTransform["position"], self.lastCameraTransform["quaternion"])
        self.uniforms.fullAccumulate = 1 if (self.options["fullAccumulate"] and not moved) else 0  # :178-180
        self.lastCameraTransform["position"] = np.asarray(cam.position, np.float64).copy()
        self.lastCameraTransform["quaternion"] = np.asarray(getattr(cam, "quaternion", (0, 0, 0, 1)), np.float64).copy()
        own_history = len(self.overrideAccumulatedTextures) == 0  # :148-151
        self.uniforms.historySource = 0 if not own_history else (1 if self.targetType == HalfFloatType else 2)
        renderer.temporal_reproject(self.uniforms)  # :192-193
        self.uniforms.keepData = 1.0  # :195
        if own_history:  # :197-201
            renderer.copy_framebuffer(self.framebufferTexture)
            hook = getattr(renderer, "after_copy_framebuffer", None)
            if hook:
                hook(self.framebufferTexture)  # multi-GPU: halo exchange of the history rows
        self._prev = abi.Camera.from_scene(getattr(cam, "unjittered", cam))  # :203-213

    # -- saved temporal state (rfx_amd.state)
    def state_slots(self):
        """The slots a later frame reads before writing, or leaves partly unwritten (K2 discards background texels)."""
        slots = [abi.TEX_TEMPORAL0] + ([abi.TEX_TEMPORAL1] if self.textureCount == 2 else [])
        if len(self.overrideAccumulatedTextures) == 0:
            slots.append(self.framebufferTexture)
        return slots

    def get_state(self) -> dict:
        return dict(frame=self.frame, textureCount=self.textureCount, targetType=self.targetType, keepData=_hex32([self.uniforms.keepData]),
                    prevCamera=_camera_state(self._prev),
                    lastCameraTransform=dict(position=_hex64(self.lastCameraTransform["position"]),
                                             quaternion=_hex64(self.lastCameraTransform["quaternion"])))

    def check_state(self, s, field):
        if _state_int(s, "textureCount", field) != self.textureCount:
            raise StateError(field + ".textureCount", "saved %d, the running pass has %d" % (s["textureCount"], self.textureCount))
        if _state_int(s, "targetType", field) != self.targetType:
            raise StateError(field + ".targetType", "saved %d, the running pass has %d (FloatType %d, HalfFloatType %d)" % (
                s["targetType"], self.targetType, FloatType, HalfFloatType))
        _state_int(s, "frame", field)
        _unhex(s.get("keepData"), "<f4", 1, field + ".keepData")
        _camera_from_state(s.get("prevCamera"), field + ".prevCamera")
        t = _state_dict(s, "lastCameraTransform", field)
        _unhex(t.get("position"), "<f8", 3, field + ".lastCameraTransform.position")
        _unhex(t.get("quaternion"), "<f8", 4, field + ".lastCameraTransform.quaternion")

    def set_state(self, s):
        self.frame = int(s["frame"])
        self.uniforms.keepData = float(_unhex(s["keepData"], "<f4", 1, "keepData")[0])
        self._prev = _camera_from_state(s["prevCamera"], "prevCamera")
        t = s["lastCameraTransform"]
        self.lastCameraTransform = dict(position=_unhex(t["position"], "<f8", 3, "position").astype(np.float64),
                                        quaternion=_unhex(t["quaternion"], "<f8", 4, "quaternion").astype(np.float64))

    def jitter(self, jitterScale=1):  # :216-220
        self.unjitter()
        return jitter(self.width, self.height, self._camera, self.frame, jitterScale)

    def unjitter(self):  # :222-224
        if hasattr(self._camera, "clearViewOffset"):
            self._camera.clearViewOffset()

    def dispose(self):
        pass


class PoissonDenoisePass:
    """src/denoise/pass/PoissonDenoisePass.js:26-152."""

    DefaultOptions = defaultPoissonBlurOptions

    def __init__(self, camera, textures, options=None, blue_noise_start=None, half_store_rtz=True):
        o = dict(defaultPoissonBlurOptions)
        o.update(options or {})
        self.iterations = defaultPoissonBlurOptions["iterations"]
        self.textures = textures
        spec = [0, 1]
        if o["inputType"] == "diffuse":
            spec = [0, 0]
        if o["inputType"] == "specular":
            spec = [1, 1]
        tc = 2 if o["inputType"] == "diffuseSpecular" else 1
        d = defaultPoissonBlurOptions
        # :48-66 — roughnessPhi/specularPhi start `undefined` until SSGIEffect's setters write them
        self.uniforms = abi.DenoiseParams(radius=d["radius"], phi=d["phi"], lumaPhi=d["lumaPhi"], depthPhi=float(o["depthPhi"]),
                                          normalPhi=float(o["normalPhi"]), roughnessPhi=float("nan"), specularPhi=float("nan"),
                                          textureCount=tc, halfStoreRTZ=1 if half_store_rtz else 0)
        self.uniforms.isTextureSpecular[:] = spec
        self.blueNoiseIndex = BlueNoiseIndex(blue_noise_start)

    def setSize(self, width, height):
        self.width, self.height = width, height

    @property
    def texture(self):
        return (abi.TEX_DENOISE_B0, abi.TEX_DENOISE_B1)

    def render(self, renderer):
        for i in range(2 * int(self.iterations)):  # :135-149
            horizontal = i % 2 == 0
            self.uniforms.inputIsTemporal = 1 if i == 0 else 0
            self.uniforms.writeToB = 0 if horizontal else 1
            self.uniforms.blueNoiseIndex = self.blueNoiseIndex.value
            renderer.poisson_denoise(self.uniforms)
            hook = getattr(renderer, "after_denoise_pass", None)
            if hook:
                hook(i, self.uniforms)  # multi-GPU: halo exchange of the target just written

    # -- saved temporal state (rfx_amd.state)
    def state_slots(self):
        """Both ping-pong targets: K3 discards background texels, which keep what the target held; B is also K2's history."""
        n = self.uniforms.textureCount
        return [abi.TEX_DENOISE_A0, abi.TEX_DENOISE_A1][:n] + [abi.TEX_DENOISE_B0, abi.TEX_DENOISE_B1][:n]

    def get_state(self) -> dict:
        return dict(textureCount=int(self.uniforms.textureCount), blueNoiseIndex=self.blueNoiseIndex.get_state())

    def check_state(self, s, field):
        if _state_int(s, "textureCount", field) != self.uniforms.textureCount:
            raise StateError(field + ".textureCount", "saved %d, the running pass has %d" % (s["textureCount"], self.uniforms.textureCount))
        self.blueNoiseIndex.check_state(_state_dict(s, "blueNoiseIndex", field), field + ".blueNoiseIndex")

    def set_state(self, s):
        self.blueNoiseIndex.set_state(s["blueNoiseIndex"])

    def dispose(self):
        pass


class DenoiserComposePass:
    """src/denoise/pass/DenoiserComposePass.js:8-136."""

    def __init__(self, camera, textures, gBufferTexture, depthTexture, options=None):
        self._camera = camera
        o = options or {}
        it = _INPUT_TYPES.index(o.get("inputType", "diffuseSpecular")) if o.get("inputType", "diffuseSpecular") in _INPUT_TYPES else 0
        # Denoiser.js:53 composerInputTextures: the denoise pass's targets, or (denoiseMode "full_temporal") K2's own
        src = 1 if tuple(textures)[0] == abi.TEX_TEMPORAL0 else 0
        self.uniforms = abi.ComposeParams(inputType=it, giSource=src)

    def setSize(self, width, height):
        self.width, self.height = width, height

    @property
    def texture(self):
        return abi.TEX_COMPOSE

    def render(self, renderer):
        self.uniforms.camera = abi.Camera.from_scene(self._camera)
        # a row-tiled renderer all-gathers the part of this target K1 reads next frame (.rgb) as 12-byte texels
        self.uniforms.writeHistoryRGB = 1 if getattr(renderer, "gather_history_rgb", False) else 0
        renderer.compose(self.uniforms)

    def dispose(self):
        pass


class Denoiser:
    """src/denoise/Denoiser.js:16-108 — temporal + spatial + compose chain."""

    def __init__(self, scene, camera, texture, options=None, blue_noise_start=None, half_store_rtz=True):
        o = dict(defaultDenoiserOptions)
        o.update(options or {})
        self.options = o
        self.velocityDepthNormalPass = o["velocityDepthNormalPass"] or VelocityDepthNormalPass(scene, camera)
        self.isOwnVelocityDepthNormalPass = not o["velocityDepthNormalPass"]
        textureCount = 2 if o["inputType"] == "diffuseSpecular" else 1
        topt = dict(fullAccumulate=True, logTransform=True, copyTextures=not o.get("denoise"), reprojectSpecular=[False, True],
                    neighborhoodClamp=[True, True], neighborhoodClampRadius=2, neighborhoodClampIntensity=0.5)
        topt.update({k: v for k, v in o.items() if k in defaultTemporalReprojectPassOptions})
        self.temporalReprojectPass = TemporalReprojectPass(scene, camera, self.velocityDepthNormalPass, texture, textureCount, topt)
        self.denoisePass = None
        self.denoiserComposePass = None
        if o["denoiseMode"] in ("full", "denoised"):
            popt = {k: v for k, v in o.items() if k in defaultPoissonBlurOptions}
            self.denoisePass = PoissonDenoisePass(camera, (abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1), popt, blue_noise_start, half_store_rtz)
            self.temporalReprojectPass.overrideAccumulatedTextures = list(self.denoisePass.texture)
        if o["denoiseMode"] not in ("full", "full_temporal", "denoised", "temporal"):
            raise ValueError("denoiseMode %r" % (o["denoiseMode"],))
        textures = (abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1)[:textureCount]
        composerInputTextures = self.denoisePass.texture if self.denoisePass else textures  # :53
        if o["denoiseMode"].startswith("full"):
            self.denoiserComposePass = DenoiserComposePass(camera, composerInputTextures, abi.TEX_GBUFFER, abi.TEX_DEPTH, o)

    @property
    def texture(self):
        m = self.options["denoiseMode"]
        if m in ("full", "full_temporal"):
            return self.denoiserComposePass.texture
        if m == "denoised":
            return self.denoisePass.texture
        return self.temporalReprojectPass.texture

    def reset(self):
        self.temporalReprojectPass.reset()

    # -- saved temporal state (rfx_amd.state)
    def state_slots(self):
        slots = self.temporalReprojectPass.state_slots()
        if self.denoisePass:
            slots += self.denoisePass.state_slots()
        if self.denoiserComposePass:
            slots.append(self.denoiserComposePass.texture)  # K1's history; K4 discards background texels
        return slots

    def get_state(self) -> dict:
        return dict(denoiseMode=self.options["denoiseMode"], temporalReprojectPass=self.temporalReprojectPass.get_state(),
                    denoisePass=self.denoisePass.get_state() if self.denoisePass else None)

    def check_state(self, s, field):
        if s.get("denoiseMode") != self.options["denoiseMode"]:
            raise StateError(field + ".denoiseMode", "saved %r, the running effect has %r" % (s.get("denoiseMode"), self.options["denoiseMode"]))
        self.temporalReprojectPass.check_state(_state_dict(s, "temporalReprojectPass", field), field + ".temporalReprojectPass")
        if self.denoisePass:
            self.denoisePass.check_state(_state_dict(s, "denoisePass", field), field + ".denoisePass")

    def set_state(self, s):
        self.temporalReprojectPass.set_state(s["temporalReprojectPass"])
        if self.denoisePass:
            self.denoisePass.set_state(s["denoisePass"])

    def setSize(self, width, height):
        for p in (self.velocityDepthNormalPass, self.temporalReprojectPass, self.denoisePass, self.denoiserComposePass):
            if p:
                p.setSize(width, height)

    def dispose(self):
        pass

    def render(self, renderer, inputBuffer=None):
        if self.isOwnVelocityDepthNormalPass:
            self.velocityDepthNormalPass.render(renderer)
        self.temporalReprojectPass.render(renderer)
        hook = getattr(renderer, "after_temporal_pass", None)
        if hook:
            hook()
        if self.denoisePass:
            self.denoisePass.render(renderer)
        if self.denoiserComposePass:
            self.denoiserComposePass.render(renderer)
            hook = getattr(renderer, "after_compose_pass", None)
            if hook:
                hook()


class SSGIPass:
    """src/ssgi/pass/SSGIPass.js:7-96."""

    def __init__(self, ssgiEffect, options, blue_noise_start=None):
        self.ssgiEffect = ssgiEffect
        self._scene, self._camera = ssgiEffect._scene, ssgiEffect._camera
        self.frame = 21483
        mode = ["ssgi", "ssr"].index(options["mode"])
        self.uniforms = abi.SsgiParams(steps=20, refineSteps=5, mode=mode, useDirectLight=0, missedRays=0, importanceSampling=0)
        self.blueNoiseIndex = BlueNoiseIndex(blue_noise_start)
        self.gBufferPass = GBufferPass(self._scene, self._camera)

    @property
    def texture(self):
        return abi.TEX_SSGI

    def setSize(self, width, height):
        # :52-57 the pass's render target (and its `resolution` uniform) is width*resolutionScale x height*resolutionScale
        s = float(self.ssgiEffect._options["resolutionScale"])
        self.renderTargetSize = (width * s, height * s) if width is not None else (None, None)
        self.uniforms.resolutionScale = s
        self.gBufferPass.setSize(width, height)

    def render(self, renderer):
        self.frame = (self.frame + 1) % 4096
        self.gBufferPass.render(renderer)
        self.uniforms.camera = abi.Camera.from_scene(self._camera)
        self.uniforms.blueNoiseIndex = self.blueNoiseIndex.value
        # :89 accumulatedTexture = ssgiEffect.denoiser.texture: K4's target, K2's texture[0] ("temporal"), or — "denoised", where the
        # getter returns the ARRAY of K3's targets — what three binds for a non-texture value: its empty texture (zeros)
        t = self.ssgiEffect.denoiser.texture
        self.uniforms.historySource = 2 if isinstance(t, (tuple, list)) else (1 if t == abi.TEX_TEMPORAL0 else 0)
        if self.uniforms.historySource == 0 and getattr(renderer, "gather_history_rgb", False):
            self.uniforms.historySource = 3  # the same values from RFX_TEX_COMPOSE_RGB (tiling.py)
        if getattr(renderer, "overlap_history_gather", False):
            # row-tiled run: last frame's composed GI is still being all-gathered; only the shading half of the draw reads it
            renderer.ssgi_trace(self.uniforms)
            renderer.before_ssgi_shade()
            renderer.ssgi_shade(self.uniforms)
        else:
            renderer.ssgi_march(self.uniforms)  # :93-94

    # -- saved temporal state (rfx_amd.state); K1 writes every texel of its target, so the pass keeps no slot
    def get_state(self) -> dict:
        return dict(frame=self.frame, blueNoiseIndex=self.blueNoiseIndex.get_state())

    def check_state(self, s, field):
        _state_int(s, "frame", field)
        self.blueNoiseIndex.check_state(_state_dict(s, "blueNoiseIndex", field), field + ".blueNoiseIndex")

    def set_state(self, s):
        self.frame = int(s["frame"])
        self.blueNoiseIndex.set_state(s["blueNoiseIndex"])

    def dispose(self):
        pass


NearestFilter, LinearFilter, LinearMipmapLinearFilter = 1003, 1006, 1008


class CubeToEquirectEnvPass:
    """src/ssgi/pass/CubeToEquirectEnvPass.js: `scene.environment` given as a CubeTexture is rendered into an equirectangular FloatType
    target (one textureCube lookup per texel), read back, and continues as a DataTexture.  The cube as dumped state: an object/dict with
    `isCubeTexture`, `faces` ((6, S, S, 4) float32 linear values, +X -X +Y -Y +Z -Z, row j = t as uploaded), and the two sampler fields
    the lookup depends on: `minFilter` (default LinearMipmapLinearFilter, three's Texture default) and `generateMipmaps` (default True)."""

    def generateEquirectEnvMap(self, renderer, cubeMap, width=None, height=None, maxWidth=4096, on_device=False):
        """on_device: the draw's target stays on the device and becomes the environment there (renderer.set_environment_cube); the DataTexture
        returned then carries no `data`."""
        get = (lambda k, d=None: cubeMap.get(k, d)) if isinstance(cubeMap, dict) else (lambda k, d=None: getattr(cubeMap, k, d))
        faces = np.ascontiguousarray(get("faces"), np.float32)
        if width is None and height is None:  # :62-69
            w = faces.shape[1]
            width = int(2 ** math.ceil(math.log2(2 * w * 3 ** 0.5)))
            height = int(2 ** math.ceil(math.log2(w * 3 ** 0.5)))
        if width > maxWidth:  # :71-74
            width, height = maxWidth, maxWidth // 2
        min_filter = get("minFilter", LinearMipmapLinearFilter)
        if min_filter == LinearMipmapLinearFilter:
            if not get("generateMipmaps", True):
                raise ValueError("CubeToEquirectEnvPass: a LinearMipmapLinearFilter cube texture without generated mipmaps is incomplete (samples black)")
            mips = True
        elif min_filter == LinearFilter:
            mips = False
        else:
            raise NotImplementedError("CubeToEquirectEnvPass: cube minFilter %r — LinearFilter and LinearMipmapLinearFilter are built" % (min_filter,))
        if on_device:
            renderer.set_environment_cube(faces, width, height, generate_mipmaps=mips)
            return dict(data=None, type=FloatType, generateMipmaps=False, isCubeTexture=False)
        data = renderer.cube_to_equirect(faces, width, height, generate_mipmaps=mips)  # render + readRenderTargetPixels :76-85
        # :87-97 DataTexture(pixelBuffer, width, height, RGBAFormat, FloatType), ClampToEdge, EquirectangularReflectionMapping
        return dict(data=data, type=FloatType, generateMipmaps=False, isCubeTexture=False)

    def dispose(self):
        pass


class SSGIEffect:
    """src/ssgi/SSGIEffect.js:27-439 — owns SSGIPass + Denoiser, reactive options."""

    DefaultOptions = defaultSSGIOptions

    def __init__(self, composer, scene, camera, options=None, seeds=None, half_store_rtz=True, env_on_device=False):
        options = dict(defaultSSGIOptions, **(options or {}))
        self._scene, self._camera, self.composer = scene, camera, composer
        # keepEnvMapUpdated keeps a changed scene.environment on the device where the renderer can (Context.has_env_device): a cube becomes the
        # environment without a read-back, the importance tables are built by K10 — the same bits as the host path, no host wait
        self._env_on_device = bool(env_on_device)
        self.isUsingRenderPass = True
        if options["mode"] == "ssr":  # :70-73
            options["reprojectSpecular"] = True
            options["neighborhoodClamp"] = True
            options["inputType"] = "specular"
        elif options["mode"] == "ssgi":  # :74-77
            options["reprojectSpecular"] = [False, True]
            options["neighborhoodClamp"] = [False, True]
        preset = options.get("preset")
        if isinstance(preset, str):  # :79-99 (the second `case "medium"` is unreachable)
            if preset == "low":
                options.update(steps=10, refineSteps=2, denoiseMode="full_temporal")
            elif preset == "medium":
                options.update(steps=20, refineSteps=4, denoiseMode="full")
        seeds = seeds or {}
        self._options = options
        self._half_store_rtz = half_store_rtz
        self.ssgiPass = SSGIPass(self, options, seeds.get("ssgi"))
        dopt = dict(gBufferPass=self.ssgiPass.gBufferPass, velocityDepthNormalPass=options.get("velocityDepthNormalPass"))
        dopt.update(options)
        self.denoiser = Denoiser(scene, camera, self.ssgiPass.texture, dopt, seeds.get("denoise"), half_store_rtz)
        self.lastSize = dict(width=options.get("width"), height=options.get("height"), resolutionScale=options["resolutionScale"])
        self.setSize(options.get("width"), options.get("height"))
        self.uniforms = abi.FinalParams(camera=abi.Camera.from_scene(camera), isDebug=0, fogMode=0)  # FinalSSGIMaterial :47-66
        self._reactive = False
        for key in list(options.keys()):  # makeOptionsReactive :157-268 — apply every option once
            self._apply(key, options[key])
        self._reactive = True
        self.outputTexture = self.denoiser.texture
        # the composer's RenderPass has run before update(): direct light is available (:124-138,143-151)
        self.updateUsingRenderPass()

    # reactive option surface: effect.<option> reads/writes go through _apply like the JS setters
    def __getattr__(self, key):
        o = self.__dict__.get("_options")
        if o is not None and key in o:
            return o[key]
        raise AttributeError(key)

    def __setattr__(self, key, value):
        o = self.__dict__.get("_options")
        if o is not None and key in o and self.__dict__.get("_reactive"):
            if o[key] == value:
                return
            o[key] = value
            self._apply(key, value)
        else:
            object.__setattr__(self, key, value)

    def _apply(self, key, value):
        dp = self.denoiser.denoisePass
        if key == "denoiseIterations":
            if dp:
                dp.iterations = value
        elif key in ("radius", "phi", "lumaPhi", "depthPhi", "normalPhi", "roughnessPhi", "specularPhi"):
            if dp:
                setattr(dp.uniforms, key, float(value))
                self.reset()
        elif key == "resolutionScale":
            self.setSize(self.lastSize["width"], self.lastSize["height"])
            self.reset()
        elif key in ("steps", "refineSteps"):
            setattr(self.ssgiPass.uniforms, key, int(value))
            self.reset()
        elif key == "importanceSampling":
            # only effective with an env map (SSGIEffect.js:344-354): keepEnvMapUpdated re-reads the option when the environment is (re)set
            object.__setattr__(self, "_env_uuid", None)
            self.reset()
        elif key == "missedRays":
            self.ssgiPass.uniforms.missedRays = 1 if value else 0
            self.reset()
        elif key == "distance":
            self.ssgiPass.uniforms.rayDistance = float(value)
            self.reset()
        elif key in ("thickness", "envBlur"):  # default branch: a uniform of the same name
            setattr(self.ssgiPass.uniforms, key, float(value))
            self.reset()
        # denoiseKernel / denoiseDiffuse / denoiseSpecular: accepted, no consumer (Appendix D-3)

    def updateUsingRenderPass(self):
        self.ssgiPass.uniforms.useDirectLight = 1 if self.isUsingRenderPass else 0

    def reset(self):
        self.denoiser.reset()

    # -- saved temporal state (rfx_amd.state).  Options that are plain uniforms (radius, phi, steps, ...) are not part of it: they may be
    # changed between frames, as in the reference.  The environment and its importance tables are inputs: the caller sets
    # scene.environment again and the first update() after set_state() hands it to the device WITHOUT the reset of :356.
    def state_slots(self):
        return self.denoiser.state_slots()

    def get_state(self) -> dict:
        return {"class": type(self).__name__, "resolutionScale": _hex64([self._options["resolutionScale"]]), "ssgiPass": self.ssgiPass.get_state(),
                "denoiser": self.denoiser.get_state(), "finalCamera": _camera_state(self.uniforms.camera),
                "useEnvMap": int(self.ssgiPass.uniforms.useEnvMap)}

    def check_state(self, s, field="effect"):
        if s.get("class") != type(self).__name__:
            raise StateError(field + ".class", "saved %r, the running effect is %r" % (s.get("class"), type(self).__name__))
        scale = float(_unhex(s.get("resolutionScale"), "<f8", 1, field + ".resolutionScale")[0])
        if scale != float(self._options["resolutionScale"]):
            raise StateError(field + ".resolutionScale", "saved %r, the running effect has %r" % (scale, self._options["resolutionScale"]))
        self.denoiser.check_state(_state_dict(s, "denoiser", field), field + ".denoiser")
        self.ssgiPass.check_state(_state_dict(s, "ssgiPass", field), field + ".ssgiPass")
        _camera_from_state(s.get("finalCamera"), field + ".finalCamera")
        _state_int(s, "useEnvMap", field)

    def set_state(self, s):
        self.ssgiPass.set_state(s["ssgiPass"])
        self.denoiser.set_state(s["denoiser"])
        self.uniforms.camera = _camera_from_state(s["finalCamera"], "finalCamera")
        object.__setattr__(self, "_env_restored", bool(s["useEnvMap"]))

    def setSize(self, width, height, force=False):
        if width is None and height is None:
            return
        self.ssgiPass.setSize(width, height)
        self.denoiser.setSize(width, height)
        # K2 samples the pass's (possibly smaller) texture NEAREST at full-resolution vUv: the device needs its size
        tw, th = self.ssgiPass.renderTargetSize
        tu = self.denoiser.temporalReprojectPass.uniforms
        tu.inputWidth, tu.inputHeight = (0, 0) if (tw is None or self._options["resolutionScale"] == 1) else (int(tw), int(th))
        self.lastSize = dict(width=width, height=height, resolutionScale=self._options["resolutionScale"])

    @property
    def depthTexture(self):
        return self.ssgiPass.gBufferPass.depthTexture

    def initialize(self, renderer=None, *args):
        pass

    def dispose(self):
        self.ssgiPass.dispose()
        self.denoiser.dispose()

    def keepEnvMapUpdated(self, renderer):
        """:309-362.  `scene.environment`: None, or an equirectangular HDR map as dumped state — an object/dict with `data`
        ((H, W, 4) float32, row 0 = bottom) and optionally `type` (HalfFloatType, what RGBELoader yields and the default, or
        FloatType).  The effect turns its mipmaps on (:323-328): here the device builds the chain (rfx_set_environment)."""
        env = getattr(self._scene, "environment", None)
        u = self.ssgiPass.uniforms
        if env is not None:
            if self.__dict__.get("_env_uuid") is not env:
                get = (lambda k, d=None: env.get(k, d)) if isinstance(env, dict) else (lambda k, d=None: getattr(env, k, d))
                on_device = self._env_on_device and bool(getattr(renderer, "has_env_device", False))
                if get("isCubeTexture"):  # :316-321 convert it to an equirectangular texture so the pass can sample it and use MIS
                    if self.__dict__.get("cubeToEquirectEnvPass") is None:
                        object.__setattr__(self, "cubeToEquirectEnvPass", CubeToEquirectEnvPass())
                    converted = self.cubeToEquirectEnvPass.generateEquirectEnvMap(renderer, env, on_device=on_device)
                    get = lambda k, d=None: converted.get(k, d)  # noqa: E731
                t = get("type", HalfFloatType)
                data = None
                if get("data") is not None:  # (None: the cube pass has set the environment on the device)
                    data = np.ascontiguousarray(get("data"), np.float32)
                    renderer.set_environment(data, half_float_type=(t == HalfFloatType), half_store_rtz=self._half_store_rtz)
                u.importanceSampling = 0
                if self._options["importanceSampling"] and on_device:  # the same tables, built from the held level 0 (K10)
                    renderer.build_environment_importance(bool(get("flipY", False)))
                    u.importanceSampling = 1
                elif self._options["importanceSampling"]:  # :348-351 EquirectHdrInfoUniform.updateFrom, then the define
                    from .envmap import build_importance
                    texels = data.astype(np.float16).astype(np.float32) if t == HalfFloatType else data  # the worker's fromHalfFloat view
                    # `data` is in GL row order (row 0 = bottom, as sampled).  With texture.flipY the reference's DataTexture array is the
                    # other way up and the worker "un-flips" it (its own, lossy way): hand it what it would have seen
                    flip = bool(get("flipY", False))
                    renderer.set_environment_importance(*build_importance(texels[::-1] if flip else texels, flip))
                    u.importanceSampling = 1
                object.__setattr__(self, "_env_uuid", env)
                u.useEnvMap = 1  # defines.USE_ENVMAP :344
                if not self.__dict__.pop("_env_restored", False):  # (set_state: the map returns to a fresh device, the accumulation goes on)
                    self.reset()  # :356
        elif u.useEnvMap:  # :361-366
            u.useEnvMap = u.importanceSampling = 0
            renderer.set_environment(None)
            object.__setattr__(self, "_env_uuid", None)

    def update(self, renderer, inputBuffer=None):
        """:372-436.  `inputBuffer` = the composer's input buffer (direct lighting) as an (H,W,4)
        float32 array covering the frame, or None to take `scene.frame.direct`."""
        self.keepEnvMapUpdated(renderer)
        direct = inputBuffer if inputBuffer is not None else self._scene.frame.direct
        _upload_plane(renderer, abi.TEX_DIRECT_LIGHT, direct, getattr(self._scene.frame, "static", False))
        self.ssgiPass.render(renderer)
        self.denoiser.render(renderer, inputBuffer)
        # :400-417 the effect's own uniforms: inputTexture = the denoiser's texture, sceneTexture = the input buffer, fog from the scene
        u = self.uniforms
        out = self.denoiser.texture  # :139,402 inputTexture = outputTexture[0] ?? outputTexture
        out = out[0] if isinstance(out, (tuple, list)) else out
        u.inputSource = {abi.TEX_COMPOSE: 0, abi.TEX_TEMPORAL0: 1, abi.TEX_DENOISE_B0: 2}[out]
        fog = getattr(self._scene, "fog", None)
        u.fogMode = 0 if fog is None else (2 if getattr(fog, "isFogExp2", False) else 1)
        if fog is not None:
            u.fogColor[:] = [float(x) for x in fog.color]
            u.fogNear, u.fogFar = float(getattr(fog, "near", 0.0) or 0.0), float(getattr(fog, "far", 0.0) or 0.0)
            u.fogDensity = float(getattr(fog, "density", 0.0) or 0.0)
            u.camera = abi.Camera.from_scene(self._camera)

    def mainImage(self, renderer):
        """The effect's own fragment (src/ssgi/shader/ssgi_compose.frag:20-45), which postprocessing's EffectPass runs after
        update(): scene colour on background texels, composed GI (+ fog) elsewhere, alpha 1 -> RFX_TEX_FINAL."""
        renderer.final_compose(self.uniforms)
        return abi.TEX_FINAL


class SSREffect(SSGIEffect):
    """src/ssgi/SSREffect.js:3-9."""

    def __init__(self, composer, scene, camera, options=None, **kw):
        options = dict(options or {})
        options["mode"] = "ssr"
        super().__init__(composer, scene, camera, options, **kw)


class TRAAEffect:
    """src/traa/TRAAEffect.js:10-78.  K2 alone, on the composer's input buffer: one texture, inputType "diffuse",
    history = the pass's own framebuffer copy.  `inputBuffer` is the composer buffer as dumped state: an object (or
    dict) with `texture` (anything carrying three's `type`: HalfFloatType for `frameBufferType: HalfFloatType`,
    example/main.js:173, or FloatType), `width`, `height` and `data` — the H x W x 4 float32 scene colour, which
    stands where the reference's previous pass rendered into the buffer."""

    DefaultOptions = defaultTemporalReprojectPassOptions

    def __init__(self, scene, camera, velocityDepthNormalPass, options=None, half_store_rtz=True):
        self._scene, self._camera = scene, camera
        self.velocityDepthNormalPass = velocityDepthNormalPass
        o = dict(options or defaultTemporalReprojectPassOptions)
        o.update(maxBlend=0.9, neighborhoodClamp=True, neighborhoodClampIntensity=1, neighborhoodClampRadius=1, logTransform=True,
                 confidencePower=4)  # :21-31
        self.options = dict(defaultTemporalReprojectPassOptions, **o)
        self.temporalReprojectPass = None
        self._half_store_rtz = half_store_rtz
        self.uniforms = {"accumulatedTexture": None}
        self.unjitteredProjectionMatrix = None

    def reset(self):
        self.temporalReprojectPass.reset()

    def setSize(self, width, height):
        if self.temporalReprojectPass:
            self.temporalReprojectPass.setSize(width, height)

    def dispose(self):
        if self.temporalReprojectPass:
            self.temporalReprojectPass.dispose()

    @staticmethod
    def _field(obj, name):
        return obj[name] if isinstance(obj, dict) else getattr(obj, name)

    def temporal_params(self, texture=None):
        """The K2 launch parameters this effect draws with (textureCount 1, inputType DIFFUSE)."""
        if self.temporalReprojectPass is None:
            self.temporalReprojectPass = TemporalReprojectPass(self._scene, self._camera, self.velocityDepthNormalPass, texture, 1, self.options,
                                                               half_store_rtz=self._half_store_rtz)
        return self.temporalReprojectPass.uniforms

    def update(self, renderer, inputBuffer):
        if self.temporalReprojectPass is None:  # :53-66
            self.temporal_params(self._field(inputBuffer, "texture"))
            self.temporalReprojectPass.setSize(self._field(inputBuffer, "width"), self._field(inputBuffer, "height"))
            self.uniforms["accumulatedTexture"] = self.temporalReprojectPass.texture
        # the raster shims stand where the composer's earlier passes ran: velocity/depth/normal plane and the input buffer
        self.velocityDepthNormalPass.render(renderer)
        data = self._field(inputBuffer, "data")
        if self.temporalReprojectPass.targetType == HalfFloatType:
            # a HalfFloatType buffer holds half-precision texels: state that on the way in (exact for a real dump of one)
            cache = self.__dict__.setdefault("_half_cache", [None, None])
            if cache[0] is not data:
                cache[0], cache[1] = data, np.asarray(data, np.float32).astype(np.float16).astype(np.float32)
            data = cache[1]
        _upload_plane(renderer, abi.TEX_SSGI, data, bool(inputBuffer.get("static", False) if isinstance(inputBuffer, dict) else getattr(inputBuffer, "static", False)))  # K2's `inputTexture` (:118)
        self.temporalReprojectPass.unjitter()  # :68-73
        self.unjitteredProjectionMatrix = np.array(self._camera.projectionMatrix, np.float32).copy()
        self.temporalReprojectPass.jitter()
        self.temporalReprojectPass.render(renderer)  # :75

    # -- saved temporal state (rfx_amd.state).  The pass is built by the first update(), from the composer buffer's type: a state saved
    # after that builds it in a fresh effect (same type, same size); a state saved before it holds no pass.
    def state_slots(self):
        return self.temporalReprojectPass.state_slots() if self.temporalReprojectPass else []

    def state_slots_of(self, s):
        """the slots this effect keeps once set_state(s) has run"""
        t = s.get("temporalReprojectPass")
        if t is None:
            return []
        return [abi.TEX_TEMPORAL0, abi.TEX_FBCOPY_F16 if t.get("targetType") == HalfFloatType else abi.TEX_FBCOPY_F32]

    def get_state(self) -> dict:
        tp = self.temporalReprojectPass
        m = self.unjitteredProjectionMatrix
        return {"class": type(self).__name__,
                "temporalReprojectPass": dict(tp.get_state(), width=int(tp.width), height=int(tp.height)) if tp else None,
                "unjitteredProjectionMatrix": None if m is None else _hex64(np.asarray(m, np.float64).ravel())}

    def check_state(self, s, field="effect"):
        if s.get("class") != type(self).__name__:
            raise StateError(field + ".class", "saved %r, the running effect is %r" % (s.get("class"), type(self).__name__))
        t, f = s.get("temporalReprojectPass"), field + ".temporalReprojectPass"
        if t is not None:
            if not isinstance(t, dict) or t.get("targetType") not in (FloatType, HalfFloatType):
                raise StateError(f + ".targetType", "FloatType (%d) or HalfFloatType (%d) is expected" % (FloatType, HalfFloatType))
            tp = self.temporalReprojectPass or TemporalReprojectPass(self._scene, self._camera, self.velocityDepthNormalPass,
                                                                     dict(type=t["targetType"]), 1, self.options)
            tp.check_state(t, f)
            _state_int(t, "width", f)
            _state_int(t, "height", f)
        if s.get("unjitteredProjectionMatrix") is not None:
            _unhex(s["unjitteredProjectionMatrix"], "<f8", 16, field + ".unjitteredProjectionMatrix")

    def set_state(self, s):
        t = s["temporalReprojectPass"]
        if t is None:
            self.temporalReprojectPass = None
            self.uniforms["accumulatedTexture"] = None
        else:
            if self.temporalReprojectPass is None:  # :53-66, from the saved type instead of the first input buffer's
                self.temporal_params(dict(type=int(t["targetType"])))
                self.uniforms["accumulatedTexture"] = self.temporalReprojectPass.texture
            self.temporalReprojectPass.setSize(int(t["width"]), int(t["height"]))
            self.temporalReprojectPass.set_state(t)
        m = s.get("unjitteredProjectionMatrix")
        self.unjitteredProjectionMatrix = None if m is None else _unhex(m, "<f8", 16, "unjitteredProjectionMatrix").astype(np.float32).reshape(
            np.shape(self._camera.projectionMatrix))

    def output(self, renderer, row0=None, rows=None):
        """traa_compose.frag (src/traa/shader/traa_compose.frag:3-7): outputColor = vec4(accumulatedTexel.rgb, 1.)."""
        t = renderer.download(self.uniforms["accumulatedTexture"], row0, rows).copy()
        t[..., 3] = 1.0
        return t


# src/motion-blur/MotionBlurEffect.js:14
defaultMotionBlurOptions = dict(intensity=1, jitter=1, samples=16)


class MotionBlurEffect:
    """src/motion-blur/MotionBlurEffect.js:16-101 (K6, rfx_motion_blur).  `velocityPass` is the VelocityDepthNormalPass whose plane
    (RFX_TEX_VELOCITY) the effect reads.  `samples` is a define fixed at construction: the reactive setters forward only `intensity` and
    `jitter` (:42-45,51-66) — setting `samples` later is stored and never drawn with, as in the reference.

    update(renderer, inputBuffer, deltaTime): `inputBuffer` is a slot id (abi.TEX_FINAL after SSGIEffect.mainImage: the blur stays on the
    device; abi.TEX_TEMPORAL0 stands for the buffer TRAA's own EffectPass wrote, alpha 1) or a host buffer like TRAAEffect's (an array, or an object / dict with `data` and optionally `texture` carrying three's `type`),
    uploaded to RFX_TEX_EFFECT_INPUT.  `frame` (renderer.info.render.frame % 4096, :91) defaults to the number of updates so far modulo 4096
    and `resolution` (window.innerWidth / innerHeight, :94) to the frame size; both are settable.  shareEffectPass(traaEffect) draws the
    README form EffectPass(camera, traaEffect, motionBlurEffect): inputColor is TRAA's output (its NEAREST target, alpha 1) and the taps read
    the pass's input buffer, the plane TRAA drew from (RFX_TEX_SSGI)."""

    def __init__(self, velocityPass, options=None, half_store_rtz=True):
        o = dict(defaultMotionBlurOptions)
        o.update(options if options is not None else defaultMotionBlurOptions)
        self.velocityPass = velocityPass
        self._options = o
        self._half_store_rtz = half_store_rtz
        self.uniforms = abi.MotionBlurParams()
        u = self.uniforms
        u.source, u.center, u.centerAlphaOne = abi.TEX_FINAL, -1, 0
        u.samples = int(round(float(o["samples"])))  # options.samples.toFixed(0) (:37-40)
        u.intensity, u.jitter = 1.0, 1.0  # the uniforms' initial values (:31-32), then makeOptionsReactive sets both (:64)
        u.halfStoreRTZ = 1 if half_store_rtz else 0
        for key in o:  # makeOptionsReactive (:51-66): `this[key] = options[key]`
            setattr(self, key, o[key])
        self.frame = None
        self.resolution = None
        self._updates = 0
        self._traa = None

    def __setattr__(self, key, value):
        if key in ("intensity", "jitter", "samples") and "_options" in self.__dict__:
            self._options[key] = value
            if key in ("intensity", "jitter"):
                setattr(self.uniforms, key, float(value))
            return
        object.__setattr__(self, key, value)

    def __getattr__(self, key):
        if key in ("intensity", "jitter", "samples"):
            return self.__dict__["_options"][key]
        raise AttributeError(key)

    def shareEffectPass(self, traaEffect):
        """draw as the second effect of EffectPass(camera, traaEffect, motionBlurEffect) (readme.md:60-79); None: the effect's own pass"""
        self._traa = traaEffect

    def update(self, renderer, inputBuffer, deltaTime):
        u = self.uniforms
        u.deltaTime = max(1 / 1000, float(deltaTime))  # :89
        u.frame = int(self._updates if self.frame is None else self.frame) % 4096  # :91
        self._updates += 1
        res = (renderer.W, renderer.H) if self.resolution is None else self.resolution  # :94
        u.resolution[:] = [float(res[0]), float(res[1])]
        half = False
        if self._traa is not None:  # README form: TRAA's target is the centre, its input plane (RFX_TEX_SSGI) the taps' buffer
            tp = self._traa.temporalReprojectPass
            u.source, u.center, u.centerAlphaOne = abi.TEX_SSGI, self._traa.uniforms["accumulatedTexture"], 1
            half = tp is not None and tp.targetType == HalfFloatType
        elif isinstance(inputBuffer, (int, np.integer)):
            # abi.TEX_TEMPORAL0 stands for the buffer TRAA's own EffectPass wrote: traa_compose.frag:6 gave it alpha 1
            u.source, u.center, u.centerAlphaOne = int(inputBuffer), -1, int(int(inputBuffer) == abi.TEX_TEMPORAL0)
        else:
            data = inputBuffer
            tex = None
            if isinstance(inputBuffer, dict):
                data, tex = inputBuffer["data"], inputBuffer.get("texture")
            elif hasattr(inputBuffer, "data") and not isinstance(inputBuffer, np.ndarray):
                data, tex = inputBuffer.data, getattr(inputBuffer, "texture", None)
            half = tex is not None and _texture_type(tex) == HalfFloatType
            data = np.asarray(data, np.float32)
            if half:  # a HalfFloatType buffer holds half-precision texels
                data = data.astype(np.float16).astype(np.float32)
            renderer.upload(abi.TEX_EFFECT_INPUT, np.ascontiguousarray(data, np.float32))
            u.source, u.center, u.centerAlphaOne = abi.TEX_EFFECT_INPUT, -1, 0
        u.targetHalf = 1 if half else 0

    # -- saved temporal state (rfx_amd.state): the frame counter behind the jitter; K6 writes every texel, so the effect keeps no slot
    def state_slots(self):
        return []

    def get_state(self) -> dict:
        return {"class": type(self).__name__, "frame": None if self.frame is None else int(self.frame), "updates": int(self._updates)}

    def check_state(self, s, field="effect"):
        if s.get("class") != type(self).__name__:
            raise StateError(field + ".class", "saved %r, the running effect is %r" % (s.get("class"), type(self).__name__))
        _state_int(s, "frame", field, allow_none=True)
        _state_int(s, "updates", field)

    def set_state(self, s):
        self.frame = s["frame"]
        self._updates = int(s["updates"])

    def mainImage(self, renderer):
        """the effect's fragment (motion_blur.frag mainImage) -> RFX_TEX_MOTION_BLUR"""
        renderer.motion_blur(self.uniforms)
        return abi.TEX_MOTION_BLUR

    def output(self, renderer, row0=None, rows=None):
        return renderer.download(abi.TEX_MOTION_BLUR, row0, rows)

    def dispose(self):
        pass
