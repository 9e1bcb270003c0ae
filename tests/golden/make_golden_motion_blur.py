#!/usr/bin/env python3
"""Generate tests/golden/motion_blur_*.npz by running the REFERENCE's own MotionBlurEffect GLSL on CPU llvmpipe.

Build-container only, like make_golden.py: needs the reference's sources (chain.REFERENCE_SRC: src/motion-blur/shader/motion_blur.frag, the blue-noise chunk and
src/traa/shader/traa_compose.frag are read from there at run time and never copied into this repository) and Mesa's swrast_dri.so.

    make -C oracle && python tests/golden/make_golden_motion_blur.py

The fragment is wrapped the way postprocessing's EffectMaterial calls an Effect (an assumption: postprocessing is not vendored,
DESIGN.md "K6"): `inputColor = texture2D(inputBuffer, vUv)` (LINEAR) and `mainImage(inputColor, vUv, outputColor)`; in the README's
EffectPass(camera, traaEffect, motionBlurEffect) form the two effects' mainImage functions are renamed apart and chained, TRAA's first.
Fixtures (each < 1 MB; velocity keeps .xy only, the one part the effect reads):
  motion_blur_float_97x55.npz   FloatType buffers, default options, frames {0, 1, 4095} x deltaTime {1/60, 1/1000}
  motion_blur_cases_128x72.npz  samples {1, 7, 32}, intensity {0.5, -1, 3}, jitter {0, 2.5}, resolution != the frame size (outputs .rgb:
                                alpha is the input's)
  motion_blur_half_96x54.npz    HalfFloatType buffers (RGBA16F target, llvmpipe's truncating store): the effect's own EffectPass and the
                                README TRAA form
Every velocity plane holds zero, sub-threshold (dot < 1e-9), off-frame and NaN texels besides ordinary motion.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "realism-effects_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "glref"))

from rfx_amd.context import load_blue_noise_table  # noqa: E402  (the 128 x 128 table the library uploads)
import chain  # noqa: E402

F16 = np.float16


def assemble(samples, traa_form=False):
    """MotionBlurEffect.js:23-41 (setupBlueNoise + the samples / samplesFloat defines) inside the EffectMaterial wrapper."""
    mb = chain._with_blue_noise(chain._rd("motion-blur/shader/motion_blur.frag"))
    mb = mb.replace("void mainImage(", "void mainImage_motionBlur(")
    head = "varying vec2 vUv;\nuniform sampler2D inputBuffer;\n"
    if traa_form:
        traa = chain._rd("traa/shader/traa_compose.frag").replace("void mainImage(", "void mainImage_traa(")
        main = ("void main() { vec4 c0 = texture2D(inputBuffer, vUv); vec4 c1; mainImage_traa(c0, vUv, c1); vec4 c2; "
                "mainImage_motionBlur(c1, vUv, c2); gl_FragColor = c2; }\n")
        body = traa + "\n" + mb
    else:
        main = "void main() { vec4 c; mainImage_motionBlur(texture2D(inputBuffer, vUv), vUv, c); gl_FragColor = c; }\n"
        body = mb
    return chain.three_prefix({"samples": "%d" % samples, "samplesFloat": "%d.0" % samples}, False) + head + body + "\n" + main


def velocity_field(rng, W, H, scale=0.1):
    v = rng.uniform(-scale, scale, (H, W, 4)).astype(np.float32)
    kind = rng.integers(0, 20, (H, W))
    v[kind < 5, :2] = 0.0                                                       # static
    v[(kind >= 5) & (kind < 7), :2] = rng.uniform(-1.5e-5, 1.5e-5, (int(((kind >= 5) & (kind < 7)).sum()), 2))  # dot < 1e-9
    v[kind == 7, :2] = rng.uniform(-1.5, 1.5, (int((kind == 7).sum()), 2))      # streaks that leave the frame
    v[kind == 8, rng.integers(0, 2)] = np.nan                                   # NaN velocity: not moved
    v[20:23, 30:40, :2] = 0.6                                                   # a fast block
    return v


class Runner:
    def __init__(self, W, H, half=False):
        self.W, self.H, self.half = W, H, half
        self.fmt = chain.FMT_RGBA16F if half else chain.FMT_RGBA32F
        self.blue = chain.Tex(128, 128, chain.FMT_RGBA8, repeat=True, data=load_blue_noise_table())
        self.progs = {}

    def prog(self, samples, traa_form):
        k = (samples, traa_form)
        if k not in self.progs:
            self.progs[k] = chain.Program(assemble(samples, traa_form))
        return self.progs[k]

    def run(self, velocity, source, samples=16, intensity=1.0, jitter=1.0, deltaTime=1 / 60, frame=0, resolution=None, accumulated=None):
        W, H = self.W, self.H
        p = self.prog(samples, accumulated is not None)
        conv = (lambda a: np.ascontiguousarray(a, F16)) if self.half else (lambda a: np.ascontiguousarray(a, np.float32))
        t_vel = chain.Tex(W, H, chain.FMT_RGBA32F, data=np.ascontiguousarray(velocity, np.float32))  # VelocityDepthNormalPass: FloatType
        t_src = chain.Tex(W, H, self.fmt, linear=True, data=conv(source))  # the composer's input buffer
        t_out = chain.Tex(W, H, self.fmt)
        tex = [t_vel, t_src, t_out]
        p.sampler("inputBuffer", t_src)
        p.sampler("inputTexture", t_src)  # MotionBlurEffect.update :85 inputTexture = inputBuffer.texture
        p.sampler("velocityTexture", t_vel)
        p.sampler("blueNoiseTexture", self.blue)
        if accumulated is not None:
            t_acc = chain.Tex(W, H, self.fmt, data=conv(accumulated))  # TemporalReprojectPass.renderTarget: NearestFilter (:66-67)
            tex.append(t_acc)
            p.sampler("accumulatedTexture", t_acc)
        res = (W, H) if resolution is None else resolution
        p.set("resolution", [float(res[0]), float(res[1])])
        p.set("blueNoiseSize", [128.0, 128.0])
        p.set("intensity", float(intensity))
        p.set("jitter", float(jitter))
        p.set("deltaTime", float(max(1 / 1000, deltaTime)))  # :89
        p.set("frame", int(frame))
        p.draw([t_out])
        out = t_out.read()
        for t in tex:
            t.free()
        return out


def save(path, out):
    """np.savez_compressed with a fixed member timestamp: the same inputs give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asanyarray(out[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), a.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
    print("%s: %d bytes" % (os.path.basename(path), os.path.getsize(path)))


def make_float(path):
    W, H = 97, 55
    rng = np.random.default_rng(97055)
    vel, src = velocity_field(rng, W, H), rng.uniform(0, 3, (H, W, 4)).astype(np.float32)
    r = Runner(W, H)
    frames, dts = (0, 1, 4095), (1 / 60, 1 / 1000)
    outs = np.stack([np.stack([r.run(vel, src, frame=f, deltaTime=dt) for dt in dts]) for f in frames])
    save(path, dict(width=W, height=H, velocity=vel[..., :2], source=src, frames=np.array(frames), deltaTimes=np.array(dts, np.float32),
                    outputs=outs, samples=16, intensity=1.0, jitter=1.0, gl_info=chain.GL.info()))


CASES = (  # samples, intensity, jitter, resolution, frame, deltaTime
    (1, 0.5, 0.0, None, 3, 1 / 60),
    (7, -1.0, 2.5, (1920, 1080), 5, 1 / 60),
    (32, 3.0, 2.5, None, 0, 1 / 30),
    (7, 3.0, 0.0, (200, 50), 4095, 1 / 144),
    (32, 0.5, 2.5, (333, 77), 17, 1 / 60),
)


def make_cases(path):
    W, H = 128, 72
    rng = np.random.default_rng(128072)
    vel, src = velocity_field(rng, W, H), rng.uniform(0, 3, (H, W, 4)).astype(np.float32)
    r = Runner(W, H)
    outs = [r.run(vel, src, samples=s, intensity=i, jitter=j, resolution=res, frame=f, deltaTime=dt)[..., :3] for s, i, j, res, f, dt in CASES]
    cases = np.array([[s, i, j, (res or (W, H))[0], (res or (W, H))[1], f, max(1 / 1000, dt)] for s, i, j, res, f, dt in CASES], np.float64)
    save(path, dict(width=W, height=H, velocity=vel[..., :2], source=src, cases=cases, outputs_rgb=np.stack(outs), gl_info=chain.GL.info()))


def make_half(path):
    W, H = 96, 54
    rng = np.random.default_rng(96054)
    vel = velocity_field(rng, W, H)
    src = rng.uniform(0, 3, (H, W, 4)).astype(F16)  # HalfFloatType buffers hold half texels
    acc = rng.uniform(0, 3, (H, W, 4)).astype(F16)
    r = Runner(W, H, half=True)
    own = [r.run(vel, src, frame=1), r.run(vel, src, samples=7, intensity=2.0, frame=0, deltaTime=1 / 30)]
    traa = [r.run(vel, src, frame=1, accumulated=acc), r.run(vel, src, samples=7, intensity=2.0, frame=0, deltaTime=1 / 30, accumulated=acc)]
    cases = np.array([[16, 1.0, 1.0, W, H, 1, 1 / 60], [7, 2.0, 1.0, W, H, 0, 1 / 30]], np.float64)
    save(path, dict(width=W, height=H, velocity=vel[..., :2], source=src, accumulated=acc, cases=cases,
                    outputs_own=np.stack(own).astype(F16), outputs_traa=np.stack(traa).astype(F16), gl_info=chain.GL.info()))


if __name__ == "__main__":
    if not os.path.isdir(chain.REFERENCE_SRC):
        sys.exit("needs the reference's sources at %s" % chain.REFERENCE_SRC)
    make_float(os.path.join(HERE, "motion_blur_float_97x55.npz"))
    make_cases(os.path.join(HERE, "motion_blur_cases_128x72.npz"))
    make_half(os.path.join(HERE, "motion_blur_half_96x54.npz"))
