"""Test double for the checkpoint / resume tests (tests/test_state_cpu.py): an in-memory renderer, the same on both hosts.

It stores uploads, serves downloads and records every draw.  A draw's record is the SHA-256 of its parameters (every float as the hex
of its float32 bytes) and of the bytes of the slots it reads; its output slot is filled with bytes derived from that digest — except on
a fixed set of "background" texels, which keep the slot's previous contents, as K2 / K3 / K4 leave them on the device.  A counter or a
camera that a resume lost changes the parameters; a plane it lost changes an input or a kept texel: either shows up in the stream of
digests and in the final slot contents.  No arithmetic on texel values anywhere, so Python (numpy) and Node (typed arrays) agree byte
for byte.  MEM_RENDERER_JS is the Node twin."""
import hashlib
import json

import numpy as np

from rfx_amd import abi

T = abi


def h32(*values):
    return np.asarray(values, "<f4").tobytes().hex()


def cam_record(c):
    return [h32(*c.projectionMatrix), h32(*c.projectionMatrixInverse), h32(*c.matrixWorld), h32(*c.matrixWorldInverse), h32(*c.position),
            h32(c.near_), h32(c.far_), int(c.isPerspective)]


class MemRenderer:
    def __init__(self, W, H):
        self.W, self.H = W, H
        self.tex = {t: np.zeros((128 if t == T.TEX_BLUE_NOISE else H) * (128 if t == T.TEX_BLUE_NOISE else W) * np.dtype(d).itemsize * ch, np.uint8)
                    for t, (d, ch) in abi.TEX_FORMAT.items()}
        self.calls = []
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        self._drawn = ((x + y) % 3 != 0).reshape(-1)  # the other texels are "background": a draw that discards leaves them alone

    # -- the Context surface the hosts use
    def held_rows(self, tex):
        return (0, 128) if tex == T.TEX_BLUE_NOISE else (0, self.H)

    def _row_bytes(self, tex):
        d, ch = abi.TEX_FORMAT[tex]
        return (128 if tex == T.TEX_BLUE_NOISE else self.W) * np.dtype(d).itemsize * ch

    def upload(self, tex, array, row0=None, rows=None):
        h0, hn = self.held_rows(tex)
        row0, rows = (h0 if row0 is None else row0), (hn if rows is None else rows)
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        rb = self._row_bytes(tex)
        assert raw.size == rows * rb, (abi.TEX_NAMES[tex], raw.size, rows * rb)
        self.tex[tex][row0 * rb:(row0 + rows) * rb] = raw

    def download(self, tex, row0=None, rows=None):
        h0, hn = self.held_rows(tex)
        row0, rows = (h0 if row0 is None else row0), (hn if rows is None else rows)
        rb = self._row_bytes(tex)
        d, ch = abi.TEX_FORMAT[tex]
        a = self.tex[tex][row0 * rb:(row0 + rows) * rb].copy().view(d)
        return a.reshape((rows, -1, ch) if ch > 1 else (rows, -1))

    def sync(self):
        pass

    # -- draws
    def _draw(self, name, record, inputs, outputs, discards):
        h = hashlib.sha256(json.dumps(record, separators=(",", ":")).encode())
        for t in inputs:
            h.update(self.tex[t].tobytes())
        digest = h.digest()
        self.calls.append([name, digest.hex()])
        d = np.frombuffer(digest, np.uint8)
        for k, t in enumerate(outputs):
            tb = np.dtype(abi.TEX_FORMAT[t][0]).itemsize * abi.TEX_FORMAT[t][1]
            i = np.arange(self.W * self.H * tb)
            fill = (d[(i + k) % 32] ^ (i & 255)).astype(np.uint8)
            if discards:
                keep = ~np.repeat(self._drawn, tb)
                fill[keep] = self.tex[t][keep]
            self.tex[t] = fill

    def ssgi_march(self, p):
        hist = {0: [T.TEX_COMPOSE], 1: [T.TEX_TEMPORAL0], 2: [], 3: [T.TEX_COMPOSE_RGB]}[p.historySource]
        self._draw("ssgi", [cam_record(p.camera), p.steps, p.refineSteps, p.mode, p.useDirectLight, p.missedRays, p.importanceSampling, p.useEnvMap,
                            h32(p.rayDistance), h32(p.thickness), h32(p.envBlur), p.blueNoiseIndex, h32(p.resolutionScale), p.historySource],
                   hist, [T.TEX_SSGI], False)

    def temporal_reproject(self, p):
        hist = [T.TEX_DENOISE_B0, T.TEX_DENOISE_B1][:p.textureCount] if p.historySource == 0 else [T.TEX_FBCOPY_F16 if p.historySource == 1 else T.TEX_FBCOPY_F32]
        self._draw("temporal", [cam_record(p.camera), cam_record(p.prevCamera), p.textureCount, p.inputType, list(p.reprojectSpecular), list(p.neighborhoodClamp),
                                p.logTransform, p.fullAccumulate, h32(p.confidencePower), h32(p.neighborhoodClampIntensity), h32(p.maxBlend), h32(p.keepData),
                                p.historySource, p.targetHalf, p.halfStoreRTZ, p.inputWidth, p.inputHeight],
                   [T.TEX_SSGI] + hist, [T.TEX_TEMPORAL0, T.TEX_TEMPORAL1][:p.textureCount], True)

    def copy_framebuffer(self, dst):
        self.calls.append(["copy", dst])
        src = self.tex[T.TEX_TEMPORAL0]
        self.tex[dst] = src.copy() if dst == T.TEX_FBCOPY_F32 else src.view(np.uint32).astype(np.uint16).view(np.uint8).copy()  # (the low halves: bytes only)

    def poisson_denoise(self, p):
        n = p.textureCount
        src = [T.TEX_TEMPORAL0, T.TEX_TEMPORAL1] if p.inputIsTemporal else ([T.TEX_DENOISE_A0, T.TEX_DENOISE_A1] if p.writeToB else [T.TEX_DENOISE_B0, T.TEX_DENOISE_B1])
        dst = [T.TEX_DENOISE_B0, T.TEX_DENOISE_B1] if p.writeToB else [T.TEX_DENOISE_A0, T.TEX_DENOISE_A1]
        self._draw("denoise", [h32(p.radius), h32(p.phi), h32(p.lumaPhi), h32(p.depthPhi), h32(p.normalPhi), h32(p.roughnessPhi), h32(p.specularPhi), n,
                               list(p.isTextureSpecular), p.blueNoiseIndex, p.inputIsTemporal, p.writeToB, p.halfStoreRTZ], src[:n], dst[:n], True)

    def compose(self, p):
        src = [T.TEX_TEMPORAL0, T.TEX_TEMPORAL1] if p.giSource else [T.TEX_DENOISE_B0, T.TEX_DENOISE_B1]
        self._draw("compose", [cam_record(p.camera), p.inputType, p.giSource, p.writeHistoryRGB], src, [T.TEX_COMPOSE], True)
        if p.writeHistoryRGB:
            self.tex[T.TEX_COMPOSE_RGB] = self.tex[T.TEX_COMPOSE].reshape(-1, 16)[:, :12].reshape(-1).copy()

    def final_compose(self, p):
        src = (T.TEX_COMPOSE, T.TEX_TEMPORAL0, T.TEX_DENOISE_B0)[p.inputSource]
        self._draw("final", [cam_record(p.camera), p.isDebug, p.inputSource, p.fogMode], [src], [T.TEX_FINAL], False)

    def motion_blur(self, p):
        self._draw("motion_blur", [p.source, p.center, p.centerAlphaOne, p.samples, h32(p.intensity), h32(p.jitter), h32(p.deltaTime), p.frame,
                                   h32(*p.resolution), p.targetHalf, p.halfStoreRTZ], [p.source] + ([p.center] if p.center >= 0 else []), [T.TEX_MOTION_BLUR], False)

    def slot_digests(self):
        return {abi.TEX_NAMES[t]: hashlib.sha256(self.tex[t].tobytes()).hexdigest() for t in sorted(self.tex) if t != T.TEX_BLUE_NOISE}


# The same renderer for the Node host (required by the drivers of tests/test_state_cpu.py: `eval`-ed after `fx`, `TEX`, `FORMAT` exist).
MEM_RENDERER_JS = r"""
const crypto = require("crypto")
const h32 = (...v) => { const a = Float32Array.from(v); return Buffer.from(a.buffer).toString("hex") }
const camRecord = c => [h32(...c.projectionMatrix), h32(...c.projectionMatrixInverse), h32(...c.matrixWorld), h32(...c.matrixWorldInverse), h32(...c.position),
  h32(c.near), h32(c.far), c.isPerspectiveCamera === undefined || c.isPerspectiveCamera ? 1 : 0]
const TEX_NAMES = []
for (const k of Object.keys(TEX)) TEX_NAMES[TEX[k]] = k.toLowerCase()
class MemRenderer {
  constructor(W, H) {
    this.width = W; this.height = H; this.calls = []; this.tex = {}
    for (const t of Object.keys(FORMAT)) {
      const n = +t === TEX.BLUE_NOISE ? 128 * 128 : W * H
      this.tex[t] = new Uint8Array(n * FORMAT[t][0].BYTES_PER_ELEMENT * FORMAT[t][1])
    }
    this.drawn = new Uint8Array(W * H)
    for (let y = 0; y < H; y++) for (let x = 0; x < W; x++) this.drawn[y * W + x] = (x + y) % 3 !== 0 ? 1 : 0
  }
  heldRows(tex) { return tex === TEX.BLUE_NOISE ? [0, 128] : [0, this.height] }
  rowBytes(tex) { return (tex === TEX.BLUE_NOISE ? 128 : this.width) * FORMAT[tex][0].BYTES_PER_ELEMENT * FORMAT[tex][1] }
  upload(tex, array, row0, rows) {
    const held = this.heldRows(tex)
    if (row0 === undefined) row0 = held[0]
    if (rows === undefined) rows = held[1]
    const raw = new Uint8Array(array.buffer, array.byteOffset, array.byteLength)
    if (raw.length !== rows * this.rowBytes(tex)) throw new Error("upload " + TEX_NAMES[tex] + ": " + raw.length + " bytes for " + rows + " rows")
    this.tex[tex].set(raw, row0 * this.rowBytes(tex))
  }
  uploadPlane(tex, plane) { this.upload(tex, plane, 0, this.height) }
  download(tex, row0, rows) {
    const held = this.heldRows(tex)
    if (row0 === undefined) row0 = held[0]
    if (rows === undefined) rows = held[1]
    const rb = this.rowBytes(tex)
    const copy = this.tex[tex].slice(row0 * rb, (row0 + rows) * rb)
    return new FORMAT[tex][0](copy.buffer)
  }
  sync() {}
  draw(name, record, inputs, outputs, discards) {
    const h = crypto.createHash("sha256").update(JSON.stringify(record))
    for (const t of inputs) h.update(this.tex[t])
    const d = h.digest()
    this.calls.push([name, d.toString("hex")])
    outputs.forEach((t, k) => {
      const tb = FORMAT[t][0].BYTES_PER_ELEMENT * FORMAT[t][1]
      const out = this.tex[t]
      for (let i = 0; i < out.length; i++) if (!discards || this.drawn[Math.floor(i / tb)]) out[i] = d[(i + k) % 32] ^ (i & 255)
    })
  }
  ssgiMarch(p) {
    const hist = { 0: [TEX.COMPOSE], 1: [TEX.TEMPORAL0], 2: [], 3: [TEX.COMPOSE_RGB] }[p.historySource]
    this.draw("ssgi", [camRecord(p.camera), p.steps, p.refineSteps, p.mode, p.useDirectLight, p.missedRays, p.importanceSampling, p.useEnvMap,
      h32(p.rayDistance), h32(p.thickness), h32(p.envBlur), p.blueNoiseIndex, h32(p.resolutionScale), p.historySource], hist, [TEX.SSGI], false)
  }
  temporalReproject(p) {
    const hist = p.historySource === 0 ? [TEX.DENOISE_B0, TEX.DENOISE_B1].slice(0, p.textureCount) : [p.historySource === 1 ? TEX.FBCOPY_F16 : TEX.FBCOPY_F32]
    this.draw("temporal", [camRecord(p.camera), camRecord(p.prevCamera), p.textureCount, p.inputType, p.reprojectSpecular, p.neighborhoodClamp,
      p.logTransform, p.fullAccumulate, h32(p.confidencePower), h32(p.neighborhoodClampIntensity), h32(p.maxBlend), h32(p.keepData),
      p.historySource, p.targetHalf, p.halfStoreRTZ, p.inputWidth, p.inputHeight], [TEX.SSGI].concat(hist), [TEX.TEMPORAL0, TEX.TEMPORAL1].slice(0, p.textureCount), true)
  }
  copyFramebuffer(dst) {
    this.calls.push(["copy", dst])
    const src = this.tex[TEX.TEMPORAL0]
    if (dst === TEX.FBCOPY_F32) this.tex[dst] = src.slice()
    else {
      const u = new Uint32Array(src.buffer, src.byteOffset, src.length / 4)
      this.tex[dst] = new Uint8Array(Uint16Array.from(u, v => v & 0xffff).buffer)
    }
  }
  poissonDenoise(p) {
    const n = p.textureCount
    const src = p.inputIsTemporal ? [TEX.TEMPORAL0, TEX.TEMPORAL1] : p.writeToB ? [TEX.DENOISE_A0, TEX.DENOISE_A1] : [TEX.DENOISE_B0, TEX.DENOISE_B1]
    const dst = p.writeToB ? [TEX.DENOISE_B0, TEX.DENOISE_B1] : [TEX.DENOISE_A0, TEX.DENOISE_A1]
    this.draw("denoise", [h32(p.radius), h32(p.phi), h32(p.lumaPhi), h32(p.depthPhi), h32(p.normalPhi), h32(p.roughnessPhi), h32(p.specularPhi), n,
      p.isTextureSpecular, p.blueNoiseIndex, p.inputIsTemporal, p.writeToB, p.halfStoreRTZ], src.slice(0, n), dst.slice(0, n), true)
  }
  compose(p) {
    const src = p.giSource ? [TEX.TEMPORAL0, TEX.TEMPORAL1] : [TEX.DENOISE_B0, TEX.DENOISE_B1]
    this.draw("compose", [camRecord(p.camera), p.inputType, p.giSource, p.writeHistoryRGB], src, [TEX.COMPOSE], true)
    if (p.writeHistoryRGB) {
      const c = this.tex[TEX.COMPOSE], r = this.tex[TEX.COMPOSE_RGB]
      for (let i = 0, j = 0; i < c.length; i += 16, j += 12) r.set(c.subarray(i, i + 12), j)
    }
  }
  finalCompose(p) {
    this.draw("final", [camRecord(p.camera), p.isDebug, p.inputSource, p.fogMode], [[TEX.COMPOSE, TEX.TEMPORAL0, TEX.DENOISE_B0][p.inputSource]], [TEX.FINAL], false)
  }
  motionBlur(p) {
    this.draw("motion_blur", [p.source, p.center, p.centerAlphaOne, p.samples, h32(p.intensity), h32(p.jitter), h32(p.deltaTime), p.frame,
      h32(...p.resolution), p.targetHalf, p.halfStoreRTZ], [p.source].concat(p.center >= 0 ? [p.center] : []), [TEX.MOTION_BLUR], false)
  }
  slotDigests() {
    const out = {}
    for (const t of Object.keys(this.tex)) if (+t !== TEX.BLUE_NOISE) out[TEX_NAMES[t]] = crypto.createHash("sha256").update(this.tex[t]).digest("hex")
    return out
  }
}
"""
