"use strict"
// Dump directory reader: frame.json + raw little-endian planes (row 0 = bottom).
//   frame.json : { width, height, camera: {...16-number matrices..., position, quaternion, near, far}, prevCamera: {...} }
//   depth.bin    Float32 W*H        gbuffer.bin  Uint32 W*H*4 (bit patterns of the RGBA32F texels)
//   velocity.bin Uint32 W*H*4       direct.bin   Float32 W*H*4
// or, instead of gbuffer.bin / velocity.bin, UNPACKED attribute planes the device packs (rfx_pack_gbuffer / rfx_pack_velocity):
//   aov_diffuse.bin F32 W*H*4  aov_normal.bin F32 W*H*3 (world)  aov_roughness.bin / aov_metalness.bin F32 W*H  aov_emissive.bin F32 W*H*3
//   aov_velocity.bin F32 W*H*2 (uv units)
// A plane whose values are halves may be stored as IEEE binary16 — aov_<name>.f16.bin / direct.f16.bin instead of the .bin — and is read as a
// Uint16Array of half bits: the typed frame Renderer.stageAov sends at two bytes per element (widenHalf gives the Float32Array the
// synchronous loaders take).  diffuse and direct may have three channels (alpha 1): the count follows from the file size.
// An ENGINE-FORM dump (include/rfx.h "AOV conventions") carries the planes as a renderer writes them: aov_position(.f16).bin (world x, y, z:
// W*H*3) or aov_view_z(.f16).bin (positive camera-axis distance: W*H) in place of depth.bin, aov_normal in camera space, aov_velocity in the
// engine's units or absent (velocity_kind "cameras"), and frame.json's "aovConventions": the record rfx_amd.conventions.AovConventions.to_json
// writes (kinds, velocity_scale, background_position; the matrices when present, else derived from the frame's cameras).  frame.depth is then
// that plane, frame.aovConventions the record; such a frame is staged (Renderer.stageFrame: --stream true), the device converts.
const fs = require("fs")
const path = require("path")

function plane(file, Ctor) {
	const b = fs.readFileSync(file)
	const ab = b.buffer.slice(b.byteOffset, b.byteOffset + b.length) // own, aligned ArrayBuffer
	return new Ctor(ab)
}

// aov_<name>.f16.bin (Uint16Array) or .bin (Float32Array), whichever exists; `channels`: the counts the plane may have
function typedPlane(dir, stem, n, channels) {
	const f16 = path.join(dir, stem + ".f16.bin")
	const half = fs.existsSync(f16)
	const a = plane(half ? f16 : path.join(dir, stem + ".bin"), half ? Uint16Array : Float32Array)
	if (!channels.some(c => a.length === c * n)) throw new Error("dump " + dir + ": " + stem + " does not match frame.json")
	return a
}

// IEEE binary16 bits -> Float32Array (exact)
function widenHalf(h) {
	if (!(h instanceof Uint16Array)) return h
	const out = new Float32Array(h.length)
	const bits = new Uint32Array(out.buffer)
	for (let i = 0; i < h.length; i++) {
		const v = h[i]
		const s = (v & 0x8000) << 16
		let e = (v >> 10) & 31
		let m = v & 0x3ff
		if (e === 31) bits[i] = s | 0x7f800000 | (m << 13)
		else if (e !== 0) bits[i] = s | ((e + 112) << 23) | (m << 13)
		else if (m === 0) bits[i] = s
		else {
			e = 113
			while (!(m & 0x400)) {
				m <<= 1
				e--
			}
			bits[i] = s | (e << 23) | ((m & 0x3ff) << 13)
		}
	}
	return out
}

// a plane of a typed frame as the synchronous entry points take it: a Float32Array of `channels` per texel (halves widened, an rgb plane given
// alpha 1); the plane itself when it is that already.  The result is remembered per plane object, so a resident plane stays the same object.
const widened = new WeakMap()
function floatPlane(p, texels, channels) {
	if (!(p instanceof Uint16Array) && !(p instanceof Float32Array && channels === 4 && p.length === 3 * texels)) return p
	let out = widened.get(p)
	if (out) return out
	out = widenHalf(p)
	if (channels === 4 && out.length === 3 * texels) {
		const rgba = new Float32Array(4 * texels)
		for (let i = 0; i < texels; i++) {
			rgba[4 * i] = out[3 * i]
			rgba[4 * i + 1] = out[3 * i + 1]
			rgba[4 * i + 2] = out[3 * i + 2]
			rgba[4 * i + 3] = 1
		}
		out = rgba
	}
	widened.set(p, out)
	return out
}

function readDump(dir) {
	const meta = JSON.parse(fs.readFileSync(path.join(dir, "frame.json"), "utf8"))
	const n = meta.width * meta.height
	const frame = {
		width: meta.width,
		height: meta.height,
		camera: meta.camera,
		prevCamera: meta.prevCamera,
		depth: null,
		aovConventions: meta.aovConventions || null,
		direct: typedPlane(dir, "direct", n, [3, 4]),
		gbuffer: null,
		velocity: null,
		aov: null
	}
	const has = stem => fs.existsSync(path.join(dir, stem + ".bin")) || fs.existsSync(path.join(dir, stem + ".f16.bin"))
	let depthChannels = 1
	if (has("aov_position")) {
		frame.depth = typedPlane(dir, "aov_position", n, [3])
		depthChannels = 3
	} else if (has("aov_view_z")) frame.depth = typedPlane(dir, "aov_view_z", n, [1])
	else frame.depth = plane(path.join(dir, "depth.bin"), Float32Array)
	if (fs.existsSync(path.join(dir, "gbuffer.bin"))) {
		frame.gbuffer = plane(path.join(dir, "gbuffer.bin"), Uint32Array)
		frame.velocity = plane(path.join(dir, "velocity.bin"), Uint32Array)
		if (frame.gbuffer.length !== 4 * n || frame.velocity.length !== 4 * n) throw new Error("dump " + dir + ": plane sizes do not match frame.json")
	} else {
		frame.aov = {}
		for (const kc of [["diffuse", 4], ["normal", 3], ["roughness", 1], ["metalness", 1], ["emissive", 3], ["velocity", 2]]) {
			if (kc[0] === "velocity" && !has("aov_velocity")) continue // (velocity_kind "cameras": no motion plane)
			frame.aov[kc[0]] = typedPlane(dir, "aov_" + kc[0], n, kc[0] === "diffuse" ? [3, 4] : [kc[1]])
		}
	}
	if (frame.depth.length !== depthChannels * n) throw new Error("dump " + dir + ": plane sizes do not match frame.json")
	return frame
}

module.exports = { readDump, widenHalf, floatPlane }
