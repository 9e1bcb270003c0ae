"use strict"
// Renderer — the device.  Stands where three's WebGLRenderer stands in the reference's
// `pass.render(renderer)` calls: one Renderer = one rfx context (librfx_hip.so) on one GPU, or on one
// row tile of the frame (tileY0 / tileRows / haloRows).  Thin wrapper over the N-API addon
// (../napi/rfx_napi.node); there is NO software fallback: loading fails if the addon or the HIP
// library is missing, and creation fails without an MI355X.
const fs = require("fs")
const path = require("path")
const addon = require("../napi/rfx_napi.node")

// texture slots — include/rfx.h `rfx_tex`
const TEX = {
	DEPTH: 0,
	GBUFFER: 1,
	VELOCITY: 2,
	DIRECT_LIGHT: 3,
	BLUE_NOISE: 4,
	SSGI: 5,
	TEMPORAL0: 6,
	TEMPORAL1: 7,
	DENOISE_A0: 8,
	DENOISE_A1: 9,
	DENOISE_B0: 10,
	DENOISE_B1: 11,
	COMPOSE: 12,
	FBCOPY_F16: 13,
	FBCOPY_F32: 14,
	FINAL: 15,
	COMPOSE_RGB: 16,
	EFFECT_INPUT: 17,
	MOTION_BLUR: 18,
	BLUR_SOURCE: 19
}
// [TypedArray constructor, elements per texel]
const FORMAT = {
	0: [Float32Array, 1],
	1: [Uint32Array, 4],
	2: [Uint32Array, 4],
	3: [Float32Array, 4],
	4: [Uint8Array, 4],
	5: [Uint32Array, 4],
	6: [Float32Array, 4],
	7: [Float32Array, 4],
	8: [Uint16Array, 4],
	9: [Uint16Array, 4],
	10: [Uint16Array, 4],
	11: [Uint16Array, 4],
	12: [Float32Array, 4],
	13: [Uint16Array, 4],
	14: [Float32Array, 4],
	15: [Float32Array, 4],
	16: [Float32Array, 3],
	17: [Float32Array, 4],
	18: [Float32Array, 4],
	19: [Float32Array, 4]
}

// rfx_export_params.format (include/rfx.h RFX_EXPORT_*): [value, TypedArray constructor of the exported elements]
const EXPORT = { F32: 0, F16: 1, U8_SRGB: 2 }
const EXPORT_ARRAY = { 0: Float32Array, 1: Uint16Array, 2: Uint8Array }
const EXPORT_TONEMAP = { linear: 0, aces: 1 }
// rfx_profile_read's kinds (include/rfx.h RFX_PROF_*), the index of profileRead()'s arrays
const PROF_KINDS = ["k1_prepass", "k1_ssgi_march", "k2_temporal_reproject", "k3_poisson_denoise_pass0", "k3_poisson_denoise_passN", "k4_compose", "k5_final_compose",
	"k6_motion_blur", "k6_motion_blur_reach", "k7_export"]
// ... and the kinds behind RFX_PROF_COUNT (rfx_profile_read_n): profileRead()'s arrays have PROF_KINDS_ALL.length entries
const PROF_KINDS_ALL = PROF_KINDS.concat(["k8_png"])
// rfx_stage_png's `filter` (include/rfx.h "PNG fragments")
const PNG_FILTERS = { adaptive: 0, none: 1, sub: 2, up: 3, paeth: 4 }
// RFX_ENCODE_MATCHES (include/rfx.h "Match form"): the flags bit of rfx_png_ex / rfx_stage_png_ex / rfx_exr_ex / rfx_stage_exr_ex
const ENCODE_MATCHES = 1
// the addon's functions per encode kind: [the byte count of a result buffer, the blocking call, the staged call]; the match forms: + "Ex"
const ENCODE = { export: ["exportBytes", "exportFrame", "stageExport"], png: ["pngBound", "pngFrame", "stagePng"], exr: ["exrBound", "exrFrame", "stageExr"] }
// ... and per form of an EXR frame's records (layout.chunks, layout.blocks, "piz": blocks with a PIZ part): [the byte count, the staging call]
const EXR_FRAME = { chunks: ["exrAovStageBytes", "stageExrAov"], blocks: ["exrBlocksStageBytes", "stageExrBlocks"], piz: ["exrBlocksPizStageBytes", "stageExrBlocksPiz"] }

// 128x128 RGBA8 blue-noise table: decoded once from the reference's PNG asset, already flipY'd
// (tools/make_blue_noise_table.py; src/utils/BlueNoiseUtils.js:9-15)
function loadBlueNoiseTable() {
	const buf = fs.readFileSync(path.join(__dirname, "..", "data", "blue_noise_128_rgba8.bin"))
	if (buf.length !== 128 * 128 * 4) throw new Error("blue noise table: unexpected size")
	return new Uint8Array(buf.buffer, buf.byteOffset, buf.length)
}

class Renderer {
	constructor(width, height, options) {
		options = options || {}
		this.width = width
		this.height = height
		this.tileY0 = options.tileY0 || 0
		this.tileRows = options.tileRows === undefined ? height - this.tileY0 : options.tileRows
		this.haloRows = options.haloRows || 0
		this._h = addon.create(options.device || 0, width, height, this.tileY0, this.tileRows, this.haloRows)
		this._resident = {}
		this.upload(TEX.BLUE_NOISE, loadBlueNoiseTable(), 0, 128)
	}

	heldRows(tex) {
		return addon.heldRows(this._h, tex)
	}

	// [row0, rows] of the K1 target TEX.SSGI holds after a draw at `resolutionScale` (rfx_ssgi_target_rows): the whole (W*s) x (H*s) target
	// on a whole-frame context, the rows K2's staging of the tile addresses on a row tile; stored from the start of the slot, pitch W*s
	ssgiTargetRows(resolutionScale) {
		return addon.ssgiTargetRows(this._h, resolutionScale === undefined ? 1 : resolutionScale)
	}

	// rows [row0, row0+rows) in FRAME rows; `array` holds exactly those rows
	upload(tex, array, row0, rows) {
		addon.upload(this._h, tex, array, ...this._heldBand(tex, row0, rows))
	}
	// the band of an upload, a download or a pack call: by default the rows the slot holds
	_heldBand(tex, row0, rows) {
		const held = this.heldRows(tex)
		return [row0 === undefined ? held[0] : row0, rows === undefined ? held[1] : rows]
	}
	// a FULL-FRAME plane -> [the rows of it the slot holds (a plane of just those rows: as it is), row0, rows]
	_heldPart(tex, plane) {
		const held = this.heldRows(tex)
		const per = FORMAT[tex][1] * this.width
		return [plane.length === held[1] * per ? plane : plane.subarray(held[0] * per, (held[0] + held[1]) * per), held[0], held[1]]
	}

	// a dumped FULL-FRAME plane: the slot takes the band it holds.  Every call uploads (the reference re-renders its raster passes every
	// frame) unless the dump declares itself unchanged (frame.static): then an already resident plane object is not re-sent — opt-in,
	// because a buffer refilled in place is the same object with new texels
	uploadPlane(tex, plane, isStatic) {
		if (isStatic === "resident" || (isStatic && this._resident[tex] === plane)) return
		this.upload(tex, ...this._heldPart(tex, plane))
		this._resident[tex] = plane
	}

	// streaming dumps (rfx.h): stage the NEXT frame's planes asynchronously (pinned memory from Renderer.hostAlloc), then stageFlip()
	// after the current frame's draws; a frame streamed this way carries `static: "resident"` so the loader shims do not upload it again
	static hostAlloc(Ctor, length) {
		return new Ctor(addon.hostAlloc(length * Ctor.BYTES_PER_ELEMENT))
	}
	// the band of a staging call: FRAME rows [row0, row0 + rows), by default from row0 (0) to the top of the frame
	_band(row0, rows) {
		return [row0 === undefined ? 0 : row0, rows === undefined ? this.height - (row0 || 0) : rows]
	}
	// streamed AOV frames (rfx.h): the attribute planes of FRAME rows [row0, row0 + rows) (default: the whole frame) — Float32Array, or Uint16Array
	// of IEEE half bits — are staged once and packed on the upload stream into the back buffers of DEPTH and of the slots the planes name
	// { diffuse, normal, roughness, metalness, emissive, velocity, depth, direct }; stageFlip() publishes them
	stageAov(planes, row0, rows) {
		addon.stageAov(this._h, planes, ...this._band(row0, rows))
		this._stagedAov = planes // keep the planes alive while they are in flight
	}
	// AOV conventions (rfx.h): what the next stageAov / stageExrAov / stageExrBlocks calls take their depth, velocity and normal planes for —
	// { depth_kind: "fragcoord" | "view_z" | "position", velocity_kind: "uv" | "scaled" | "cameras", normal_space: "world" | "view", perspective,
	// velocity_scale: [sx, sy], near, far, velocityMatrix, prevVelocityMatrix, projectionMatrix, projectionMatrixInverse, cameraMatrixWorld (16
	// column-major floats each), background_position: [x, y, z] | null }: the record rfx_amd.conventions.AovConventions.to_json writes.
	// null / undefined: the default.  Set per frame: the matrices change.  Under "position" / "view_z" the depth plane holds that.
	get hasAovConventions() {
		return typeof addon.setAovConventions === "function"
	}
	static velocityMatrix(projectionMatrix, matrixWorldInverse) {
		// three's Matrix4.multiplyMatrices on the float32 elements, every sum in float64 left to right, rounded once: what the reference uploads
		// for an identity model matrix (the Python host forms the same 16 floats: conventions.multiply_matrices)
		const a = projectionMatrix, b = matrixWorldInverse, out = new Float32Array(16)
		for (let j = 0; j < 4; j++) {
			for (let i = 0; i < 4; i++) {
				let s = a[i] * b[4 * j]
				s = s + a[4 + i] * b[4 * j + 1]
				s = s + a[8 + i] * b[4 * j + 2]
				s = s + a[12 + i] * b[4 * j + 3]
				out[4 * j + i] = s
			}
		}
		return out
	}
	// a record without matrices (a dump directory's, a command line's) completed from the frame's cameras
	static conventionsFor(record, camera, prevCamera) {
		const prev = prevCamera || camera
		return Object.assign({
			perspective: camera.isPerspectiveCamera !== false, near: camera.near, far: camera.far,
			velocityMatrix: Renderer.velocityMatrix(Float32Array.from(camera.projectionMatrix), Float32Array.from(camera.matrixWorldInverse)),
			prevVelocityMatrix: Renderer.velocityMatrix(Float32Array.from(prev.projectionMatrix), Float32Array.from(prev.matrixWorldInverse)),
			projectionMatrix: camera.projectionMatrix, projectionMatrixInverse: camera.projectionMatrixInverse, cameraMatrixWorld: camera.matrixWorld
		}, record)
	}
	setAovConventions(conv) {
		if (!this.hasAovConventions) throw new Error("this addon has no setAovConventions")
		this._conventionsSet = !(conv === null || conv === undefined)
		if (conv === null || conv === undefined) return addon.setAovConventions(this._h, null, null)
		const pick = (table, v, what) => {
			if (!(v in table)) throw new RangeError("AOV conventions: " + what + " " + Object.keys(table).join(" | "))
			return table[v]
		}
		const bg = conv.background_position
		const kinds = Int32Array.of(
			pick({ fragcoord: 0, view_z: 1, position: 2 }, conv.depth_kind === undefined ? "fragcoord" : conv.depth_kind, "depth_kind"),
			pick({ uv: 0, scaled: 1, cameras: 2 }, conv.velocity_kind === undefined ? "uv" : conv.velocity_kind, "velocity_kind"),
			pick({ world: 0, view: 1 }, conv.normal_space === undefined ? "world" : conv.normal_space, "normal_space"),
			conv.perspective === false ? 0 : 1, bg ? 1 : 0)
		const f = new Float32Array(87)
		const scale = conv.velocity_scale || [1, 1]
		f[0] = scale[0]; f[1] = scale[1]; f[2] = conv.near || 0; f[3] = conv.far || 0
		const names = ["velocityMatrix", "prevVelocityMatrix", "projectionMatrix", "projectionMatrixInverse", "cameraMatrixWorld"]
		names.forEach((n, k) => {
			const m = conv[n] || [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
			if (m.length !== 16) throw new RangeError("AOV conventions: " + n + " has 16 elements")
			f.set(m, 4 + 16 * k)
		})
		if (bg) f.set(bg, 84)
		addon.setAovConventions(this._h, kinds, f)
	}
	aovStageBytes(planes, row0, rows) {
		return addon.aovStageBytes(this._h, planes, ...this._band(row0, rows))
	}
	// streamed EXR frames (rfx.h): stageAov for a frame that is still an OpenEXR file — `bytes` the file (a Uint8Array / Buffer; over hostAlloc
	// memory the copies are asynchronous), `layout` = imageio.exrAovLayout(bytes): the chunks of the band cross PCIe packed and are decoded on
	// the device.  exrAovStatus() waits for that decode -> [bad chunks, index of the first bad chunk or -1, its error code or 0]
	stageExrAov(bytes, layout, row0, rows) {
		this._exrFrame(1, "chunks", bytes, layout, row0, rows)
	}
	exrAovStageBytes(bytes, layout, row0, rows) {
		return this._exrFrame(0, "chunks", bytes, layout, row0, rows)
	}
	exrAovStatus() {
		return addon.exrAovStatus(this._h)
	}
	// EXR blocks (rfx.h): the same for tiled parts, RLE and PXR24, a moved data window — `layout` = imageio.exrAovLayout(bytes, names, { forms:
	// "blocks" }), whose `blocks` are rectangles of the frame (a scanline chunk or a tile each).  exrAovStatus() reports on either call.
	// A layout with a PIZ part (exrAovLayout(..., { forms: "blocks", piz: true }); rfx.h "EXR blocks with PIZ") goes through rfx_stage_exr_blocks_piz.
	static _layoutHasPiz(layout) {
		const w = layout.parts
		for (let k = 0, at = 1; k < w[0]; k++) {
			if (w[at] === 4) return true
			at += 2 + 3 * w[at + 1] // compression, channels, three words per channel
		}
		return false
	}
	stageExrBlocks(bytes, layout, row0, rows) {
		this._exrFrame(1, "blocks", bytes, layout, row0, rows)
	}
	exrBlocksStageBytes(bytes, layout, row0, rows) {
		return this._exrFrame(0, "blocks", bytes, layout, row0, rows)
	}
	// the four calls above: the addon function of EXR_FRAME for the records the layout holds (stage: 1 = the staging call, 0 = its byte count)
	_exrFrame(stage, records, bytes, layout, row0, rows) {
		const form = records === "blocks" && Renderer._layoutHasPiz(layout) ? "piz" : records
		const result = addon[EXR_FRAME[form][stage]](this._h, bytes, layout.parts, layout[records], ...this._band(row0, rows))
		if (stage) (this._stagedExrNow = this._stagedExrNow || []).push(bytes) // kept alive until the copies of this batch have executed (stageFlip)
		return result
	}
	// a frame with packed planes, or — no `gbuffer` — with `aov` attribute planes
	stageFrame(frame) {
		this._staged = frame // keep the planes alive while they are in flight
		if (!frame.gbuffer) {
			// an engine-form frame (dump.js): its conventions are set for this call; a reference-form frame after one resets them
			if (frame.aovConventions) this.setAovConventions(Renderer.conventionsFor(frame.aovConventions, frame.camera, frame.prevCamera))
			else if (this._conventionsSet) this.setAovConventions(null)
			return this.stageAov(Object.assign({ depth: frame.depth, direct: frame.direct }, frame.aov))
		}
		for (const [tex, plane] of [[TEX.DEPTH, frame.depth], [TEX.GBUFFER, frame.gbuffer], [TEX.VELOCITY, frame.velocity], [TEX.DIRECT_LIGHT, frame.direct]])
			addon.stageUpload(this._h, tex, ...this._heldPart(tex, plane))
	}
	stageFlip() {
		addon.stageFlip(this._h)
		// rfx_stage_flip returns when the copies published by the PREVIOUS flip have executed: keep this batch's file bytes and the one before's
		this._stagedExrKeep = [this._stagedExrKeep ? this._stagedExrKeep[1] : [], this._stagedExrNow || []]
		this._stagedExrNow = []
	}

	// streamed frame export (rfx.h "streamed frame export"): the tile rows of `source`, encoded on the device.  params: { source, format: EXPORT.*
	// or "f32" / "f16" / "u8_srgb", channels: 3 | 4, tonemap: "linear" | "aces" (u8_srgb only), exposure }
	exportParams(params) {
		const p = Object.assign({ channels: 3, tonemap: 0, exposure: 1 }, params)
		if (typeof p.format === "string") p.format = EXPORT[p.format.toUpperCase()]
		if (typeof p.tonemap === "string") p.tonemap = EXPORT_TONEMAP[p.tonemap]
		if (p.format === undefined || p.tonemap === undefined) throw new RangeError("export: unknown format or tonemap")
		return p
	}
	exportBytes(params) {
		return addon.exportBytes(this._h, this.exportParams(params))
	}
	// the copy of a staged encode writes `out` until its ticket retires (exportWait) or two later tickets exist
	_keepUntilRetired(ticket, out) {
		if (!this._exports) this._exports = new Map()
		this._exports.set(ticket, out)
		for (const t of this._exports.keys()) if (t <= ticket - 2) this._exports.delete(t)
		return ticket
	}
	// one call of ENCODE[kind], blocking (-> out, allocated at the bound when not given) or staged (-> ticket).  Only png's calls take `filter`;
	// options.matches selects the Ex form and passes its flags
	_encode(kind, staged, p, filter, out, options) {
		const [bound, call, stage] = ENCODE[kind], matches = options && options.matches, Ctor = (kind === "export" && EXPORT_ARRAY[p.format]) || Uint8Array
		if (!out && !staged) out = new Ctor(Math.max(1, addon[bound](this._h, p) / Ctor.BYTES_PER_ELEMENT))
		const args = [this._h, p]
		if (kind === "png") args.push(this.pngFilter(filter))
		if (matches) args.push(ENCODE_MATCHES)
		const result = addon[(staged ? stage : call) + (matches ? "Ex" : "")](...args, out)
		return staged ? this._keepUntilRetired(result, out) : out
	}
	// -> Float32Array / Uint16Array (half bits) / Uint8Array of tileRows * width * channels elements, row 0 = bottom; blocks (rfx_export)
	exportFrame(params, out) {
		return this._encode("export", false, this.exportParams(params), undefined, out)
	}
	// enqueue the encode and the copy into `out` (a Renderer.hostAlloc array for an asynchronous copy) -> ticket; `out` is complete once
	// exportWait(ticket) has returned.  Returns only when the export two tickets earlier has completed: alternate two buffers (rfx_stage_export)
	stageExport(params, out) {
		return this._encode("export", true, this.exportParams(params), undefined, out)
	}
	// PNG fragments (rfx.h "PNG fragments"): the U8_SRGB export encoded on the device as the IDAT chunks of the tile rows.  params as for
	// exportFrame (format is U8_SRGB); filter: "adaptive" | "none" | "sub" | "up" | "paeth" or 0..4.  io.pngFromFragments wraps the result.
	pngParams(params) {
		return this.exportParams(Object.assign({}, params, { format: EXPORT.U8_SRGB }))
	}
	pngFilter(filter) {
		const f = filter === undefined ? 0 : typeof filter === "string" ? PNG_FILTERS[filter] : filter
		if (f === undefined) throw new RangeError("png: unknown filter")
		return f
	}
	pngBound(params) {
		return addon.pngBound(this._h, this.pngParams(params || {}))
	}
	// -> the result buffer (Uint8Array of pngBound bytes: 32-byte header, fragment, slack); blocks (rfx_png)
	// options: { matches: true } encodes with run-length matches (rfx.h "Match form": rfx_png_ex with RFX_ENCODE_MATCHES); the same for
	// stagePng, exr and stageExr
	png(params, filter, out, options) {
		return this._encode("png", false, this.pngParams(params), filter, out, options)
	}
	// stageExport's contract with a PNG fragment as the payload; the ticket is one of the same sequence and exportWait retires it (rfx_stage_png)
	stagePng(params, filter, out, options) {
		return this._encode("png", true, this.pngParams(params), filter, out, options)
	}
	// EXR fragments (rfx.h "EXR fragments"): the F16 export encoded on the device as the ZIPS chunks of the tile rows.  params as for exportFrame
	// (format is F16; channels 4 by default).  io.exrFromFragments wraps the result.
	exrParams(params) {
		return this.exportParams(Object.assign({ channels: 4 }, params, { format: EXPORT.F16 }))
	}
	exrBound(params) {
		return addon.exrBound(this._h, this.exrParams(params || {}))
	}
	// -> the result buffer (Uint8Array of exrBound bytes: 32-byte header, fragment, slack); blocks (rfx_exr)
	exr(params, out, options) {
		return this._encode("exr", false, this.exrParams(params), undefined, out, options)
	}
	// stageExport's contract with an EXR fragment as the payload; the ticket is one of the same sequence and exportWait retires it (rfx_stage_exr)
	stageExr(params, out, options) {
		return this._encode("exr", true, this.exrParams(params), undefined, out, options)
	}
	exportWait(ticket) {
		addon.exportWait(this._h, ticket)
		if (this._exports) this._exports.delete(ticket)
	}

	download(tex, row0, rows) {
		const band = this._heldBand(tex, row0, rows)
		const f = FORMAT[tex]
		const out = new f[0](band[1] * (tex === TEX.BLUE_NOISE ? 128 : this.width) * f[1])
		addon.download(this._h, tex, out, ...band)
		return out
	}

	clear(tex) {
		addon.clear(this._h, tex)
	}

	// importer: unpacked attribute planes (Float32Arrays over rows [row0, row0+rows)) -> the packed render targets (rfx_pack_gbuffer / _velocity)
	packGBuffer(aov, row0, rows) {
		addon.packGBuffer(this._h, aov, ...this._heldBand(TEX.GBUFFER, row0, rows))
	}
	packVelocity(aov, row0, rows) {
		addon.packVelocity(this._h, aov, ...this._heldBand(TEX.VELOCITY, row0, rows))
	}

	// scene.environment: Float32Array(H*W*4) equirect map (row 0 = bottom) or null — rfx_set_environment
	setEnvironment(data, width, height, halfFloatType, halfStoreRTZ) {
		addon.setEnvironment(this._h, data || null, width || 0, height || 0, halfFloatType ? 1 : 0, halfStoreRTZ ? 1 : 0)
		this._envSize = data ? [width | 0, height | 0] : null // (downloadEnvironmentImportance)
	}

	// EquirectHdrInfoUniform's tables for importanceSampling (js/envmap.js buildImportance) — rfx_set_environment_importance
	setEnvironmentImportance(marginalWeights, conditionalWeights, totalSumValue) {
		const whole = Math.trunc(totalSumValue) // ~~totalSumValue (EquirectHdrInfoUniform.js:391-394)
		addon.setEnvironmentImportance(this._h, marginalWeights, conditionalWeights, whole, totalSumValue - whole)
	}

	// the four draws + the framebuffer copy (include/rfx.h)
	ssgiMarch(uniforms) {
		addon.ssgiMarch(this._h, uniforms)
	}
	// restrict the rows the following draws produce to [y0, y1); no arguments resets (rfx_set_row_window)
	setRowWindow(y0, y1) {
		addon.setRowWindow(this._h, y0 | 0, y1 | 0)
	}
	// CubeToEquirectEnvPass's draw + read-back (rfx_cube_to_equirect): faces = Float32Array(6 * size * size * 4), +X -X +Y -Y +Z -Z, row j = t
	// as uploaded; returns Float32Array(width * height * 4), row 0 = bottom
	cubeToEquirect(faces, size, width, height, generateMipmaps) {
		const out = new Float32Array(width * height * 4)
		addon.cubeToEquirect(this._h, faces, size | 0, generateMipmaps ? 1 : 0, out, width | 0, height | 0)
		return out
	}
	// ---- the environment kept on the device (include/rfx.h): stream-ordered, no read-back, no host build of the tables
	get hasEnvDevice() {
		return typeof addon.buildEnvironmentImportance === "function"
	}
	// cubeToEquirect + setEnvironment(equirect, width, height, false, false) with the map never leaving the device (rfx_set_environment_cube);
	// `faces` may be reused on return.  Invalidates the importance tables
	setEnvironmentCube(faces, size, width, height, generateMipmaps) {
		addon.setEnvironmentCube(this._h, faces, size | 0, generateMipmaps ? 1 : 0, width | 0, height | 0)
		this._envSize = [width | 0, height | 0]
	}
	// the tables and sums of js/envmap.js buildImportance, built from level 0 of the held environment (K10), bit for bit
	buildEnvironmentImportance(flipY) {
		addon.buildEnvironmentImportance(this._h, flipY ? 1 : 0)
	}
	// { marginalWeights, conditionalWeights, totalSumValue, whole, decimal } as the context holds them (synchronises); width, height: the
	// environment's, remembered from setEnvironment / setEnvironmentCube when not given
	downloadEnvironmentImportance(width, height) {
		const [w, h] = width ? [width | 0, height | 0] : this._envSize || [0, 0]
		if (!w || !h) throw new Error("downloadEnvironmentImportance: no environment set")
		const marginalWeights = new Float32Array(h), conditionalWeights = new Float32Array(w * h)
		return Object.assign({ marginalWeights, conditionalWeights }, addon.downloadEnvironmentImportance(this._h, marginalWeights, conditionalWeights, w, h))
	}
	// which vUv the following draws' fragments see (rfx_set_uv_model): "ideal" = (i + 0.5) / n, "reference_gl" = what the reference GL's
	// rasteriser interpolates for three's full-screen triangle, bit for bit
	setUvModel(model) {
		const m = { ideal: 0, reference_gl: 1 }[model]
		if (m === undefined) throw new RangeError("setUvModel: \"ideal\" or \"reference_gl\"")
		addon.setUvModel(this._h, m)
	}
	// the same draw in two launches (rfx_ssgi_trace / rfx_ssgi_shade): only the second reads last frame's composed GI
	ssgiTrace(uniforms) {
		addon.ssgiTrace(this._h, uniforms)
	}
	ssgiShade(uniforms) {
		addon.ssgiShade(this._h, uniforms)
	}
	temporalReproject(uniforms) {
		addon.temporalReproject(this._h, uniforms)
	}
	// renderer.copyFramebufferToTexture of TemporalReprojectPass.js:198-201
	copyFramebuffer(dstTex) {
		addon.copyFramebuffer(this._h, dstTex)
	}
	poissonDenoise(uniforms) {
		addon.poissonDenoise(this._h, uniforms)
	}
	compose(uniforms) {
		addon.compose(this._h, uniforms)
	}

	// SSGIEffect's own fragment (ssgi_compose.frag mainImage)
	finalCompose(uniforms) {
		addon.finalCompose(this._h, uniforms)
	}
	// MotionBlurEffect's fragment (K6, rfx_motion_blur) -> TEX.MOTION_BLUR
	motionBlur(uniforms) {
		addon.motionBlur(this._h, uniforms)
	}
	// a row tile: its rows of the source into TEX.BLUR_SOURCE; arms the tiled motionBlur for that source (rfx_motion_blur_stage)
	motionBlurStage(uniforms) {
		addon.motionBlurStage(this._h, uniforms)
	}
	// -> Uint32Array(height): bit b of entry y = motionBlur(uniforms) loads a source texel of frame row y in column block b (rfx_motion_blur_reach_mask)
	motionBlurReachMask(uniforms) {
		const mask = new Uint32Array(this.height)
		addon.motionBlurReachMask(this._h, uniforms, mask)
		return mask
	}
	// stage + reach mask + the exchange of the named column blocks over the context's communicator -> bytes received (rfx_motion_blur_gather)
	motionBlurGather(uniforms) {
		return addon.motionBlurGather(this._h, uniforms)
	}

	sync() {
		addon.sync(this._h)
	}
	haloViolations() {
		return addon.haloViolations(this._h)
	}
	// per-draw device timing inside a frame loop (rfx_profile / rfx_profile_read): { ms: [...], launches: [...] } indexed by RFX_PROF_* of include/rfx.h
	profile(enable) {
		addon.profile(this._h, enable ? 1 : 0)
	}
	profileRead() {
		return addon.profileRead(this._h)
	}
	timeBegin() {
		addon.timeBegin(this._h)
	}
	timeEnd() {
		return addon.timeEnd(this._h)
	}
	dispose() {
		this._h = null // the context is destroyed by the handle's finalizer
	}
}

module.exports = { Renderer, TEX, FORMAT, EXPORT, EXPORT_ARRAY, PROF_KINDS, PROF_KINDS_ALL, PNG_FILTERS, ENCODE_MATCHES, loadBlueNoiseTable, abiVersion: addon.abiVersion, constants: addon.constants }
