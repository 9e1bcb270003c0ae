"use strict"
// Per-frame output of an offline run (run_dump.js --framesOut): every frame leaves the device through the streamed export (rfx.h "streamed
// frame export") — encoded by K7, copied on the download stream into one of two pinned buffers — and is written by the existing writers,
// which take the device's bytes as they are.  Python twin: rfx_amd/frames.py.
//   png -> RFX_EXPORT_U8_SRGB x 3 (tonemap / exposure)     exr -> RFX_EXPORT_F16 x 4     pfm -> RFX_EXPORT_F32 x 3
// submit(source) is called once per frame AFTER the frame's draws are enqueued: it stages this frame's export, then waits for the PREVIOUS
// frame's ticket — which has had this frame's draws to hide behind — and writes it.  At most two exports are in flight; finish() waits for
// the last one.
const fs = require("fs")
const path = require("path")
const { Renderer, EXPORT, EXPORT_ARRAY } = require("./Renderer")
const io = require("./imageio")

const FRAME_FORMATS = { png: [EXPORT.U8_SRGB, 3], exr: [EXPORT.F16, 4], pfm: [EXPORT.F32, 3] }

class FrameExporter {
	// options: { format: "png" | "exr" | "pfm", tonemap: "aces" | "linear", exposure, hostAlloc, write,
	//            encode: "host" (default) | "device" — png only: the frame leaves the device as a PNG fragment (rfx_stage_png, K8) and the host
	//            only wraps and writes it; filter: the fragment's filter, "adaptive" by default;
	//            compression: "none" (default) | "zips" — exr only: the frame leaves the device as finished ZIPS chunks (rfx_stage_exr, rfx.h "EXR
	//            fragments") and the host only wraps and writes them;
	//            matches: false (default) | true — with encode "device" or compression "zips" only: the device encode with run-length matches
	//            (rfx.h "Match form") }
	constructor(renderer, dir, options) {
		options = options || {}
		this.renderer = renderer
		this.dir = dir
		this.format = options.format || "png"
		const f = FRAME_FORMATS[this.format]
		if (!f) throw new RangeError("framesFormat: \"png\", \"exr\" or \"pfm\"")
		const tonemap = options.tonemap === undefined ? "aces" : options.tonemap
		if (tonemap !== "aces" && tonemap !== "linear") throw new RangeError("tonemap: \"aces\" or \"linear\"")
		this.params = { format: f[0], channels: f[1], tonemap: f[0] === EXPORT.U8_SRGB ? tonemap : 0, exposure: f[0] === EXPORT.U8_SRGB && options.exposure !== undefined ? options.exposure : 1 }
		this.encode = options.encode === undefined ? "host" : options.encode
		if (this.encode !== "host" && this.encode !== "device") throw new RangeError("framesEncode: \"host\" or \"device\"")
		if (this.encode === "device" && this.format !== "png") throw new RangeError("framesEncode \"device\" is for framesFormat \"png\" only")
		this.filter = options.filter === undefined ? "adaptive" : options.filter
		this.compression = options.compression === undefined ? "none" : options.compression
		if (this.compression !== "none" && this.compression !== "zips") throw new RangeError("framesCompression: \"none\" or \"zips\"")
		if (this.compression === "zips" && this.format !== "exr") throw new RangeError("framesCompression \"zips\" is for framesFormat \"exr\" only")
		const zips = this.compression === "zips"
		this.matches = !!options.matches
		if (this.matches && this.encode !== "device" && !zips) throw new RangeError("framesMatches is for framesEncode \"device\" or framesCompression \"zips\" only")
		const n = this.encode === "device" ? renderer.pngBound(this.params) : zips ? renderer.exrBound(this.params) : renderer.width * renderer.tileRows * f[1]
		const alloc = options.hostAlloc || Renderer.hostAlloc
		this.buffers = [0, 1].map(() => alloc(zips ? Uint8Array : EXPORT_ARRAY[f[0]], n))
		this.write = options.write || ((index, data) => this.writeFrame(index, data))
		this.count = 0
		this.pending = null // { ticket, index, buffer }
	}
	writeFrame(index, data) {
		const file = path.join(this.dir, "frame_" + String(index).padStart(5, "0") + "." + this.format)
		const w = this.renderer.width, h = this.renderer.tileRows
		if (this.encode === "device") fs.writeFileSync(file, io.pngFromFragments(w, h, 3, [data]))
		else if (this.compression === "zips") fs.writeFileSync(file, io.exrFromFragments(w, h, 4, [data]))
		else if (this.format === "png") io.writePNG(file, data, w, h, 3)
		else if (this.format === "exr") io.writeEXR(file, data, w, h, true)
		else io.writePFM(file, data, w, h, 3)
	}
	submit(source) {
		const index = this.count++
		const buffer = this.buffers[index & 1]
		const ticket = this.encode === "device" ? this.renderer.stagePng(Object.assign({ source }, this.params), this.filter, buffer, { matches: this.matches })
			: this.compression === "zips" ? this.renderer.stageExr(Object.assign({ source }, this.params), buffer, { matches: this.matches })
			: this.renderer.stageExport(Object.assign({ source }, this.params), buffer)
		this.retire()
		this.pending = { ticket, index, buffer }
	}
	retire() {
		const p = this.pending
		if (!p) return
		this.pending = null
		this.renderer.exportWait(p.ticket)
		this.write(p.index, p.buffer)
	}
	finish() {
		this.retire()
	}
}

module.exports = { FrameExporter, FRAME_FORMATS }
