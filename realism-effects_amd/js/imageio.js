"use strict"
// On-disk outputs of an offline run (SURVEY.md §8 f4; Python twin: rfx_amd/imageio.py): the effect's final image (RFX_TEX_FINAL,
// RGBA32F, row 0 = bottom) as OpenEXR (scene-linear, float32, uncompressed scanlines), PFM, or a tone-mapped 8-bit PNG — ACES filmic,
// the reference example's renderer.toneMapping (example/main.js), then the sRGB transfer function.
const fs = require("fs")
const zlib = require("zlib")

function crc32(buf) {
	let table = crc32.table
	if (!table) {
		table = crc32.table = new Int32Array(256)
		for (let n = 0; n < 256; n++) {
			let c = n
			for (let k = 0; k < 8; k++) c = c & 1 ? 0xedb88320 ^ (c >>> 1) : c >>> 1
			table[n] = c
		}
	}
	let c = -1
	for (let i = 0; i < buf.length; i++) c = table[(c ^ buf[i]) & 255] ^ (c >>> 8)
	return (c ^ -1) >>> 0
}

function pngChunk(tag, payload) {
	const body = Buffer.concat([Buffer.from(tag, "ascii"), payload])
	const out = Buffer.alloc(8 + payload.length + 4)
	out.writeUInt32BE(payload.length, 0)
	body.copy(out, 4)
	out.writeUInt32BE(crc32(body), 8 + payload.length)
	return out
}

// The host's wrap of include/rfx.h "PNG fragments": `fragments` are the result buffers of Renderer.png / stagePng (32-byte header, then the IDAT
// chunks of a tile's rows), TOP TILE FIRST -> the file's bytes (a Buffer).  The tiles' Adler-32s are combined, never recomputed.
function pngFromFragments(width, height, channels, fragments) {
	if (channels !== 3 && channels !== 4) throw new RangeError("PNG: 3 or 4 channels")
	const ihdr = Buffer.alloc(13)
	ihdr.writeUInt32BE(width, 0)
	ihdr.writeUInt32BE(height, 4)
	ihdr[8] = 8
	ihdr[9] = channels === 3 ? 2 : 6
	const parts = [Buffer.from([0x89, 0x50, 0x4e, 0x47, 0x0d, 0x0a, 0x1a, 0x0a]), pngChunk("IHDR", ihdr), pngChunk("IDAT", Buffer.from([0x78, 0x01]))]
	let A = 1, B = 0, raw = 0
	for (const f of fragments) {
		const b = Buffer.from(f.buffer, f.byteOffset, f.byteLength)
		const n = Number(b.readBigUInt64LE(0)), a2 = b.readUInt32LE(8), b2 = b.readUInt32LE(12), len2 = Number(b.readBigUInt64LE(16))
		if (32 + n > b.length) throw new RangeError("PNG fragment: header says " + n + " bytes, buffer holds " + (b.length - 32))
		parts.push(b.subarray(32, 32 + n))
		B = (B + b2 + (len2 % 65521) * (A + 65520)) % 65521 // B1 + B2 + len2 * (A1 - 1)   (below 2^53: 65520 * 131040)
		A = (A + a2 + 65520) % 65521 // A1 + A2 - 1
		raw += len2
	}
	if (raw !== height * (1 + width * channels)) throw new RangeError("PNG fragments: " + raw + " filtered bytes do not make a " + width + " x " + height + " x " + channels + " image")
	const tail = Buffer.alloc(6)
	tail[0] = 0x03
	tail.writeUInt32BE(((B << 16) | A) >>> 0, 2)
	parts.push(pngChunk("IDAT", tail), pngChunk("IEND", Buffer.alloc(0)))
	return Buffer.concat(parts)
}

// rgba8: Uint8Array(H*W*channels), row 0 = bottom
function writePNG(file, rgb8, width, height, channels) {
	const stride = width * channels
	const raw = Buffer.alloc((stride + 1) * height)
	for (let y = 0; y < height; y++) {
		raw[y * (stride + 1)] = 0 // filter type 0
		Buffer.from(rgb8.buffer, rgb8.byteOffset + (height - 1 - y) * stride, stride).copy(raw, y * (stride + 1) + 1) // PNG rows run top -> bottom
	}
	const chunk = (tag, payload) => {
		const body = Buffer.concat([Buffer.from(tag, "ascii"), payload])
		const out = Buffer.alloc(8 + payload.length + 4)
		out.writeUInt32BE(payload.length, 0)
		body.copy(out, 4)
		out.writeUInt32BE(crc32(body), 8 + payload.length)
		return out
	}
	const ihdr = Buffer.alloc(13)
	ihdr.writeUInt32BE(width, 0)
	ihdr.writeUInt32BE(height, 4)
	ihdr[8] = 8
	ihdr[9] = channels === 3 ? 2 : 6
	fs.writeFileSync(file, Buffer.concat([Buffer.from([0x89, 0x50, 0x4e, 0x47, 0x0d, 0x0a, 0x1a, 0x0a]), chunk("IHDR", ihdr), chunk("IDAT", zlib.deflateSync(raw, { level: 6 })), chunk("IEND", Buffer.alloc(0))]))
}

// ACES filmic (three.js ACESFilmicToneMapping: RRT + ODT fit, exposure / 0.6) or "linear" (clamp), then the sRGB OETF -> Uint8Array RGB
function tonemap(rgba, width, height, operator, exposure) {
	operator = operator || "aces"
	exposure = exposure === undefined ? 1 : exposure
	const out = new Uint8Array(width * height * 3)
	const san = v => (v !== v ? 0 : Math.min(Math.max(v, 0), 65504))
	const fit = v => (v * (v + 0.0245786) - 0.000090537) / (v * (0.983729 * v + 0.432951) + 0.238081)
	const oetf = v => {
		v = Math.min(Math.max(v, 0), 1)
		return Math.floor((v <= 0.0031308 ? v * 12.92 : 1.055 * Math.pow(v, 1 / 2.4) - 0.055) * 255 + 0.5)
	}
	for (let i = 0; i < width * height; i++) {
		let r = san(rgba[4 * i]) * exposure, g = san(rgba[4 * i + 1]) * exposure, b = san(rgba[4 * i + 2]) * exposure
		if (operator === "aces") {
			r /= 0.6
			g /= 0.6
			b /= 0.6
			const r1 = fit(0.59719 * r + 0.35458 * g + 0.04823 * b), g1 = fit(0.076 * r + 0.90834 * g + 0.01566 * b), b1 = fit(0.0284 * r + 0.13383 * g + 0.83777 * b)
			r = 1.60475 * r1 - 0.53108 * g1 - 0.07367 * b1
			g = -0.10208 * r1 + 1.10813 * g1 - 0.00605 * b1
			b = -0.00327 * r1 - 0.07276 * g1 + 1.07602 * b1
		}
		out[3 * i] = oetf(r)
		out[3 * i + 1] = oetf(g)
		out[3 * i + 2] = oetf(b)
	}
	return out
}

// scene-linear RGBA32F -> single-part scanline OpenEXR, FLOAT channels A B G R, no compression.  half: `rgba` is a Uint16Array of binary16
// BITS (the device's RFX_EXPORT_F16 stream as it is: no float round trip) and the channels are HALF — byte for byte what
// rfx_amd/imageio.py write_exr(compression="none", half=True) writes for the same plane
function writeEXR(file, rgba, width, height, half) {
	const sz = half ? 2 : 4
	const names = ["A", "B", "G", "R"], src = [3, 2, 1, 0]
	const attr = (name, type, payload) => Buffer.concat([Buffer.from(name + "\0" + type + "\0", "ascii"), (() => { const b = Buffer.alloc(4); b.writeInt32LE(payload.length, 0); return b })(), payload])
	const chlist = Buffer.concat(names.map(n => { const b = Buffer.alloc(n.length + 1 + 16); b.write(n, 0, "ascii"); b.writeInt32LE(half ? 1 : 2, n.length + 1); b.writeInt32LE(1, n.length + 9); b.writeInt32LE(1, n.length + 13); return b }).concat([Buffer.from([0])]))
	const box = Buffer.alloc(16)
	box.writeInt32LE(width - 1, 8)
	box.writeInt32LE(height - 1, 12)
	const f32 = v => { const b = Buffer.alloc(4); b.writeFloatLE(v, 0); return b }
	const header = Buffer.concat([Buffer.from([0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0]), attr("channels", "chlist", chlist), attr("compression", "compression", Buffer.from([0])),
		attr("dataWindow", "box2i", box), attr("displayWindow", "box2i", box), attr("lineOrder", "lineOrder", Buffer.from([0])), attr("pixelAspectRatio", "float", f32(1)),
		attr("screenWindowCenter", "v2f", Buffer.concat([f32(0), f32(0)])), attr("screenWindowWidth", "float", f32(1)), Buffer.from([0])])
	const lineBytes = 8 + 4 * sz * width
	const table = Buffer.alloc(8 * height), body = Buffer.alloc(lineBytes * height)
	for (let y = 0; y < height; y++) {
		const off = header.length + table.length + y * lineBytes
		table.writeUInt32LE(off >>> 0, 8 * y)
		table.writeUInt32LE(Math.floor(off / 4294967296), 8 * y + 4)
		body.writeInt32LE(y, y * lineBytes)
		body.writeInt32LE(4 * sz * width, y * lineBytes + 4)
		const row = height - 1 - y // EXR y = 0 is the top row
		if (half) for (let c = 0; c < 4; c++) for (let x = 0; x < width; x++) body.writeUInt16LE(rgba[4 * (row * width + x) + src[c]], y * lineBytes + 8 + 2 * (c * width + x))
		else for (let c = 0; c < 4; c++) for (let x = 0; x < width; x++) body.writeFloatLE(rgba[4 * (row * width + x) + src[c]], y * lineBytes + 8 + 4 * (c * width + x))
	}
	fs.writeFileSync(file, Buffer.concat([header, table, body]))
}

// The host's wrap of include/rfx.h "EXR fragments": `fragments` are the result buffers of Renderer.exr / stageExr (32-byte header, then the ZIPS
// chunks of a tile's rows), TOP TILE FIRST -> the file's bytes (a Buffer): the scanline header of writeEXR with HALF channels and compression 2,
// the offset table built by walking the chunks' size fields, the fragments.  Byte for byte rfx_amd/imageio.py exr_from_fragments.
function exrFromFragments(width, height, channels, fragments) {
	if (channels !== 3 && channels !== 4) throw new RangeError("EXR: 3 or 4 channels")
	const names = channels === 4 ? ["A", "B", "G", "R"] : ["B", "G", "R"]
	const attr = (name, type, payload) => Buffer.concat([Buffer.from(name + "\0" + type + "\0", "ascii"), (() => { const b = Buffer.alloc(4); b.writeInt32LE(payload.length, 0); return b })(), payload])
	const chlist = Buffer.concat(names.map(n => { const b = Buffer.alloc(n.length + 1 + 16); b.write(n, 0, "ascii"); b.writeInt32LE(1, n.length + 1); b.writeInt32LE(1, n.length + 9); b.writeInt32LE(1, n.length + 13); return b }).concat([Buffer.from([0])]))
	const box = Buffer.alloc(16)
	box.writeInt32LE(width - 1, 8)
	box.writeInt32LE(height - 1, 12)
	const f32 = v => { const b = Buffer.alloc(4); b.writeFloatLE(v, 0); return b }
	const header = Buffer.concat([Buffer.from([0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0]), attr("channels", "chlist", chlist), attr("compression", "compression", Buffer.from([2])),
		attr("dataWindow", "box2i", box), attr("displayWindow", "box2i", box), attr("lineOrder", "lineOrder", Buffer.from([0])), attr("pixelAspectRatio", "float", f32(1)),
		attr("screenWindowCenter", "v2f", Buffer.concat([f32(0), f32(0)])), attr("screenWindowWidth", "float", f32(1)), Buffer.from([0])])
	const n = 2 * width * channels
	const table = Buffer.alloc(8 * height), bodies = []
	let pos = header.length + table.length, y = 0
	for (const f of fragments) {
		const b = Buffer.from(f.buffer, f.byteOffset, f.byteLength)
		const nbytes = Number(b.readBigUInt64LE(0)), chunks = b.readUInt32LE(8), firstY = b.readUInt32LE(12), raw = Number(b.readBigUInt64LE(16))
		if (32 + nbytes > b.length) throw new RangeError("EXR fragment: header says " + nbytes + " bytes, buffer holds " + (b.length - 32))
		if (firstY !== y || raw !== chunks * n || y + chunks > height) throw new RangeError("EXR fragments: a tile of " + chunks + " scanlines from y = " + firstY + " (" + raw + " raw bytes) where y = " + y + " of a " + width + " x " + height + " x " + channels + " image is due")
		const body = b.subarray(32, 32 + nbytes)
		let at = 0
		for (let k = 0; k < chunks; k++) {
			if (at + 8 > nbytes) throw new RangeError("EXR fragment: chunk " + k + " of the tile at y = " + y + " is damaged")
			const cy = body.readInt32LE(at), size = body.readInt32LE(at + 4)
			if (cy !== y + k || size < 0 || size > n || at + 8 + size > nbytes) throw new RangeError("EXR fragment: chunk " + k + " of the tile at y = " + y + " is damaged")
			const off = pos + at
			table.writeUInt32LE(off >>> 0, 8 * (y + k))
			table.writeUInt32LE(Math.floor(off / 4294967296), 8 * (y + k) + 4)
			at += 8 + size
		}
		if (at !== nbytes) throw new RangeError("EXR fragment: " + (nbytes - at) + " bytes behind the last chunk")
		bodies.push(body)
		pos += nbytes
		y += chunks
	}
	if (y !== height) throw new RangeError("EXR fragments: " + y + " scanlines, the image has " + height)
	return Buffer.concat([header, table].concat(bodies))
}

// channels 3: `rgba` is already the file's body, tightly packed RGB float32 (the device's RFX_EXPORT_F32 x 3 stream), written as it is
function writePFM(file, rgba, width, height, channels) {
	let body
	if (channels === 3) body = Buffer.from(rgba.buffer, rgba.byteOffset, 12 * width * height)
	else {
		body = Buffer.alloc(12 * width * height)
		for (let i = 0; i < width * height; i++) for (let c = 0; c < 3; c++) body.writeFloatLE(rgba[4 * i + c], 4 * (3 * i + c))
	}
	fs.writeFileSync(file, Buffer.concat([Buffer.from("PF\n" + width + " " + height + "\n-1.0\n", "ascii"), body]))
}

// ---- AOV EXR -> the descriptor of the device decode (rfx.h "streamed EXR frames"; the twin of rfx_amd/imageio.py exr_aov_layout)
// layer.channel names an AOV EXR is expected to carry, in rfx_aov_frame's plane order (pass `names` to override a layer's channels)
const AOV_LAYOUT = {
	diffuse: ["diffuse.R", "diffuse.G", "diffuse.B", "diffuse.A"],
	normal: ["normal.X", "normal.Y", "normal.Z"],
	roughness: ["roughness.Y"],
	metalness: ["metalness.Y"],
	emissive: ["emissive.R", "emissive.G", "emissive.B"],
	velocity: ["velocity.X", "velocity.Y"],
	depth: ["depth.Z"],
	direct: ["direct.R", "direct.G", "direct.B", "direct.A"]
}
class ExrNotStreamable extends Error {}
// Parse the header(s) and offset table(s) of a scanline AOV EXR held in `buffer` (a Buffer / Uint8Array: the whole file).  Returns
// { width, height, fileBytes, parts: Int32Array, chunks: Uint8Array, chunkCount, planes: { name: [channels, "half" | "float"] } } — `parts` and
// `chunks` in the layout Renderer.stageExrAov hands to the addon: parts = [n, then per part: compression, channels, then per channel: pixel type,
// plane or -1, component]; chunks = 32-byte records { int32 part, y, rows, 0; uint64 offset of the packed data, packed bytes }.
// Throws ExrNotStreamable for what stays on the host: tiled or deep files, RLE / PIZ / PXR24 parts, UINT channels, a dataWindow that is not the
// displayWindow.
// options.forms = "blocks" (rfx.h "EXR blocks", Renderer.stageExrBlocks): `blocks` in place of `chunks` — 40-byte records { int32 part, x, y, cols,
// rows, 0; uint64 offset of the packed data, packed bytes }, a scanline chunk or a tile each — and `blockCount`; scanline and tiled parts (level 0
// of a mip-mapped one), NONE / RLE / ZIPS / ZIP / PXR24, any data window every part shares (the frame is the data window).  ExrNotStreamable then:
// PIZ, deep data, UINT channels, parts of different data windows.
// options.piz = true (with forms "blocks"; rfx.h "EXR blocks with PIZ"): PIZ parts too — compression 4, a scanline block of 32 rows —, which
// Renderer.stageExrBlocks sends through rfx_stage_exr_blocks_piz; tiles of 128 x 128 texels or more stay ExrNotStreamable.  The default refuses PIZ.
const ENGINE_DEPTH_LAYOUT = { position: ["position.X", "position.Y", "position.Z"], view_z: ["depth.Z"] }
function exrAovLayout(buffer, names, options) {
	const forms = (options && options.forms) || "scanline"
	if (forms !== "scanline" && forms !== "blocks") throw new Error('forms: "scanline" or "blocks"')
	const asBlocks = forms === "blocks"
	const piz = !!(options && options.piz)
	if (piz && !asBlocks) throw new Error('piz: true needs forms: "blocks"')
	const b = Buffer.from(buffer.buffer, buffer.byteOffset, buffer.byteLength)
	if (b.length < 8 || b.readUInt32LE(0) !== 0x01312f76) throw new Error("not an OpenEXR file")
	const version = b.readInt32LE(4)
	if (version & 0x800) throw new ExrNotStreamable("deep data")
	if (version & 0x200 && !asBlocks) throw new ExrNotStreamable("a tiled file")
	const multipart = !!(version & 0x1000)
	const cstr = pos => {
		const e = b.indexOf(0, pos)
		if (e < 0) throw new Error("damaged EXR header")
		return [b.toString("latin1", pos, e), e + 1]
	}
	const headers = []
	let pos = 8
	for (;;) {
		const attrs = {}
		while (b[pos] !== 0) {
			let name, type
			;[name, pos] = cstr(pos)
			;[type, pos] = cstr(pos)
			const n = b.readInt32LE(pos)
			attrs[name] = b.subarray(pos + 4, pos + 4 + n)
			pos += 4 + n
		}
		pos++
		headers.push(attrs)
		if (!multipart || b[pos] === 0) break
	}
	if (multipart) pos++
	// names may carry ONE of `position` / `view_z` (rfx.h "AOV conventions": an array of channel names, or null for the default ones): the
	// depth plane is then fed by those channels — components 0..2 of a world position, or the view Z
	const given = Object.assign({}, names || {})
	const engine = Object.keys(ENGINE_DEPTH_LAYOUT).filter(k => k in given)
	if (engine.length > 1 || (engine.length && "depth" in given)) throw new RangeError("names: depth, position and view_z are one plane")
	for (const k of engine) {
		given.depth = given[k] && given[k].length ? Array.from(given[k]) : ENGINE_DEPTH_LAYOUT[k]
		if (given.depth.length !== ENGINE_DEPTH_LAYOUT[k].length) throw new RangeError("names: " + k + " has " + ENGINE_DEPTH_LAYOUT[k].length + " channels")
		delete given[k]
	}
	const layout = Object.assign({}, AOV_LAYOUT, given)
	const feeds = {}
	Object.keys(AOV_LAYOUT).forEach((key, pi) => layout[key].forEach((cn, j) => (feeds[cn] = [pi, j])))
	const partWords = [headers.length], records = [], seen = {}
	let W = -1, H = -1, window = null
	headers.forEach((attrs, k) => {
		const type = attrs.type ? attrs.type.toString("latin1").replace(/\0+$/, "") : version & 0x200 ? "tiledimage" : "scanlineimage"
		if (type !== "scanlineimage" && !(asBlocks && type === "tiledimage")) throw new ExrNotStreamable("a part of type " + type)
		const tiled = type === "tiledimage"
		const comp = attrs.compression[0]
		if (comp !== 0 && comp !== 2 && comp !== 3 && !(asBlocks && (comp === 1 || comp === 5)) && !(piz && comp === 4)) {
			if (comp === 1 || comp === 4 || comp === 5) throw new ExrNotStreamable("compression " + { 1: "RLE", 4: "PIZ", 5: "PXR24" }[comp])
			throw new Error("compression " + comp + " not supported")
		}
		if (!asBlocks && Buffer.compare(attrs.dataWindow, attrs.displayWindow) !== 0) throw new ExrNotStreamable("the dataWindow is not the displayWindow")
		if (asBlocks && window && Buffer.compare(attrs.dataWindow, window) !== 0) throw new ExrNotStreamable("parts of different data windows")
		window = attrs.dataWindow
		const dw = attrs.dataWindow, y0 = dw.readInt32LE(4)
		const w = dw.readInt32LE(8) - dw.readInt32LE(0) + 1, h = dw.readInt32LE(12) - y0 + 1
		if (W >= 0 && (w !== W || h !== H)) throw new Error("parts of different sizes")
		W = w
		H = h
		const pname = attrs.name ? attrs.name.toString("latin1").replace(/\0+$/, "") : ""
		const cl = attrs.channels, chans = []
		for (let p = 0; cl[p] !== 0; ) {
			const e = cl.indexOf(0, p), nm = cl.toString("latin1", p, e), pt = cl.readInt32LE(e + 1)
			if (cl.readInt32LE(e + 9) !== 1 || cl.readInt32LE(e + 13) !== 1) throw new Error("subsampled channels are not supported")
			if (pt === 0) throw new ExrNotStreamable("UINT channel " + nm)
			const full = nm.includes(".") || !pname ? nm : pname + "." + nm
			const f = feeds[full] || [-1, 0]
			if (f[0] >= 0) {
				if (full in seen) throw new Error("channel " + full + " appears in two parts")
				seen[full] = pt
			}
			chans.push(pt, f[0], f[1])
			p = e + 17
		}
		partWords.push(comp, chans.length / 3, ...chans)
		const per = comp === 3 || comp === 5 ? 16 : comp === 4 ? 32 : 1
		let level0 = Math.ceil(H / per), n = level0, tw = 0, th = 0, ntx = 0, nty = 0
		if (tiled) {
			tw = attrs.tiles.readUInt32LE(0)
			th = attrs.tiles.readUInt32LE(4)
			const mode = attrs.tiles[8]
			if ((mode & 15) === 2) throw new Error("rip-mapped tiles are not supported")
			ntx = Math.ceil(W / tw)
			nty = Math.ceil(H / th)
			level0 = n = ntx * nty // level 0 comes first in the offset table (the only level, or the mip chain's base)
			if (mode & 15) for (let lw = W, lh = H; !(lw === 1 && lh === 1); n += Math.ceil(lw / tw) * Math.ceil(lh / th)) {
				lw = Math.max(1, (lw + (mode >> 4)) >> 1)
				lh = Math.max(1, (lh + (mode >> 4)) >> 1)
			}
		}
		if (attrs.chunkCount) n = attrs.chunkCount.readInt32LE(0)
		if (!tiled) level0 = n
		const hdr = (multipart ? 4 : 0) + (tiled ? 20 : 8)
		for (let i = 0; i < level0; i++) {
			const o = Number(b.readBigUInt64LE(pos + 8 * i))
			if (o + hdr > b.length) throw new Error("a chunk offset outside the file")
			if (multipart && b.readInt32LE(o) !== k) throw new Error("a chunk of part " + k + " carries another part number")
			const packed = b.readInt32LE(o + hdr - 4)
			if (tiled) {
				const tx = b.readInt32LE(o + hdr - 20), ty = b.readInt32LE(o + hdr - 16)
				if (b.readInt32LE(o + hdr - 12) || b.readInt32LE(o + hdr - 8) || tx < 0 || tx >= ntx || ty < 0 || ty >= nty)
					throw new Error("an unexpected tile among the first " + level0 + " of part " + k + " (level 0 comes first)")
				if (comp === 4 && Math.min(tw, W - tx * tw) >= 128 && Math.min(th, H - ty * th) >= 128) throw new ExrNotStreamable("PIZ tiles of 128 x 128 texels or more")
				records.push([k, tx * tw, ty * th, Math.min(tw, W - tx * tw), Math.min(th, H - ty * th), o + hdr, packed])
			} else {
				const y = b.readInt32LE(o + hdr - 8) - y0 // relative to the data window, like a tile's coordinates
				records.push([k, 0, y, W, Math.min(per, H - y), o + hdr, packed])
			}
		}
		pos += 8 * n
	})
	const planes = {}
	for (const key of Object.keys(AOV_LAYOUT)) {
		const have = layout[key].filter(c => c in seen), missing = layout[key].filter(c => !(c in seen))
		if (!have.length) continue
		if (missing.length && !((key === "diffuse" || key === "direct") && missing.length === 1 && missing[0] === layout[key][3]))
			throw new Error("channel(s) " + missing.join(", ") + " of AOV " + key + " missing")
		planes[key] = [have.length, have.every(c => seen[c] === 1) ? "half" : "float"]
	}
	if (asBlocks) {
		const blocks = Buffer.alloc(40 * records.length)
		records.forEach((r, i) => {
			for (let j = 0; j < 5; j++) blocks.writeInt32LE(r[j], 40 * i + 4 * j)
			blocks.writeBigUInt64LE(BigInt(r[5]), 40 * i + 24)
			blocks.writeBigUInt64LE(BigInt(r[6]), 40 * i + 32)
		})
		return { width: W, height: H, fileBytes: b.length, parts: Int32Array.from(partWords), blocks: new Uint8Array(blocks.buffer, blocks.byteOffset, blocks.length), blockCount: records.length, planes }
	}
	const chunks = Buffer.alloc(32 * records.length)
	records.forEach(([part, , y, , rows, offset, packed], i) => {
		chunks.writeInt32LE(part, 32 * i)
		chunks.writeInt32LE(y, 32 * i + 4)
		chunks.writeInt32LE(rows, 32 * i + 8)
		chunks.writeBigUInt64LE(BigInt(offset), 32 * i + 16)
		chunks.writeBigUInt64LE(BigInt(packed), 32 * i + 24)
	})
	return { width: W, height: H, fileBytes: b.length, parts: Int32Array.from(partWords), chunks: new Uint8Array(chunks.buffer, chunks.byteOffset, chunks.length), chunkCount: records.length, planes }
}

module.exports = { writePNG, pngFromFragments, writeEXR, exrFromFragments, writePFM, tonemap, exrAovLayout, ExrNotStreamable, AOV_LAYOUT, ENGINE_DEPTH_LAYOUT }
