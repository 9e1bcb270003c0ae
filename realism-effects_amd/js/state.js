"use strict"
// Checkpoint and resume of the temporal state (Python twin: rfx_amd/state.py — the two hosts read each other's checkpoints).
//
// Everything the chain carries from one frame to the next is either a device slot a later frame reads before writing — or leaves partly
// unwritten: K2, K3 and K4 discard background texels, which keep the target's previous contents — or a handful of host-side numbers (the
// blue-noise recurrences, keepData, the previous camera, frame counters).  saveState() writes both down at a frame boundary; loadState()
// puts them back into fresh effects on a fresh context, and the frames that follow are byte-identical to an uninterrupted run.
//
// A checkpoint is a directory:
//   state.json                  the header, written LAST (to a temporary name, then renamed over the previous one)
//   <slot>.<generation>.plane   one raw whole-frame plane per saved slot: all H rows in frame order, the bytes rfx_download returns
// The planes are whole-frame whatever the tiling: a row tile writes its own rows at their offset, rank 0 writes the header, and any rank
// count loads the result — each tile takes the rows it holds, halo included, slots held whole (the composed GI) whole, so no exchange is
// needed after a load.  Which slots are saved is asked of the effect objects (stateSlots()); input planes are not state.
//
// Every save uses a new generation number in the plane names, so an interrupted save never touches the files the existing header names:
// the previous checkpoint stays loadable until the new header has replaced it, and planes without a header are never read.  A load
// validates the header, every plane (size, SHA-256) and the fit to the running effects (class, texture count, target type, denoiseMode,
// resolutionScale) BEFORE it touches an effect or the device, and names the field it refuses (StateError.field).
const fs = require("fs")
const path = require("path")
const crypto = require("crypto")
const { TEX, FORMAT: TEX_FORMAT } = require("./Renderer")
const { StateError } = require("./effects")

const FORMAT = "rfx-temporal-state"
const VERSION = 1
const HEADER = "state.json"
const TEX_NAMES = []
for (const k of Object.keys(TEX)) TEX_NAMES[TEX[k]] = k.toLowerCase()

// the two file operations of a save (tests make them fail part-way)
const io = {
	// `buf` at `offset` of `file` (created if missing, never truncated: other ranks write other rows of the same plane)
	write(file, offset, buf) {
		const fd = fs.openSync(file, fs.constants.O_RDWR | fs.constants.O_CREAT, 0o644)
		try {
			let done = 0
			while (done < buf.length) done += fs.writeSync(fd, buf, done, buf.length - done, offset + done)
			fs.fsyncSync(fd)
		} finally {
			fs.closeSync(fd)
		}
	},
	replace(src, dst) {
		fs.renameSync(src, dst)
	}
}

function texelBytes(tex) {
	return TEX_FORMAT[tex][0].BYTES_PER_ELEMENT * TEX_FORMAT[tex][1]
}
function asList(effects) {
	return Array.isArray(effects) ? effects : [effects]
}
// the slots a checkpoint of these effects holds, in a fixed order (each effect's stateSlots(), first mention wins)
function stateSlots(effects) {
	const slots = []
	for (const e of asList(effects)) for (const t of e.stateSlots()) if (slots.indexOf(t) < 0) slots.push(t)
	return slots
}
function geometry(renderer) {
	const H = renderer.height
	const y0 = renderer.tileY0 || 0
	return { W: renderer.width, H, y0, rows: renderer.tileRows === undefined ? H - y0 : renderer.tileRows, rank: renderer.rank || 0, world: renderer.nranks || 1 }
}
function barrier(renderer, world) {
	if (world > 1) {
		if (!renderer.stateBarrier) throw new Error("saveState: a row-tiled renderer needs stateBarrier() (TiledRenderer has one)")
		renderer.stateBarrier()
	}
}
// frame boundary: no exchange in flight, every draw finished
function settle(renderer) {
	if (renderer.commWait) renderer.commWait()
	renderer.sync()
}
function sha256(buf) {
	return crypto.createHash("sha256").update(buf).digest("hex")
}
function bytesOf(a) {
	return Buffer.from(a.buffer, a.byteOffset, a.byteLength)
}

// the parsed header of the checkpoint in `dir`, its format and version checked
function readHeader(dir) {
	const file = path.join(dir, HEADER)
	let text, header
	try {
		text = fs.readFileSync(file, "utf8")
	} catch (e) {
		throw new StateError("header", "no checkpoint in " + dir + " (" + e.message + ")")
	}
	try {
		header = JSON.parse(text)
	} catch (e) {
		throw new StateError("header", file + " is not JSON (" + e.message + ")")
	}
	if (!header || typeof header !== "object" || header.format !== FORMAT)
		throw new StateError("format", JSON.stringify(header && header.format) + ", expected " + JSON.stringify(FORMAT))
	if (header.version !== VERSION) throw new StateError("version", JSON.stringify(header.version) + ", this build reads version " + VERSION)
	return header
}
function previousGeneration(dir) {
	try {
		const g = readHeader(dir).generation
		return Number.isInteger(g) && g >= 0 ? g : 0
	} catch (e) {
		if (e instanceof StateError) return 0
		throw e
	}
}

// Write the temporal state of `effects` on `renderer` into `dir` and return the header.  Call it between frames.  On a row-tiled renderer
// every rank calls it: each writes its own rows, rank 0 the header.
function saveState(dir, renderer, effects) {
	effects = asList(effects)
	const g = geometry(renderer)
	settle(renderer)
	fs.mkdirSync(dir, { recursive: true })
	const generation = previousGeneration(dir) + 1 // (the header does not change before the barrier below)
	const slots = stateSlots(effects)
	const names = {}
	const digests = {}
	for (const t of slots) {
		names[t] = TEX_NAMES[t] + "." + generation + ".plane"
		const band = bytesOf(renderer.download(t, g.y0, g.rows))
		const rowBytes = g.W * texelBytes(t)
		if (band.length !== g.rows * rowBytes)
			throw new Error("saveState: " + TEX_NAMES[t] + " rows [" + g.y0 + ", " + (g.y0 + g.rows) + ") came back as " + band.length + " bytes, expected " + g.rows * rowBytes)
		io.write(path.join(dir, names[t]), g.y0 * rowBytes, band)
		if (g.rows === g.H) digests[t] = sha256(band) // the whole plane went through this rank's hands: no need to read it back
	}
	barrier(renderer, g.world) // every rank's rows are on disk
	const header = { format: FORMAT, version: VERSION, generation, width: g.W, height: g.H, planes: [], effects: effects.map(e => e.getState()) }
	if (g.rank === 0) {
		for (const t of slots) {
			const file = path.join(dir, names[t])
			fs.truncateSync(file, g.H * g.W * texelBytes(t)) // (a longer leftover of an interrupted save at another frame size)
			header.planes.push({ slot: TEX_NAMES[t], file: names[t], texelBytes: texelBytes(t), rows: g.H, sha256: digests[t] || sha256(fs.readFileSync(file)) })
		}
		const tmp = path.join(dir, HEADER + ".tmp")
		if (fs.existsSync(tmp)) fs.unlinkSync(tmp)
		io.write(tmp, 0, Buffer.from(JSON.stringify(header, null, 1)))
		io.replace(tmp, path.join(dir, HEADER)) // the checkpoint exists from here on
		const keep = Object.keys(names).map(t => names[t])
		for (const name of fs.readdirSync(dir)) // the planes of earlier generations
			if (name.endsWith(".plane") && keep.indexOf(name) < 0) try { fs.unlinkSync(path.join(dir, name)) } catch (e) { /* another process's */ }
	}
	barrier(renderer, g.world) // nobody returns (to load, or to save again) before the header is there
	return g.rank === 0 ? header : readHeader(dir)
}

function uploadHeld(renderer, tex, plane, W) {
	const held = renderer.heldRows(tex)
	const per = TEX_FORMAT[tex][1] * W
	renderer.upload(tex, plane.subarray(held[0] * per, (held[0] + held[1]) * per), held[0], held[1])
}

// Restore the checkpoint in `dir` into `effects` and `renderer` (fresh or running) and return its header.  Everything is validated first:
// a refusal throws a StateError naming the field and leaves the effects and the device untouched.
function loadState(dir, renderer, effects) {
	effects = asList(effects)
	const W = renderer.width, H = renderer.height
	const header = readHeader(dir)
	if (header.width !== W) throw new StateError("width", "saved " + JSON.stringify(header.width) + ", the renderer has " + W)
	if (header.height !== H) throw new StateError("height", "saved " + JSON.stringify(header.height) + ", the renderer has " + H)
	const saved = header.effects
	if (!Array.isArray(saved) || saved.length !== effects.length)
		throw new StateError("effects", (Array.isArray(saved) ? saved.length : "none") + " saved, " + effects.length + " given")
	effects.forEach((e, i) => {
		if (!saved[i] || typeof saved[i] !== "object") throw new StateError("effects[" + i + "]", "not a record")
		e.checkState(saved[i], "effects[" + i + "]")
	})
	// the slots the RESTORED effects will keep (TRAAEffect builds its pass from the record)
	const want = []
	effects.forEach((e, i) => {
		for (const t of e.stateSlotsOf ? e.stateSlotsOf(saved[i]) : e.stateSlots()) if (want.indexOf(t) < 0) want.push(t)
	})
	const planes = header.planes
	if (!Array.isArray(planes) || !planes.every(p => p && typeof p === "object")) throw new StateError("planes", "missing")
	const have = planes.map(p => String(p.slot)).sort()
	const wantNames = want.map(t => TEX_NAMES[t]).sort()
	if (JSON.stringify(have) !== JSON.stringify(wantNames))
		throw new StateError("planes", "saved " + JSON.stringify(have) + ", the running effects keep " + JSON.stringify(wantNames))
	const data = []
	for (const p of planes) {
		const t = TEX_NAMES.indexOf(p.slot)
		const field = "planes[" + p.slot + "]"
		if (p.texelBytes !== texelBytes(t)) throw new StateError(field + ".texelBytes", "saved " + JSON.stringify(p.texelBytes) + ", the slot has " + texelBytes(t))
		if (p.rows !== H) throw new StateError(field + ".rows", "saved " + JSON.stringify(p.rows) + ", the frame has " + H)
		if (typeof p.file !== "string" || path.basename(p.file) !== p.file) throw new StateError(field + ".file", JSON.stringify(p.file) + " is not a file name")
		let raw
		try {
			raw = fs.readFileSync(path.join(dir, p.file))
		} catch (e) {
			throw new StateError(field + ".file", e.message)
		}
		if (raw.length !== H * W * texelBytes(t)) throw new StateError(field + ".size", raw.length + " bytes, expected " + H * W * texelBytes(t))
		if (sha256(raw) !== p.sha256) throw new StateError(field + ".sha256", "the plane does not match its checksum")
		const ab = raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length) // own, aligned ArrayBuffer
		data.push([t, new TEX_FORMAT[t][0](ab)])
	}
	// ---- everything fits: apply
	settle(renderer)
	for (const tp of data) {
		uploadHeld(renderer, tp[0], tp[1], W)
		if (tp[0] === TEX.COMPOSE && renderer.gatherHistoryRGB) {
			// a row-tiled run hands K1 the .rgb twin of the composed GI (tiling.js); it is not a plane of its own
			const rgb = new Float32Array(W * H * 3)
			const src = new Uint32Array(tp[1].buffer, tp[1].byteOffset, tp[1].length) // bit patterns: a NaN's payload survives
			const dst = new Uint32Array(rgb.buffer)
			for (let i = 0, j = 0; i < src.length; i += 4, j += 3) {
				dst[j] = src[i]
				dst[j + 1] = src[i + 1]
				dst[j + 2] = src[i + 2]
			}
			uploadHeld(renderer, TEX.COMPOSE_RGB, rgb, W)
		}
	}
	effects.forEach((e, i) => e.setState(saved[i]))
	renderer.sync()
	return header
}

module.exports = { saveState, loadState, readHeader, stateSlots, STATE_FORMAT: FORMAT, STATE_VERSION: VERSION, stateIO: io }
