#!/usr/bin/env node
"use strict"
// node run_dump.js <dumpdir0> [<dumpdir1> ...] --out <dir> [--steps N --refineSteps N --denoiseIterations N]
// Runs SSGIEffect.update() over a sequence of dumped frames on GPU 0 and writes compose.bin / denoise_b0.bin /
// denoise_b1.bin / temporal0.bin / ssgi.bin / final.bin (the effect's mainImage output) of the LAST frame into --out.
// With --traa '"half"' | '"float"': runs TRAAEffect.update() instead, the dump's direct.bin standing for the composer's
// input buffer (HalfFloatType / FloatType), and writes traa.bin (traa_compose output, RGBA32F) of the last frame.
// --png <file> [--tonemap '"aces"'|'"linear"' --exposure X] / --exr <file> / --pfm <file>: also write final.bin as an image (tone-mapped
// 8-bit sRGB PNG; scene-linear float OpenEXR / PFM) — js/imageio.js.
// --uvModel '"reference_gl"': the reference GL's own vUv instead of (i + 0.5) / n (parity runs against the reference on llvmpipe).
// --stream true: the dumps cross PCIe on the context's upload stream from pinned planes, frame n+1 while frame n is drawn (packed dumps through
// rfx_stage_upload; unpacked and typed ones — aov_*.bin / aov_*.f16.bin — through rfx_stage_aov, which packs them on that stream)
// (rfx_stage_upload / rfx_stage_flip); same outputs.
// With --ranks N (N > 1): the frame is cut into N row tiles, ONE NODE PROCESS PER GPU (this process spawns them: rank r drives
// device r), which exchange halo rows and the composed GI over RCCL through the C ABI (js/tiling.js); rank 0 creates the
// ncclUniqueId and hands it over through a file.  The parent stitches the tiles: the outputs are bit-identical to a --ranks 1 run.
// --historyGather '"all"' (default) | '"bounded"' | '"peer"': how next frame's K1 gets the composed GI of the other tiles (js/tiling.js); "peer"
// moves no collective at all — each rank's kernel loads what its rays read through HIP IPC mappings (the blobs travel through files too).
// --motionBlur '{"intensity":1,"jitter":1,"samples":16}' [--deltaTime X] (default 1/60): MotionBlurEffect after every frame — on the device,
// after SSGIEffect's final image, or with --traa in the README form EffectPass(camera, traaEffect, motionBlurEffect); writes motion_blur.bin
// of the last frame, and --png / --exr / --pfm write the blurred frame instead of final.bin.  With --ranks every rank gathers the source texels
// its streaks reach from their owners (rfx_motion_blur_gather, js/tiling.js) and writes its rows as motion_blur.rank<r>.bin, which the parent
// stitches like the other outputs; the image writers stay whole-frame-only, as they are for every tiled run.
// --framesOut DIR [--framesFormat '"png"'|'"exr"'|'"pfm"'] [--tonemap ... --exposure X]: EVERY frame leaves the device — encoded there (K7: 8-bit
// sRGB x 3, half x 4 or float x 3) and copied on the context's download stream into one of two pinned buffers while the next frame is drawn
// (rfx_stage_export, js/frames.js) — and is written as DIR/frame_%05d.<ext>: the blurred frame with --motionBlur, else the effect's final image
// (with --traa alone: TRAA's accumulated colour, png / pfm).  Every other output is byte-identical with and without it.  Whole-frame runs only:
// with --ranks it throws, like the other image writers.  --framesEncode '"device"' (png only; default '"host"'): the frame leaves the device as a
// finished PNG data stream (rfx_stage_png, K8: per-scanline adaptive filter + literal-only dynamic Huffman blocks) and the host only wraps it.
// --framesCompression '"zips"' (exr only; default '"none"'): the frame leaves the device as finished OpenEXR ZIPS chunks (rfx_stage_exr, K8 behind
// the EXR byte predictor) and the host only wraps them; the samples are the uncompressed file's.  --framesMatches true (with either of the two;
// default false): the device encode with run-length matches (rfx.h "Match form"): smaller files where pixels repeat exactly.
// --env / --envCube (below, where they are read): scene.environment; --envCube with %d in the name: a cube per frame; --envOnDevice true: every
// change of the environment stays on the device (SSGIEffect's envOnDevice: rfx_set_environment_cube, rfx_build_environment_importance), same bytes.
// --saveState DIR [--saveEvery N]: write a checkpoint of the temporal state (js/state.js) into DIR after every N-th frame and after the last;
// --loadState DIR: restore one first — the dump directories given are then the REMAINING frames, and the outputs are byte-identical to an
// uninterrupted run.  Both work with --ranks (every rank writes its rows of the whole-frame planes; any rank count loads them), --traa,
// --motionBlur and --stream (the save waits for the frame boundary).  A checkpoint written by the Python host loads here, and the reverse.
const fs = require("fs")
const path = require("path")
const rfx = require("./index")

const args = process.argv.slice(2)
const dumps = []
const opt = {}
let out = "."
for (let i = 0; i < args.length; i++) {
	if (args[i] === "--out") out = args[++i]
	else if (args[i] === "--saveState" || args[i] === "--loadState" || args[i] === "--framesOut") {
		// a directory, plain or JSON-quoted like the other path options
		let v = args[i + 1]
		try { v = JSON.parse(v) } catch (e) { /* plain */ }
		opt[args[i++].slice(2)] = String(v)
	} else if (args[i].startsWith("--")) opt[args[i].slice(2)] = JSON.parse(args[++i])
	else dumps.push(args[i])
}
if (!dumps.length) {
	console.error("usage: run_dump.js <dumpdir>... --out <dir> [--steps N ...]")
	process.exit(2)
}
if (opt.framesOut !== undefined && opt.ranks > 1) throw new Error("--framesOut writes whole frames: not with --ranks (the image writers are whole-frame-only for every tiled run)")
// ---- row-tiled run: parent process
if (opt.ranks > 1 && opt.rank === undefined) {
	const cp = require("child_process")
	const os = require("os")
	fs.mkdirSync(out, { recursive: true })
	const idDir = fs.mkdtempSync(path.join(os.tmpdir(), "rfx-"))
	const idFile = path.join(idDir, "nccl_id")
	const cleanup = () => {
		try { fs.unlinkSync(idFile) } catch (e) { /* never written */ }
		try { for (const f of fs.readdirSync(idDir)) if (f.startsWith("nccl_id.peer")) fs.unlinkSync(path.join(idDir, f)) } catch (e) { /* not that mode */ }
		try { fs.rmdirSync(idDir) } catch (e) { /* not empty: leave it */ }
	}
	const kids = []
	for (let r = 0; r < opt.ranks; r++)
		kids.push(cp.spawn(process.execPath, [__filename].concat(args, ["--rank", String(r), "--idFile", JSON.stringify(idFile)]), { stdio: ["ignore", "pipe", "inherit"] }))
	let left = kids.length, failed = false
	const lines = new Array(kids.length).fill("")
	kids.forEach((k, r) => {
		k.stdout.on("data", d => (lines[r] += d))
		k.on("exit", code => {
			if (code !== 0 && !failed) {
				// a rank that dies before the communicator exists leaves the others waiting for it (ncclCommInitRank, the id file): stop them now
				failed = true
				console.error("rank " + r + " exited with code " + code + ": stopping the other ranks")
				kids.forEach((q, i) => { if (i !== r && q.exitCode === null) q.kill() })
			}
			if (--left) return
			cleanup()
			if (failed) process.exit(1)
			// stitch the row tiles (rank order = ascending rows)
			for (const name of ["final", "compose", "denoise_b0", "denoise_b1", "temporal0", "ssgi"].concat(opt.motionBlur ? ["motion_blur"] : [])) {
				const parts = kids.map((_, q) => fs.readFileSync(path.join(out, name + ".rank" + q + ".bin")))
				fs.writeFileSync(path.join(out, name + ".bin"), Buffer.concat(parts))
				kids.forEach((_, q) => fs.unlinkSync(path.join(out, name + ".rank" + q + ".bin")))
			}
			const info = lines.map(l => JSON.parse(l.trim().split("\n").pop()))
			console.log(JSON.stringify({ frames: dumps.length, width: info[0].width, height: info[0].height, ranks: opt.ranks, haloRows: info[0].haloRows,
				haloViolations: info.reduce((a, b) => a + b.haloViolations, 0), exchanges: info[0].exchanges }))
		})
	})
	return
}
const tiled = opt.ranks > 1 ? { rank: opt.rank, ranks: opt.ranks, idFile: opt.idFile, historyGather: opt.historyGather || "all" } : null
delete opt.historyGather
delete opt.ranks
delete opt.rank
delete opt.idFile
const stream = !!opt.stream
delete opt.stream
const images = { png: opt.png, exr: opt.exr, pfm: opt.pfm, tonemap: opt.tonemap, exposure: opt.exposure }
for (const k of Object.keys(images)) delete opt[k]
const framesOut = opt.framesOut === undefined ? null : { dir: String(opt.framesOut), format: opt.framesFormat || "png", encode: opt.framesEncode || "host", compression: opt.framesCompression || "none", matches: !!opt.framesMatches }
delete opt.framesOut
delete opt.framesFormat
delete opt.framesEncode
delete opt.framesCompression
delete opt.framesMatches
let frames = null
function openFrames() {
	if (!framesOut) return
	fs.mkdirSync(framesOut.dir, { recursive: true })
	frames = new rfx.FrameExporter(renderer, framesOut.dir, { format: framesOut.format, tonemap: images.tonemap, exposure: images.exposure, encode: framesOut.encode, compression: framesOut.compression, matches: framesOut.matches })
}
const checkpoint = { save: opt.saveState, every: opt.saveEvery, load: opt.loadState }
delete opt.saveState
delete opt.saveEvery
delete opt.loadState
// after frame n of this run (1-based): every --saveEvery-th frame and the last
function saveAfter(n, effects) {
	if (checkpoint.save && ((checkpoint.every && n % checkpoint.every === 0) || n === dumps.length)) rfx.saveState(checkpoint.save, renderer, effects)
}
const motionBlur = opt.motionBlur
const deltaTime = opt.deltaTime === undefined ? 1 / 60 : opt.deltaTime
delete opt.motionBlur
delete opt.deltaTime
// the blurred frame of the last step -> motion_blur.bin (and the images); a tile writes its own rows, the parent stitches them
function writeMotionBlur(mb) {
	const a = tiled ? mb.output(renderer, renderer.tileY0, renderer.tileRows) : mb.output(renderer)
	fs.writeFileSync(path.join(out, "motion_blur" + (tiled ? ".rank" + tiled.rank : "") + ".bin"), Buffer.from(a.buffer, a.byteOffset, a.byteLength))
	if (tiled) return
	if (images.exr) rfx.writeEXR(images.exr, a, first.width, first.height)
	if (images.pfm) rfx.writePFM(images.pfm, a, first.width, first.height)
	if (images.png) rfx.writePNG(images.png, rfx.tonemap(a, first.width, first.height, images.tonemap, images.exposure), first.width, first.height, 3)
}
const seeds = { ssgi: opt.ssgiSeed === undefined ? 11 : opt.ssgiSeed, denoise: opt.denoiseSeed === undefined ? 22 : opt.denoiseSeed }
delete opt.ssgiSeed
delete opt.denoiseSeed
// --aovConventions '{"depth_kind": "view_z", "velocity_kind": "scaled", "velocity_scale": [sx, sy], ...}': the unpacked dumps are in an engine's
// conventions (rfx.h "AOV conventions"; the record of rfx_amd.conventions.AovConventions.to_json, matrices optional: they come from each frame's
// cameras) — for directories whose frame.json does not say so itself.  Engine-form frames are converted on the device: --stream true.
const aovConventions = opt.aovConventions || null
delete opt.aovConventions
const readDump = d => {
	const f = rfx.readDump(d)
	if (aovConventions && !f.gbuffer) f.aovConventions = aovConventions
	return f
}
const first = readDump(dumps[0])
if (first.aovConventions && !(stream && !tiled)) throw new Error("engine-form AOV planes (aovConventions) are converted by the staged import: add --stream true")
const scene = { frame: first }
// --env <file.bin> --envWidth W --envHeight H [--envFlipY true]: a raw Float32 RGBA equirect map (row 0 = bottom) as scene.environment, a
// HalfFloatType texture; --envFlipY: its flipY is set (the importance tables are then built from the worker's "un-flipped" rows)
if (opt.env) {
	const b = fs.readFileSync(opt.env)
	scene.environment = { data: new Float32Array(b.buffer, b.byteOffset, b.length / 4), width: opt.envWidth, height: opt.envHeight }
	if (opt.envFlipY) scene.environment.flipY = true
	delete opt.env
	delete opt.envWidth
	delete opt.envHeight
}
delete opt.envFlipY
// --envCube <file.bin> --envCubeSize S [--envCubeMipmaps false]: scene.environment as a CubeTexture — six S x S Float32 RGBA faces (+X -X +Y -Y
// +Z -Z, row j = t as uploaded), converted once through CubeToEquirectEnvPass (three's default sampler state unless --envCubeMipmaps false:
// LinearFilter, no chain).  A name with %d names the file of frame index %d (0-based): every frame that has one gets a NEW scene.environment
// object, a frame without one keeps the environment it found — an environment that changes during the sequence (a re-rendered probe, an animated
// sky).  --envOnDevice true (SSGIEffect's envOnDevice): every change stays on the device (rfx_set_environment_cube, rfx_build_environment_importance)
let frameEnvironment = () => {}
if (opt.envCube) {
	const cubeName = String(opt.envCube), cubeSize = opt.envCubeSize, cubeMipmaps = opt.envCubeMipmaps
	const loadCube = file => {
		const b = fs.readFileSync(file)
		const cube = { isCubeTexture: true, faces: new Float32Array(b.buffer, b.byteOffset, b.length / 4), size: cubeSize }
		if (cubeMipmaps === false) Object.assign(cube, { minFilter: rfx.LinearFilter, generateMipmaps: false })
		return cube
	}
	if (cubeName.includes("%d")) {
		let held = null
		frameEnvironment = i => {
			const file = cubeName.replace("%d", String(i))
			if (file !== held && fs.existsSync(file)) {
				scene.environment = loadCube(file)
				held = file
			}
		}
	} else scene.environment = loadCube(cubeName)
	delete opt.envCube
	delete opt.envCubeSize
	delete opt.envCubeMipmaps
}
const camera = Object.assign({}, first.camera)
let renderer
if (tiled) {
	// halo: the K3 tap footprint, the largest vertical motion of the sequence and K1's source rows at --resolutionScale (rfx_amd/tiling.py required_halo)
	let vmax = 0
	for (const d of dumps) {
		const f = d === dumps[0] ? first : readDump(d)
		if (!f.velocity) throw new Error("--ranks needs packed velocity.bin dumps")
		const v = new Float32Array(f.velocity.buffer, f.velocity.byteOffset, f.velocity.length)
		for (let i = 1; i < v.length; i += 4) if (Math.abs(v[i]) > vmax) vmax = Math.abs(v[i])
	}
	const halo = rfx.requiredHalo(opt.radius === undefined ? 3 : opt.radius, vmax, first.height, first.width, opt.resolutionScale)
	const waitFor = (file, what) => {
		const t0 = Date.now()
		while (!fs.existsSync(file)) {
			if (Date.now() - t0 > 120000) throw new Error("rank " + tiled.rank + ": no " + what)
			Atomics.wait(new Int32Array(new SharedArrayBuffer(4)), 0, 0, 20)
		}
		return fs.readFileSync(file)
	}
	let id
	if (tiled.rank === 0) {
		id = rfx.commUniqueId()
		fs.writeFileSync(tiled.idFile + ".tmp", id)
		fs.renameSync(tiled.idFile + ".tmp", tiled.idFile)
	} else {
		id = waitFor(tiled.idFile, "ncclUniqueId from rank 0")
	}
	renderer = new rfx.TiledRenderer(first.width, first.height, tiled.rank, tiled.ranks, halo, id,
		{ device: process.env.RFX_ONE_GPU === "1" ? 0 : tiled.rank, historyGather: tiled.historyGather === "peer" ? "all" : tiled.historyGather })
	// --historyGather '"peer"': the ranks' export blobs (192 plain bytes each) travel once, through files next to the id file
	// (called again by a checkpoint, where the ranks only meet: every round has its own files)
	let round = 0
	if (tiled.historyGather === "peer")
		renderer.usePeerHistory(blob => {
			const base = tiled.idFile + ".peer" + (round ? "_" + round + "_" : "")
			round++
			fs.writeFileSync(base + tiled.rank + ".tmp", blob)
			fs.renameSync(base + tiled.rank + ".tmp", base + tiled.rank)
			const all = []
			for (let r = 0; r < tiled.ranks; r++) all.push(waitFor(base + r, "peer blob of rank " + r))
			return all
		})
} else renderer = new rfx.Renderer(first.width, first.height)
// --uvModel '"reference_gl"': every fragment sees the vUv the reference GL's rasteriser interpolates (rfx_set_uv_model) instead of (i + 0.5) / n
if (opt.uvModel) (renderer.inner || renderer).setUvModel(opt.uvModel)
if (opt.traa) {
	const half = opt.traa === "half"
	const velocityPass = new rfx.VelocityDepthNormalPass(scene, camera)
	const traa = new rfx.TRAAEffect(scene, camera, velocityPass, { fullAccumulate: true }, true)
	const mb = motionBlur ? new rfx.MotionBlurEffect(velocityPass, motionBlur, true) : null
	if (mb) mb.shareEffectPass(traa)
	const effects = mb ? [traa, mb] : [traa]
	if (checkpoint.load) rfx.loadState(checkpoint.load, renderer, effects)
	if (framesOut && !mb && framesOut.format === "exr") throw new Error("--framesOut with --traa alone: png or pfm (TRAA's alpha of 1 is written by the host's traa_compose)")
	openFrames()
	dumps.forEach((d, i) => {
		const f = d === dumps[0] ? first : readDump(d)
		scene.frame = f
		Object.assign(camera, f.camera)
		traa.update(renderer, { texture: { type: half ? rfx.HalfFloatType : rfx.FloatType }, width: f.width, height: f.height, data: rfx.floatPlane(f.direct, f.width * f.height, 4) })
		if (mb) {
			mb.update(renderer, null, deltaTime)
			mb.mainImage(renderer)
		}
		if (frames) {
			if (!mb && traa.uniforms.accumulatedTexture !== rfx.TEX.TEMPORAL0) throw new Error("--framesOut with --traa: the accumulated colour is not in TEX.TEMPORAL0")
			frames.submit(mb ? rfx.TEX.MOTION_BLUR : rfx.TEX.TEMPORAL0)
		}
		saveAfter(i + 1, effects)
	})
	if (frames) frames.finish()
	renderer.sync()
	fs.mkdirSync(out, { recursive: true })
	const a = traa.output(renderer)
	fs.writeFileSync(path.join(out, "traa.bin"), Buffer.from(a.buffer, a.byteOffset, a.byteLength))
	if (mb) writeMotionBlur(mb)
	console.log(JSON.stringify({ frames: dumps.length, width: first.width, height: first.height, haloViolations: renderer.haloViolations() }))
	process.exit(0)
}
const effect = new rfx.SSGIEffect(null, scene, camera, Object.assign({ width: first.width, height: first.height }, opt), seeds, true)
const mb = motionBlur ? new rfx.MotionBlurEffect(new rfx.VelocityDepthNormalPass(scene, camera), motionBlur, true) : null
// MotionBlurEffect in the pass after SSGIEffect: its input buffer is the effect's final image, on the device
function blurFrame() {
	if (!mb) return
	effect.mainImage(renderer)
	mb.update(renderer, rfx.TEX.FINAL, deltaTime)
	mb.mainImage(renderer)
}
// --framesOut: after the frame's draws the effect's own fragment (it writes TEX.FINAL only), then the staged export of what the frame shows
function exportFrame() {
	if (!frames) return
	if (!mb) effect.mainImage(renderer)
	frames.submit(mb ? rfx.TEX.MOTION_BLUR : rfx.TEX.FINAL)
}
const effects = mb ? [effect, mb] : [effect]
if (checkpoint.load) rfx.loadState(checkpoint.load, renderer, effects)
openFrames()
if (stream && !tiled) {
	// two alternating sets of pinned planes shaped like the first dump's: packed planes, or — an unpacked / typed dump — its attribute planes
	// as they are on disk (Float32Array, or Uint16Array of halves), which Renderer.stageFrame hands to rfx_stage_aov
	const pinned = a => rfx.Renderer.hostAlloc(a.constructor, a.length)
	const top = first.gbuffer ? ["depth", "gbuffer", "velocity", "direct"] : ["depth", "direct"]
	const sets = [0, 1].map(() => {
		const set = {}
		for (const k of top) set[k] = pinned(first[k])
		if (!first.gbuffer) {
			set.aov = {}
			for (const k of Object.keys(first.aov)) set.aov[k] = pinned(first.aov[k])
		}
		return set
	})
	const fill = (dst, src, what) => {
		if (!src || src.constructor !== dst.constructor || src.length !== dst.length) throw new Error("--stream: " + what + " differs in type or size from the first dump's")
		dst.set(src)
	}
	const load = (d, set) => { // disk -> pinned planes (a reader thread's job in a long run)
		const f = d === dumps[0] ? first : readDump(d)
		for (const k of top) fill(set[k], f[k], d + " " + k)
		if (set.aov) for (const k of Object.keys(set.aov)) fill(set.aov[k], f.aov && f.aov[k], d + " aov " + k)
		return Object.assign({}, f, set, { static: "resident" })
	}
	let cur = load(dumps[0], sets[0])
	renderer.stageFrame(cur)
	renderer.stageFlip()
	for (let i = 0; i < dumps.length; i++) {
		const next = i + 1 < dumps.length ? load(dumps[i + 1], sets[(i + 1) & 1]) : null
		if (next) renderer.stageFrame(next) // frame i+1 starts crossing PCIe ...
		scene.frame = cur
		Object.assign(camera, cur.camera)
		frameEnvironment(i)
		effect.update(renderer, null) // ... while frame i is drawn
		blurFrame()
		exportFrame() // (before the flip: the effect's fragment reads this frame's planes)
		renderer.stageFlip()
		saveAfter(i + 1, effects) // at the frame boundary: the save waits for the draws; the staged planes of frame i+1 are inputs, not state
		cur = next
	}
} else
	dumps.forEach((d, i) => {
		const f = d === dumps[0] ? first : readDump(d)
		scene.frame = f
		Object.assign(camera, f.camera)
		frameEnvironment(i)
		effect.update(renderer, null)
		blurFrame()
		exportFrame()
		saveAfter(i + 1, effects)
	})
if (frames) frames.finish()
renderer.sync()
fs.mkdirSync(out, { recursive: true })
const T = rfx.TEX
effect.mainImage(renderer) // the effect's own fragment -> final.bin
// --resolutionScale S < 1: ssgi.bin is the (W*S) x (H*S) target K1 drew, nothing else of the slot.  A tile holds the target rows
// ssgiTargetRows names from the start of its slot (include/rfx.h rfx_ssgi_target_rows) and contributes the ones whose nearest full-resolution
// row, floor((j + 0.5) * H / (H*S)), is one of its own: every target row exactly once, in rank order
const scale = opt.resolutionScale === undefined ? 1 : Number(opt.resolutionScale)
function scaledTarget() {
	const ws = Math.round(first.width * scale), hs = Math.round(first.height * scale)
	const held = (renderer.inner || renderer).ssgiTargetRows(scale)
	const y0 = tiled ? renderer.tileY0 : 0, y1 = tiled ? renderer.tileY0 + renderer.tileRows : first.height
	const owner = j => Math.min(first.height - 1, Math.floor(((j + 0.5) * first.height) / hs))
	let lo = 0
	while (lo < hs && owner(lo) < y0) lo++
	let hi = lo
	while (hi < hs && owner(hi) < y1) hi++
	if (hi > lo && (lo < held[0] || hi > held[0] + held[1])) throw new Error("target rows [" + lo + ", " + hi + ") are not all among the rows this tile drew")
	return renderer.download(T.SSGI).subarray((lo - held[0]) * ws * 4, (hi - held[0]) * ws * 4)
}
for (const [name, tex] of [["final", T.FINAL], ["compose", T.COMPOSE], ["denoise_b0", T.DENOISE_B0], ["denoise_b1", T.DENOISE_B1], ["temporal0", T.TEMPORAL0], ["ssgi", T.SSGI]]) {
	// a tile writes its own rows; the parent stitches them
	const a = tex === T.SSGI && scale !== 1 ? scaledTarget() : tiled ? renderer.download(tex, renderer.tileY0, renderer.tileRows) : renderer.download(tex)
	fs.writeFileSync(path.join(out, name + (tiled ? ".rank" + tiled.rank : "") + ".bin"), Buffer.from(a.buffer, a.byteOffset, a.byteLength))
}
if (mb) writeMotionBlur(mb)
else if (!tiled && (images.png || images.exr || images.pfm)) {
	const fin = renderer.download(T.FINAL)
	if (images.exr) rfx.writeEXR(images.exr, fin, first.width, first.height)
	if (images.pfm) rfx.writePFM(images.pfm, fin, first.width, first.height)
	if (images.png) rfx.writePNG(images.png, rfx.tonemap(fin, first.width, first.height, images.tonemap, images.exposure), first.width, first.height, 3)
}
console.log(JSON.stringify({ frames: dumps.length, width: first.width, height: first.height, haloViolations: renderer.haloViolations(),
	haloRows: tiled ? renderer.haloRows : 0, exchanges: tiled ? renderer.exchangeCount : 0 }))
