"""-m gpu: resolutionScale < 1 on row-tiled contexts.  A tile draws the rows of the smaller K1 target that K2's staging of the tile
addresses (rfx_ssgi_target_rows, rfx_launch.h rfx_scaled_rows) from the start of its RFX_TEX_SSGI; everything downstream must equal the
whole-frame context bit for bit: the chain through SSGIEffect, the split draw, the hit mask that bounds the history gathers, and the ring
of one on the real RCCL.  Before rfx_ssgi_target_rows existed the library refused every one of these draws with RFX_EUNSUPPORTED."""
import types

import numpy as np
import pytest

from test_gpu_parity import _LocalTiles, _params

pytestmark = pytest.mark.gpu

W, H, NF = 200, 132, 3  # tile boundaries 66 and 44 / 88: fractional target boundaries at 0.75 and 0.25, whole ones at 0.5
_frames, _whole = {}, {}


def frames(w=W, h=H):
    from rfx_amd.scene import synthetic_frame
    if (w, h) not in _frames:
        _frames[(w, h)] = [synthetic_frame(w, h, i) for i in range(NF)]
    return _frames[(w, h)]


def halo_for(s, w=W, h=H):
    from rfx_amd import tiling
    vmax = max(float(np.abs(f.velocity[..., 1].view(np.float32)).max()) for f in frames(w, h))
    return tiling.required_halo(3.0, vmax, h, w, resolution_scale=s)


def run_chain(renderer, s, extra, after_frame=None):
    from rfx_amd.effect import SSGIEffect
    scene = types.SimpleNamespace(frame=None)
    cam = types.SimpleNamespace(**vars(frames()[0].camera))
    fx = SSGIEffect(None, scene, cam, dict(width=W, height=H, steps=12, refineSteps=3, resolutionScale=s, **extra), seeds=dict(ssgi=3, denoise=4))
    for f in frames():
        scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        fx.update(renderer, None)
        if after_frame:
            after_frame(fx)


CHAIN_TEX = ("TEX_TEMPORAL0", "TEX_TEMPORAL1", "TEX_DENOISE_B0", "TEX_DENOISE_B1", "TEX_COMPOSE")


def whole_chain(s, uv, extra):
    """the whole-frame context's result of a configuration, computed once: the chain slots and the (W*s) x (H*s) K1 target"""
    from rfx_amd import abi
    from rfx_amd.context import Context
    key = (s, uv, tuple(sorted(extra.items())))
    if key not in _whole:
        ctx = Context(W, H)
        ctx.set_uv_model(uv)
        run_chain(ctx, s, extra)
        r0, target = ctx.download_ssgi_target(s)
        assert r0 == 0 and target.shape == (int(H * s), int(W * s), 4) and ctx.ssgi_target_rows(s) == (0, int(H * s))
        _whole[key] = dict({t: ctx.download(getattr(abi, t)) for t in CHAIN_TEX}, target=target)
        ctx.close()
    return _whole[key]


@pytest.mark.parametrize("s,ntiles,uv,extra", [
    (0.5, 2, "reference_gl", {}), (0.5, 3, "reference_gl", {}), (0.75, 2, "reference_gl", {}), (0.75, 3, "reference_gl", {}),
    (0.25, 2, "reference_gl", {}), (0.25, 3, "reference_gl", {}),
    (0.75, 3, "ideal", {}),  # the other vUv model: (i + 0.5) / n (the contexts' default is the reference GL's)
    (0.5, 3, "reference_gl", dict(denoiseMode="full_temporal")), (0.25, 2, "reference_gl", dict(mode="ssr"))])
def test_scaled_row_tiled_chain_is_bit_identical_to_the_whole_frame_context(s, ntiles, uv, extra):
    """SSGIEffect over 3 frames (the composed-GI feedback and K2's history are live) at resolutionScale s on 2 and 3 row tiles with
    required_halo(resolution_scale=s) rows of halo: every chain slot, gathered, and every tile's rows of the K1 target equal the whole-frame
    context's as bytes; no tile counts a halo violation."""
    from rfx_amd import abi
    want = whole_chain(s, uv, extra)
    tiled = _LocalTiles(W, H, ntiles, halo_for(s))
    for c in tiled.ctxs:
        c.set_uv_model(uv)
    run_chain(tiled, s, extra)
    for t in CHAIN_TEX:
        assert np.array_equal(tiled.gather(getattr(abi, t)).view(np.uint8), want[t].view(np.uint8)), t
    Hs = int(H * s)
    covered = np.zeros(Hs, bool)
    for c in tiled.ctxs:
        r0, rows = c.download_ssgi_target(s)
        assert 0 <= r0 and r0 + len(rows) <= Hs and len(rows) > 0
        assert np.array_equal(rows, want["target"][r0:r0 + len(rows)]), "target rows [%d, %d) of the tile at row %d" % (r0, r0 + len(rows), c.tile_y0)
        covered[r0:r0 + len(rows)] = True
        assert c.halo_violations() == 0
        c.close()
    assert covered.all() and (want["target"] != 0).any()


def test_scaled_row_tile_with_an_undersized_halo_counts_violations():
    """halo 2 at resolutionScale 0.25 on an interior tile: the tile draws target rows whose source rows (up to 2 rows beyond the +-2 rows K2
    stages) lie outside the held band.  Those G-buffer fetches go through rfx_xy_index -> rfx_local_row, which clamps the row into the band
    and counts it: nothing is read out of bounds, and the run is reported as wrong instead of being silently wrong."""
    from rfx_amd import abi
    from rfx_amd.context import Context
    f = frames()[1]
    sp, _, _, _ = _params(abi, f, f.camera, 1.0, 12, 3)
    sp.resolutionScale, sp.blueNoiseIndex = 0.25, 5
    ctx = Context(W, H, tile_y0=44, tile_rows=44, halo_rows=2)
    ctx.upload_frame(f)
    ctx.upload(abi.TEX_COMPOSE, np.zeros((H, W, 4), np.float32))
    ctx.ssgi_march(sp)
    assert ctx.halo_violations() > 0
    ctx.close()
    ok = Context(W, H, tile_y0=44, tile_rows=44, halo_rows=halo_for(0.25))
    ok.upload_frame(f)
    ok.upload(abi.TEX_COMPOSE, np.zeros((H, W, 4), np.float32))
    ok.ssgi_march(sp)
    assert ok.halo_violations() == 0
    ok.close()


def test_scaled_row_tiled_env_importance_sampling_at_an_odd_target_size_is_bit_identical():
    """202 x 134 at 0.5: a 101 x 67 target, whose last column and row have quad partners OUTSIDE the target (the implicit-lod fetch of the MIS
    specialisation takes them from coordinates, never from a drawn neighbour) — on 3 tiles, also for the first and last target row a tile draws."""
    from rfx_amd import abi
    from rfx_amd.context import Context
    from rfx_amd.envmap import build_importance
    from rfx_amd.scene import synthetic_environment, synthetic_frame

    w, h, s = 202, 134, 0.5
    env = synthetic_environment(64, 32)
    imp = build_importance(env.astype(np.float16).astype(np.float32), False)
    f = synthetic_frame(w, h, 1)
    comp = np.random.RandomState(1).rand(h, w, 4).astype(np.float32)
    sp, _, _, _ = _params(abi, f, f.camera, 1.0, 12, 3)
    sp.useEnvMap, sp.importanceSampling, sp.envBlur, sp.blueNoiseIndex, sp.resolutionScale = 1, 1, 0.5, 77, s

    def run(ctx):
        ctx.set_environment(env, half_float_type=True, half_store_rtz=True)
        ctx.set_environment_importance(*imp)
        ctx.upload_frame(f)
        ctx.upload(abi.TEX_COMPOSE, comp)
        ctx.ssgi_march(sp)
        return ctx.download_ssgi_target(s)
    whole = Context(w, h)
    _, ref = run(whole)
    whole.close()
    assert ref.shape == (67, 101, 4) and (ref[:, -1] != 0).any() and (ref[-1] != 0).any()
    halo = halo_for(s, w, h)
    seen_odd_first = seen_odd_last = False
    for r in range(3):
        y0, rows = Context.split_rows(h, 3, r)
        c = Context(w, h, tile_y0=y0, tile_rows=rows, halo_rows=halo)
        r0, got = run(c)
        assert np.array_equal(got, ref[r0:r0 + len(got)]), r
        assert c.halo_violations() == 0
        seen_odd_first |= bool(r0 & 1)                       # the first drawn row is the LOWER row of its quad: its partner row is not drawn
        seen_odd_last |= bool((r0 + len(got) - 1) & 1) == 0  # the last drawn row is the UPPER row of its quad
        c.close()
    assert seen_odd_first or seen_odd_last  # some tile draws half a quad


@pytest.mark.parametrize("s", [0.5, 0.75])
@pytest.mark.parametrize("missed", [0, 1])
def test_scaled_tile_hit_mask_bounds_what_the_shade_reads(s, missed):
    """The split draw and the bounded gather on scaled tiles: after rfx_ssgi_trace, rfx_ssgi_hit_mask names the full-resolution history rows
    and column blocks the shade of the tile's target rows reads.  The composed GI is NaN everywhere else; the shade must not notice (a missed
    texel shows as NaN): the tile's target rows equal the whole-frame context's as bytes, with missedRays on and off; trace + shade == march on
    the tile; and the tiles' masks OR together to the whole-frame context's mask."""
    from rfx_amd import abi, tiling
    from rfx_amd.context import Context
    f = frames()[1]
    sp, _, _, _ = _params(abi, f, f.prev_camera, 1.0, 12, 3, missed=missed)
    sp.blueNoiseIndex, sp.resolutionScale = 4242, s
    hist = np.random.RandomState(3).rand(H, W, 4).astype(np.float32) * 3.0
    blocks = (np.arange(W, dtype=np.int64) * 32) // W

    whole = Context(W, H)
    whole.upload_frame(f)
    whole.upload(abi.TEX_COMPOSE, hist)
    whole.ssgi_march(sp)
    _, want = whole.download_ssgi_target(s)
    whole.ssgi_trace(sp)
    whole_mask = whole.ssgi_hit_mask()
    lo, hi = whole.ssgi_hit_rows()
    used = np.flatnonzero(whole_mask)
    assert used.size and (lo, hi) == (used[0], used[-1])
    whole.ssgi_shade(sp)
    assert np.array_equal(whole.download_ssgi_target(s)[1], want)
    whole.close()

    halo = halo_for(s)
    union = np.zeros(H, np.uint32)
    seen_sparse = False
    for y0, rows in tiling.split_rows(H, 3):
        c = Context(W, H, tile_y0=y0, tile_rows=rows, halo_rows=halo)
        c.upload_frame(f)
        c.upload(abi.TEX_COMPOSE, hist)
        c.ssgi_march(sp)
        r0, fused = c.download_ssgi_target(s)
        assert np.array_equal(fused, want[r0:r0 + len(fused)])
        c.clear(abi.TEX_SSGI)
        c.upload(abi.TEX_COMPOSE, np.full((H, W, 4), 1e6, np.float32))  # the gather still in flight: the trace must not look at it
        c.ssgi_trace(sp)
        mask = c.ssgi_hit_mask()
        union |= mask
        needed = ((mask[:, None] >> blocks[None, :].astype(np.uint32)) & 1).astype(bool)  # (H, W): the texel's block bit
        seen_sparse |= bool(needed.mean() < 0.9)
        bad = hist.copy()
        bad[~needed] = np.nan
        c.upload(abi.TEX_COMPOSE, bad)  # between trace and shade: exactly where the bounded gather delivers the named texels
        c.ssgi_shade(sp)
        r1, got = c.download_ssgi_target(s)
        assert r1 == r0 and np.array_equal(got, fused), "tile rows [%d, %d): trace + shade != march, or the shade read a history texel whose mask bit is clear" % (y0, y0 + rows)
        assert c.halo_violations() == 0
        c.close()
    assert np.array_equal(union, whole_mask)
    assert seen_sparse  # (vacuous if every mask named the whole frame)


def test_scaled_checkpoints_are_independent_of_the_row_tiling(tmp_path):
    """A run at resolutionScale 0.5 saves and loads like any other (the K1 target is not state: every frame redraws it): saved whole-frame
    after 3 frames and resumed on 3 row tiles, and the reverse — the same checkpoint files, the same frames afterwards, no halo violation."""
    import os
    from rfx_amd import abi, state
    from rfx_amd.context import Context
    from test_gpu_state import K, Run, _frames, _local_tiles
    s = 0.5
    from rfx_amd import tiling
    from test_gpu_state import H as SH, W as SW
    fr = _frames(K + 2)
    halo = tiling.required_halo(3.0, max(float(np.abs(f.velocity[..., 1].view(np.float32)).max()) for f in fr), SH, SW, resolution_scale=s)  # the frames this test runs, that file's frame
    case = ("ssgi", dict(resolutionScale=s), False, False)
    stages = (abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1, abi.TEX_DENOISE_B0, abi.TEX_DENOISE_B1, abi.TEX_COMPOSE)

    def gathered(run):
        return {abi.TEX_NAMES[t]: run.r.download(t).tobytes() for t in stages}
    single = Context(SW, SH)
    straight = Run(case, single, seeds=dict(ssgi=3, denoise=4)).frames(fr[:K], record=False)
    whole_dir, tiled_dir = str(tmp_path / "whole"), str(tmp_path / "tiled")
    whole_header = state.save_state(whole_dir, single, straight.effects)
    straight.frames(fr[K:], record=False)
    want = gathered(straight)
    single.close()
    tiles = _local_tiles(3, halo)
    resumed = Run(case, tiles)._build(fr[K].camera)
    state.load_state(whole_dir, tiles, resumed.effects)
    resumed.frames(fr[K:], record=False)
    assert gathered(resumed) == want and all(c.halo_violations() == 0 for c in tiles.ctxs)
    tiles.close()
    tiles = _local_tiles(3, halo)
    first = Run(case, tiles, seeds=dict(ssgi=3, denoise=4)).frames(fr[:K], record=False)
    tiled_header = state.save_state(tiled_dir, tiles, first.effects)
    tiles.close()
    assert tiled_header == whole_header
    for p in whole_header["planes"]:
        assert open(os.path.join(whole_dir, p["file"]), "rb").read() == open(os.path.join(tiled_dir, p["file"]), "rb").read(), p["slot"]


def test_scaled_peer_pull_delivers_what_the_shade_reads():
    """rfx_peer_gather_history after a SCALED trace, both ranks in one process (one host thread per context): each tile's plane of the RGB history
    holds its own rows and NaN elsewhere; the pull brings the column blocks the scaled hit mask names out of the other tile's plane, and the shade
    then leaves the whole-frame context's target rows, bit for bit.  A second pull reports that no rank missed the first one's barrier.  On the
    device this runs like its unscaled twin, test_peer_history_gather_between_two_contexts_of_one_process: in a fresh interpreter with 8
    hardware queues, so that the two contexts' barrier kernels are resident together, with the twin's one reported second attempt."""
    import os
    import threading
    if os.environ.get("RFX_HOSTSIM") != "1" and int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 8:
        import subprocess
        import sys
        me = "%s::test_scaled_peer_pull_delivers_what_the_shade_reads" % os.path.abspath(__file__)
        for attempt in (1, 2):
            r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", me], env=dict(os.environ, GPU_MAX_HW_QUEUES="8"),
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            if r.returncode == 0 or attempt == 2 or "did not reach the previous call's barrier" not in r.stdout:
                break
            print("NOTE: the two contexts' barrier kernels were not resident together (hardware queue scheduling); second attempt")
        assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-4000:]
        return
    from rfx_amd import abi
    from rfx_amd.context import Context
    s = 0.5
    f = frames()[1]
    sp, _, _, _ = _params(abi, f, f.prev_camera, 1.0, 12, 3)
    sp.blueNoiseIndex, sp.historySource, sp.resolutionScale = 4242, 3, s
    hist = (np.random.RandomState(3).rand(H, W, 3) * 3.0).astype(np.float32)
    whole = Context(W, H)
    whole.upload_frame(f)
    whole.upload(abi.TEX_COMPOSE_RGB, hist)
    whole.ssgi_march(sp)
    _, want = whole.download_ssgi_target(s)
    whole.close()
    tiles = [Context.split_rows(H, 2, r) for r in range(2)]
    ctxs = [Context(W, H, tile_y0=y0, tile_rows=rows, halo_rows=halo_for(s)) for y0, rows in tiles]
    blobs = [c.peer_export(abi.TEX_COMPOSE_RGB) for c in ctxs]
    for r, c in enumerate(ctxs):
        c.peer_open(abi.TEX_COMPOSE_RGB, blobs, r, 2)
        plane = np.full((H, W, 3), np.nan, np.float32)
        y0, rows = tiles[r]
        plane[y0:y0 + rows] = hist[y0:y0 + rows]
        c.upload_frame(f)
        c.upload(abi.TEX_COMPOSE_RGB, plane)

    def on_both(fn):  # fn(rank) on one thread per context; the results in rank order
        out, errs = [None, None], []

        def run(r):
            try:
                out[r] = fn(r)
            except BaseException as e:  # noqa: BLE001 (re-raised below)
                errs.append(e)
        ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errs:
            raise errs[0]
        return out

    def pull(r):  # every rank issues the calls; neither waits on the host before the pull is enqueued
        ctxs[r].ssgi_trace(sp)
        return ctxs[r].peer_gather_history(abi.TEX_COMPOSE_RGB)
    assert on_both(pull) == [0, 0]  # (what the PREVIOUS call pulled: there was none)
    got, pulled = [], []
    for r, c in enumerate(ctxs):
        c.comm_wait()
        c.ssgi_shade(sp)
        c.sync()
        oy0, orows = tiles[1 - r]
        pulled.append(int(np.isfinite(c.download(abi.TEX_COMPOSE_RGB)[oy0:oy0 + orows]).all(-1).sum()))
        got.append(c.download_ssgi_target(s))
    assert on_both(pull) == [p * 12 for p in pulled]  # the next call reports the previous one's bytes, and raises if a peer missed its barrier
    assert sum(pulled) > 0  # (vacuous otherwise: reflections do cross the tile boundary)
    for r, c in enumerate(ctxs):
        c.comm_wait()
        c.sync()
        r0, rows = got[r]
        assert np.array_equal(rows, want[r0:r0 + len(rows)]), "rank %d: the shade read a history texel the pull did not deliver" % r
        assert c.halo_violations() == 0
        c.peer_close()
        c.close()


def test_scaled_bounded_gather_on_a_ring_of_one():
    """CommTiledRenderer(history_gather="bounded") on a ring of one over the real RCCL at resolutionScale 0.5: the frames equal a plain
    context's, and after every frame the bounded form itself runs with a SCALED trace pending — the device reduction of the scaled hit mask,
    the all-gather of the one mask with its host-side wait, no row travels on a ring of one, then the shade: the frame's K1 target again."""
    import os
    if os.environ.get("RFX_HOSTSIM") == "1":
        pytest.skip("--hostsim: the multi-process run over the stand-in library covers the exchange")
    from rfx_amd import abi, tiling
    from rfx_amd.context import Context
    s = 0.5
    want = whole_chain(s, "reference_gl", {})
    ctx = Context(W, H)
    r = tiling.CommTiledRenderer(ctx, 0, 1, Context.comm_unique_id(), history_gather="bounded")

    plain = Context(W, H)  # the same chain on a plain context, re-shaded the same way after every frame: what the bounded form must leave

    def reshade(c, sp, bounded):
        c.ssgi_trace(sp)
        if bounded:
            assert c.ssgi_hit_mask().any()
            c.ssgi_trace(sp)
            assert c.gather_history_rows(abi.TEX_COMPOSE) == 0  # a ring of one: nothing travels
            c.comm_wait()
        c.ssgi_shade(sp)
        return c.download_ssgi_target(s)[1]  # (K4 has replaced the composed GI since the frame's own K1: not the frame's target any more)
    reshaded = []
    run_chain(plain, s, {}, lambda fx: reshaded.append(reshade(plain, fx.ssgiPass.uniforms, False)))
    plain.close()
    frame_no = [0]

    def bounded_again(fx):
        got = reshade(ctx, fx.ssgiPass.uniforms, True)
        assert np.array_equal(got, reshaded[frame_no[0]]) and (got != 0).any(), "frame %d" % frame_no[0]
        frame_no[0] += 1
    run_chain(r, s, {}, bounded_again)
    for t in CHAIN_TEX:
        assert np.array_equal(r.download(getattr(abi, t)).view(np.uint8), want[t].view(np.uint8)), t
    ctx.comm_destroy()
    ctx.close()
