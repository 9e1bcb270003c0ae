"""-m gpu: K3's foreground map.  K1's depth pre-pass writes one byte per frame-aligned 64 x 8-texel tile (0 = every depth
texel of the tile is 1.0) and a K3 workgroup whose tile's byte is 0 returns before it stages anything.  The map may only ever skip work whose
result is "every pixel discards", so every stage output must be BYTE-identical to a run that never uses the map — the same library on a
context whose depth plane is bound with rfx_bind_external — whatever the targets held before (they are pre-filled with a sentinel pattern: a
discarded texel keeps it).  The K3 outputs are also held against the C restatement on the same inputs, with the metric and the bound of
tests/test_gpu_parity.py.

The frames are small (the cases also run thread by thread under --hostsim): 128 x 16 = 2 x 2 map tiles, 97 x 55 = partial tiles at the
right and top edges.  At 128 x 16 the aspect is 8 and the taps reach 24 texels sideways: no tiled pitch fits and both K3 passes draw k3_generic; the
same cases therefore also run at 128 x 72, where both passes draw k3_tiled — the kernel whose early return the production frame runs
(K3_KERNELS below, asserted through tests/specialisations.py from the plans of the loaded library)."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.quick]

STEPS, REFINE = 8, 2
# the frames of the one-tile cases and the K3 kernel both passes draw there; the carved tile is rows 8-16 x columns 0-64 at either size
SIZES = [(128, 16), (128, 72)]
K3_KERNELS = {(128, 16): "k3_generic", (128, 72): "k3_tiled"}
ONE = np.float32(1.0).view(np.uint32)


def _abi():
    from rfx_amd import abi
    return abi


def _targets():
    abi = _abi()
    return (abi.TEX_SSGI, abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1, abi.TEX_DENOISE_A0, abi.TEX_DENOISE_A1, abi.TEX_DENOISE_B0, abi.TEX_DENOISE_B1,
            abi.TEX_COMPOSE)


_GROUND = {}


def ground_frame(W, H, fi=0):
    """An all-foreground W x H frame: the lowest rows of a taller synthetic frame, which show the ground plane and what stands on it (the
    camera belongs to the taller frame: the kernels and the restatement are functions of the planes and the matrices, whatever they show)."""
    from rfx_amd.scene import Frame, synthetic_frame
    key = (W, H, fi)
    if key not in _GROUND:
        f = synthetic_frame(W, 4 * H, fi)
        assert (f.depth[:H] != 1.0).all(), "the cropped rows were meant to hold no background"
        _GROUND[key] = Frame(W, H, f.depth[:H].copy(), f.gbuffer[:H].copy(), f.velocity[:H].copy(), f.direct[:H].copy(), f.camera, f.prev_camera, fi)
    g = _GROUND[key]  # (shared: every test carves a copy)
    return Frame(W, H, g.depth.copy(), g.gbuffer.copy(), g.velocity.copy(), g.direct.copy(), g.camera, g.prev_camera, fi)


def carve(f, ys, xs):
    """background in rows ys x columns xs (slices): depth 1.0 in the depth plane and in the velocity texel's .w, as a G-buffer pass clears them"""
    f.depth[ys, xs] = 1.0
    f.velocity[ys, xs, 3] = ONE
    return f


def sentinel(W, H, seed=11):
    """what every target holds before the first draw: finite, different in every texel"""
    abi = _abi()
    rs = np.random.RandomState(seed)
    s = {}
    for t in _targets():
        if t in (abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1, abi.TEX_COMPOSE):
            s[t] = (rs.rand(H, W, 4) * 2).astype(np.float32)
        else:  # half-stored targets; K1's packed texel is eight halfs
            n = 8 if t == abi.TEX_SSGI else 4
            s[t] = (rs.rand(H, W, n) * 3).astype(np.float16).view(np.uint32 if t == abi.TEX_SSGI else np.uint16)
    return s


class NoMap:
    """A context whose depth plane lives in a caller's buffer (rfx_bind_external): the library never trusts a map of it.  The buffer is the
    depth slot of a second context, which exists only to own device memory."""

    def __init__(self, W, H, **kw):
        from rfx_amd.context import Context
        abi = _abi()
        self.holder = Context(W, H)
        self.ctx = Context(W, H, **kw)
        self.ctx.bind_external(abi.TEX_DEPTH, self.holder.device_ptr(abi.TEX_DEPTH))

    def upload_frame(self, f):
        abi = _abi()
        self.holder.upload(abi.TEX_DEPTH, f.depth)
        for tex, plane in ((abi.TEX_GBUFFER, f.gbuffer), (abi.TEX_VELOCITY, f.velocity), (abi.TEX_DIRECT_LIGHT, f.direct)):
            r0, n = self.ctx.held_rows(tex)
            self.ctx.upload(tex, plane[r0:r0 + n], r0, n)

    def close(self):
        self.ctx.close()
        self.holder.close()


class WithMap:
    def __init__(self, W, H):
        from rfx_amd.context import Context
        self.ctx = Context(W, H)

    def upload_frame(self, f):
        self.ctx.upload_frame(f)

    def close(self):
        self.ctx.close()


def params(f, prev_cam, keep, fi=0):
    from test_gpu_parity import _params
    sp, tp, dp, cp = _params(_abi(), f, prev_cam, keep, STEPS, REFINE)
    sp.blueNoiseIndex = 1000 + fi
    return sp, tp, dp, cp


def k3_pass(ctx, dp, fi, i):
    dp.blueNoiseIndex, dp.inputIsTemporal, dp.writeToB = 2000 + 2 * fi + i, (1, 0)[i], i
    ctx.poisson_denoise(dp)


def draw_frame(ctx, f, prev_cam, keep, fi=0):
    """K1 -> K2 -> one denoise iteration (K3 pass 0: temporal -> A, pass 1: A -> B) -> K4, planes already uploaded"""
    sp, tp, dp, cp = params(f, prev_cam, keep, fi)
    ctx.ssgi_march(sp)
    ctx.temporal_reproject(tp)
    k3_pass(ctx, dp, fi, 0)
    k3_pass(ctx, dp, fi, 1)
    ctx.compose(cp)


def fill(ctx, sent):
    for t, a in sent.items():
        r0, n = ctx.held_rows(t)
        ctx.upload(t, a[r0:r0 + n], r0, n)


def snapshot(ctx):
    return {t: ctx.download(t) for t in _targets()}


def assert_same(got, want, what):
    abi = _abi()
    for t in want:
        g, w = np.ascontiguousarray(got[t]).view(np.uint8), np.ascontiguousarray(want[t]).view(np.uint8)
        if not np.array_equal(g, w):
            ys, xs = np.nonzero((g != w).reshape(g.shape[0], g.shape[1], -1).any(-1))
            raise AssertionError("%s: %s differs from the run without a map in %d texels, first (y, x) = (%d, %d)" % (what, abi.TEX_NAMES[t], ys.size, ys[0], xs[0]))


def check_k3_against_restatement(what, f, blue, sent, out, fi=0):
    """both K3 passes of `out` (a snapshot after draw_frame from the sentinel state) against the C restatement fed the device's own inputs"""
    import rfx_oracle as O
    from test_gpu_parity import FLIP, assert_close
    abi = _abi()
    h8 = lambda o: O.half_bits_to_float(np.ascontiguousarray(o).view(np.uint16))  # noqa: E731
    _, _, dp, _ = params(f, f.camera, 0.0, fi)
    T = [out[abi.TEX_TEMPORAL0], out[abi.TEX_TEMPORAL1]]

    def run(ins, init, i):
        dp.blueNoiseIndex, dp.inputIsTemporal, dp.writeToB = 2000 + 2 * fi + i, (1, 0)[i], i
        outs = [a.copy() for a in init]
        O.denoise(f.depth, f.gbuffer, ins[0], ins[1], blue, dp, outs[0], outs[1])
        return outs

    A0 = [sent[abi.TEX_DENOISE_A0], sent[abi.TEX_DENOISE_A1]]
    A = [out[abi.TEX_DENOISE_A0], out[abi.TEX_DENOISE_A1]]
    B0 = [sent[abi.TEX_DENOISE_B0], sent[abi.TEX_DENOISE_B1]]
    B = [out[abi.TEX_DENOISE_B0], out[abi.TEX_DENOISE_B1]]
    wantA, wantB = run(T, A0, 0), run(A, B0, 1)
    for j in range(2):
        assert_close("%s K3 pass 0 [%d]" % (what, j), h8(A[j]), h8(wantA[j]), FLIP["denoise"], prove=lambda j=j: h8(run(T, A0, 0)[j]))
        assert_close("%s K3 pass 1 [%d]" % (what, j), h8(B[j]), h8(wantB[j]), FLIP["denoise"], prove=lambda j=j: h8(run(A, B0, 1)[j]))
        # a discarded texel keeps the sentinel: the restatement and the kernel agree on WHICH texels those are
        for g, w, s in ((A[j], wantA[j], A0[j]), (B[j], wantB[j], B0[j])):
            assert np.array_equal((g == s).all(-1), (w == s).all(-1)), "%s: the set of discarded texels differs from the restatement's" % what


def assert_k3_kernels(W, H):
    """both K3 passes of draw_frame on a whole-frame W x H context select the kernel K3_KERNELS names"""
    import specialisations as SP
    abi = _abi()
    plans = SP.Plans(abi.load_library())
    f = ground_frame(W, H)
    _, _, dp, _ = params(f, f.camera, 0.0)
    for i in range(2):
        dp.inputIsTemporal, dp.writeToB = (1, 0)[i], i
        key = SP.k3_key(plans, dp, W, H, whole=True)
        assert key[:3] == (K3_KERNELS[(W, H)], (1, 0)[i], 2), key
        assert key[0] == "k3_generic" or key[4] == 1


def one_frame(cls, f, sent, **kw):
    r = cls(f.width, f.height, **kw)
    fill(r.ctx, sent)
    r.upload_frame(f)
    draw_frame(r.ctx, f, f.camera, 0.0)
    out = snapshot(r.ctx)
    assert r.ctx.halo_violations() == 0
    r.close()
    return out


def _variant(name, W, H):
    f = ground_frame(W, H)
    if name == "background_tile":
        carve(f, slice(8, 16), slice(0, 64))
    elif name == "corner_pixel":  # all background except the pixel in the tile's last corner
        carve(f, slice(8, 16), slice(0, 64))
        g = ground_frame(W, H)
        for a, b in ((f.depth, g.depth), (f.velocity, g.velocity)):
            a[15, 63] = b[15, 63]
    elif name == "nan_texel":  # depth NaN != 1.0: the pixel is not discarded, the tile must be processed
        carve(f, slice(8, 16), slice(0, 64))
        f.depth[11, 30] = np.float32(np.nan)
    else:
        assert name == "all_foreground"
    return f


# (the 128 x 16 cases keep the ids they had before the second size existed)
@pytest.mark.parametrize("name,W,H", [pytest.param(n, W, H, id=n if (W, H) == SIZES[0] else "%s-%dx%d" % (n, W, H))
                                      for W, H in SIZES for n in ("background_tile", "corner_pixel", "nan_texel", "all_foreground")])
def test_one_tile_variants(blue_noise, name, W, H):
    assert_k3_kernels(W, H)
    f, sent = _variant(name, W, H), sentinel(W, H)
    got, want = one_frame(WithMap, f, sent), one_frame(NoMap, f, sent)
    assert_same(got, want, name)
    abi = _abi()
    kept = (got[abi.TEX_DENOISE_A0] == sent[abi.TEX_DENOISE_A0]).all(-1)
    if name == "background_tile":
        assert kept[8:16, 0:64].all() and not kept[0:8].any() and not kept[:, 64:].any()
    if name == "corner_pixel":
        assert not kept[15, 63] and kept[8:14, 0:62].all()
    if name == "nan_texel":
        assert not kept[11, 30], "the NaN-depth pixel takes no discard: its tile may not be skipped"
    if name == "all_foreground":
        assert not kept.any()
    if name != "nan_texel":  # (the metric compares finite values)
        check_k3_against_restatement(name, f, blue_noise, sent, got)


def test_partial_edge_tiles(blue_noise):
    """97 x 55: the tile column at x = 64 is 33 texels wide, the tile row at y = 48 is 7 rows high.  The top partial row is all background (its map
    bytes come from the 7 rows that exist), the right partial column is mixed"""
    W, H = 97, 55
    f = ground_frame(W, H)
    carve(f, slice(48, 55), slice(0, W))
    carve(f, slice(16, 24), slice(64, W))   # a whole partial tile of the right column
    carve(f, slice(24, 32), slice(70, W))   # ... one that keeps six foreground columns
    carve(f, slice(3, 13), slice(80, 90))   # ... and a patch across a tile boundary
    sent = sentinel(W, H)
    got, want = one_frame(WithMap, f, sent), one_frame(NoMap, f, sent)
    assert_same(got, want, "partial tiles")
    abi = _abi()
    kept = (got[abi.TEX_DENOISE_B0] == sent[abi.TEX_DENOISE_B0]).all(-1)
    assert kept[48:55].all() and kept[16:24, 64:].all() and not kept[24:32, 64:70].any()
    check_k3_against_restatement("partial tiles", f, blue_noise, sent, got)


@pytest.mark.parametrize("W,H", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_stale_map_is_not_used(blue_noise, W, H):
    """the map describes the depth plane of the last K1 pre-pass: after rfx_upload of another plane (foreground where there was background) a
    K3 draw without a new K1 draw must process those tiles"""
    assert_k3_kernels(W, H)
    abi = _abi()
    f0, f1 = carve(ground_frame(W, H), slice(8, 16), slice(0, 64)), carve(ground_frame(W, H), slice(0, 8), slice(64, 128))
    sent = sentinel(W, H)
    outs = []
    for cls in (WithMap, NoMap):
        r = cls(W, H)
        fill(r.ctx, sent)
        r.upload_frame(f0)
        draw_frame(r.ctx, f0, f0.camera, 0.0)
        fill(r.ctx, sent)
        r.upload_frame(f1)
        _, _, dp, _ = params(f1, f1.camera, 0.0)
        k3_pass(r.ctx, dp, 0, 0)
        k3_pass(r.ctx, dp, 0, 1)
        outs.append(snapshot(r.ctx))
        r.close()
    assert_same(outs[0], outs[1], "stale map")
    kept = (outs[0][abi.TEX_DENOISE_A0] == sent[abi.TEX_DENOISE_A0]).all(-1)
    assert not kept[8:16, 0:64].any(), "the tile that was background under the old depth plane was skipped"
    assert kept[0:8, 64:128].all()
    check_k3_against_restatement("stale map", f1, blue_noise, sent, outs[0])


@pytest.mark.parametrize("W,H", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_three_queued_frames_with_a_moving_background(W, H):
    """three frames queued without a synchronisation in between (staged uploads: no entry point waits for the draws): the pre-pass of frame
    n + 1 runs under frame n's K3 draws and must not touch the map they read"""
    assert_k3_kernels(W, H)
    abi = _abi()
    frames = [carve(ground_frame(W, H, 0), slice(8, 16), slice(0, 64)), carve(ground_frame(W, H, 1), slice(0, 8), slice(0, 128)),
              carve(ground_frame(W, H, 2), slice(8, 16), slice(64, 128))]
    sent = sentinel(W, H)
    inputs = ((abi.TEX_GBUFFER, "gbuffer"), (abi.TEX_VELOCITY, "velocity"), (abi.TEX_DIRECT_LIGHT, "direct"))

    def run(with_map):
        from rfx_amd.context import Context
        ctx = Context(W, H)
        holders = []
        if not with_map:  # one caller-owned depth plane per frame, all filled before the first draw
            for f in frames:
                h = Context(W, H)
                h.upload(abi.TEX_DEPTH, f.depth)
                holders.append(h)
        fill(ctx, sent)
        ctx.sync()
        prev, keep = frames[0].camera, 0.0
        for fi, f in enumerate(frames):
            for tex, name in inputs + (((abi.TEX_DEPTH, "depth"),) if with_map else ()):
                ctx.stage_upload(tex, getattr(f, name))
            ctx.stage_flip()
            if not with_map:
                ctx.bind_external(abi.TEX_DEPTH, holders[fi].device_ptr(abi.TEX_DEPTH))
            draw_frame(ctx, f, prev, keep, fi)
            prev, keep = f.camera, 1.0
        ctx.sync()
        out = snapshot(ctx)
        assert ctx.halo_violations() == 0
        ctx.close()
        for h in holders:
            h.close()
        return out

    got, want = run(True), run(False)
    assert_same(got, want, "three queued frames")
    # frame 2 wrote rows 0..7 everywhere and rows 8..15 of the left half; the right half of rows 8..15 still holds frame 1's texels
    assert not (got[abi.TEX_DENOISE_B0] == sent[abi.TEX_DENOISE_B0]).all(-1).any()


def test_row_window_and_row_tiles_bypass_the_map(blue_noise):
    """a launch whose first row is no multiple of 8 has another tile grid than the map, and a row-tiled context holds bands, not the frame: both
    draw without the map and leave what the whole-frame draw leaves"""
    from rfx_amd import tiling
    from test_gpu_parity import _LocalTiles
    abi = _abi()
    W, H = 128, 48
    # rows 0..7 of the left tile column are background, rows 8..15 are not: a windowed launch from row 4 that indexed the map with ITS tile rows
    # (4..11 -> map row 0) would skip rows 8..11; likewise the second row tile (from row 24) against map rows 0..2
    f = carve(carve(ground_frame(W, H), slice(0, 8), slice(0, 64)), slice(40, 48), slice(64, 128))
    sent = sentinel(W, H)
    want = one_frame(WithMap, f, sent)
    assert_same(want, one_frame(NoMap, f, sent), "whole frame")

    r = WithMap(W, H)
    fill(r.ctx, sent)
    r.upload_frame(f)
    sp, tp, dp, cp = params(f, f.camera, 0.0)
    draws = (lambda: r.ctx.ssgi_march(sp), lambda: r.ctx.temporal_reproject(tp), lambda: k3_pass(r.ctx, dp, 0, 0), lambda: k3_pass(r.ctx, dp, 0, 1),
             lambda: r.ctx.compose(cp))
    for draw in draws:
        for y0, y1 in ((0, 4), (4, H)):
            r.ctx.set_row_window(y0, y1)
            draw()
    r.ctx.set_row_window()
    assert_same(snapshot(r.ctx), want, "row window from y0 = 4")
    r.close()

    vmax = float(np.abs(f.velocity[..., 1].view(np.float32)).max())
    tiles = _LocalTiles(W, H, 2, tiling.required_halo(3.0, vmax, H, W))
    for t, a in sent.items():
        tiles.upload(t, a)
    tiles.upload(abi.TEX_DEPTH, f.depth)
    for tex, plane in ((abi.TEX_GBUFFER, f.gbuffer), (abi.TEX_VELOCITY, f.velocity), (abi.TEX_DIRECT_LIGHT, f.direct)):
        tiles.upload(tex, plane)
    tiles.ssgi_march(sp)
    tiles.temporal_reproject(tp)
    tiles.after_temporal_pass()
    for i in range(2):
        dp.blueNoiseIndex, dp.inputIsTemporal, dp.writeToB = 2000 + i, (1, 0)[i], i
        tiles.poisson_denoise(dp)
        tiles.after_denoise_pass(i, dp)
    tiles.compose(cp)
    got = {t: tiles.gather(t) for t in _targets()}
    # (K1's target: a tile also draws the two rows beyond its own that K2's clamp reads; the gather takes every tile's own rows)
    assert_same(got, want, "two row tiles")
    assert all(c.halo_violations() == 0 for c in tiles.ctxs)
    for c in tiles.ctxs:
        c.close()
