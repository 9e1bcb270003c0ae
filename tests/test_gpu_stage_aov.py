"""rfx.h "streamed AOV frames" (rfx_stage_aov / rfx_aov_stage_bytes; the kernel: k0_import.hip k0_aov_pack).  The reference everywhere is the
synchronous importer on the WIDENED planes — rfx_pack_gbuffer + rfx_pack_velocity + rfx_upload — and the check is equality of bytes: half ->
float is exact and the fused kernel calls the packers' own device functions, so there is nothing to tolerate.  Runs on the device (-m gpu) and
on the host simulator (--hostsim; tests/test_stage_aov_cpu.py spawns that run)."""
import ctypes as C
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("diffuse", "normal", "roughness", "metalness", "emissive", "velocity", "depth", "direct")
CHANNELS = dict(diffuse=4, normal=3, roughness=1, metalness=1, emissive=3, velocity=2, depth=1, direct=4)
# plane-type sets: the planes that travel as halves; `direct3`: the direct plane has three channels
TYPESETS = {
    "f32": (frozenset(), False),
    "f16": (frozenset(NAMES), False),
    "typed": (frozenset(NAMES) - {"velocity", "depth"}, False),  # the 44 B/px frame
    "mix": (frozenset(NAMES) - {"normal"}, True),
}
CLEAR = np.array([0, 0, 0, 0x3f800000], np.uint32)
_BASE = {}


def _abi():
    from rfx_amd import abi
    return abi


def _slots():
    abi = _abi()
    return (abi.TEX_DEPTH, abi.TEX_GBUFFER, abi.TEX_VELOCITY, abi.TEX_DIRECT_LIGHT)


def base_planes(W, H):
    """float32 planes of one frame (computed once per size, never modified): the golden fixture's at 96 x 54, AnalyticScene's otherwise; emissive
    lit on a seeded quarter of the texels; a seeded direct plane"""
    if (W, H) in _BASE:
        return _BASE[(W, H)]
    rng = np.random.RandomState(11)
    if (W, H) == (96, 54):
        g = np.load(os.path.join(HERE, "golden", "pack_96x54.npz"))
        p = {k[4:]: np.array(g[k]) for k in g.files if k.startswith("aov_")}
        p["depth"] = np.array(g["depth"])
    else:
        from rfx_amd.scene import AnalyticScene
        f = AnalyticScene(1234).render(W, H, 1, aov=True)
        p = {k: np.array(v) for k, v in f.aov.items()}
        p["depth"] = np.array(f.depth)
        if not (p["depth"] == 1.0).any():  # (so small a frame sees no sky: two texels of it, one of them in the tail)
            p["depth"][-1, -2:] = 1.0
    m = rng.rand(H, W) < 0.25
    p["emissive"][m] = (rng.rand(int(m.sum()), 3) * np.array([6, 3, 1])).astype(np.float32)
    p["direct"] = (rng.rand(H, W, 4) * np.array([4, 2, 1, 1])).astype(np.float32)
    assert set(p) == set(NAMES) and (p["depth"] == 1.0).any() and (p["depth"] < 1.0).any()
    for v in p.values():
        v.setflags(write=False)
    _BASE[(W, H)] = p
    return p


def typed(planes, halves, direct3=False):
    """-> (the planes as they are staged, the same values as float32 planes of full channel count: what the synchronous path is given)"""
    staged, wide = {}, {}
    for k, v in planes.items():
        v = v[..., :3] if (k == "direct" and direct3) else v
        s = np.ascontiguousarray(v.astype(np.float16) if k in halves else v)
        staged[k] = s
        wide[k] = np.ascontiguousarray(s.astype(np.float32))
    if direct3:
        wide["direct"] = np.ascontiguousarray(np.concatenate([wide["direct"], np.ones(wide["direct"].shape[:2] + (1,), np.float32)], -1))
    return staged, wide


def sync_import(ctx, wide):
    """the parent path: whole-frame float32 planes -> the rows each slot holds"""
    abi = _abi()
    r0, n = ctx.held_rows(abi.TEX_GBUFFER)
    band = {k: v[r0:r0 + n] for k, v in wide.items()}
    ctx.pack_gbuffer(band, band["depth"], r0, n)
    ctx.pack_velocity(band, band["depth"], r0, n)
    ctx.upload(abi.TEX_DEPTH, wide["depth"])
    ctx.upload(abi.TEX_DIRECT_LIGHT, band["direct"], r0, n)


def slots_of(ctx):
    return [ctx.download(t) for t in _slots()]


def assert_same(got, want, what=""):
    abi = _abi()
    for t, a, b in zip(_slots(), got, want):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %s differs in %d texels" % (
            what, abi.TEX_NAMES[t], int((a.reshape(a.shape[0], a.shape[1], -1) != b.reshape(a.shape[0], a.shape[1], -1)).any(-1).sum()))


def reference(W, H, wide):
    from rfx_amd.context import Context
    b = Context(W, H)
    sync_import(b, wide)
    out = slots_of(b)
    b.close()
    return out


@pytest.mark.parametrize("W,H", [(96, 54), (97, 55), (5, 3)])
@pytest.mark.parametrize("kind", list(TYPESETS))
def test_staged_aov_frame_equals_the_synchronous_importer(W, H, kind):
    """1. stage_aov + stage_flip against pack_gbuffer + pack_velocity + upload on the widened planes: DEPTH, GBUFFER, VELOCITY and DIRECT_LIGHT
    hold the same bytes.  97 x 55 = 5335 pixels leaves a tail of three, 5 x 3 has three groups and a tail of three in one workgroup.  All-float32
    at 96 x 54 is also held against the reference GLSL's own texels (the fixture), under test_pack_gbuffer_and_velocity_vs_golden's masks."""
    from rfx_amd.context import Context
    halves, direct3 = TYPESETS[kind]
    staged, wide = typed(base_planes(W, H), halves, direct3)
    assert {k for k, v in staged.items() if v.dtype == np.float16} == set(halves) and staged["direct"].shape[-1] == (3 if direct3 else 4)
    a = Context(W, H)
    per_px = sum(v.dtype.itemsize * (v.size // (W * H)) for v in staged.values())
    assert a.aov_stage_bytes(staged) == W * H * per_px
    if kind == "typed":
        assert per_px == 44
    if kind == "f32":
        assert per_px == 76
    a.stage_aov(staged)
    a.stage_flip()
    got = slots_of(a)
    a.close()
    assert_same(got, reference(W, H, wide), "%s %dx%d" % (kind, W, H))
    if kind == "f32" and (W, H) == (96, 54):
        g = np.load(os.path.join(HERE, "golden", "pack_96x54.npz"))
        cov, lit = wide["depth"] < 1.0, np.asarray(g["aov_emissive"]).max(-1) > 0
        assert cov.any()
        for ch in range(3):
            assert np.array_equal(got[1][..., ch][cov], g["gbuffer"][..., ch][cov]), ch
        # (the emissive word where the FIXTURE's emissive is lit: the texels this test lights on top carry other values than the fixture's)
        same_emissive = (wide["emissive"] == g["aov_emissive"]).all(-1)
        assert np.array_equal(got[1][..., 3][cov & lit & same_emissive], g["gbuffer"][..., 3][cov & lit & same_emissive])
        assert np.array_equal(got[2][cov], g["velocity"][cov])


@pytest.mark.parametrize("kind", ["f16", "typed"])
def test_half_edge_values(kind):
    """2. 16 x 4 with the edge values of the half format in the planes: denormals, +-0, 65504, +inf in the emissive, depth exactly 1.0.  No NaN
    goes in.  Background texels hold the clear colour in both packed slots; everything equals the synchronous path on the widened planes."""
    from rfx_amd.context import Context
    W, H = 16, 4
    rng = np.random.RandomState(5)
    h = lambda *shape: rng.rand(*shape).astype(np.float16)  # noqa: E731
    p = dict(diffuse=h(H, W, 4), normal=(h(H, W, 3) - np.float16(0.5)), roughness=h(H, W), metalness=h(H, W), emissive=h(H, W, 3),
             velocity=(h(H, W, 2) - np.float16(0.5)), depth=(h(H, W) * np.float16(0.5) + np.float16(0.25)), direct=h(H, W, 4))
    tiny, big = np.array([1, 0x3ff, 0x8001, 0x83ff], np.uint16).view(np.float16), np.float16(65504)
    p["diffuse"][0, :4, 0] = tiny
    p["diffuse"][0, 4:8, 1] = [0.0, -0.0, big, 1.0]
    p["normal"][1, :4, 2] = [0.0, -0.0, tiny[0], tiny[2]]
    p["normal"][1, :4, 0] = 1.0  # (never the zero vector: 0 / 0 would be a NaN of the test's own making)
    p["roughness"][1, 4:8] = [0.0, -0.0, tiny[1], big]
    p["metalness"][1, 8:12] = [0.0, -0.0, tiny[1], big]
    p["emissive"][2, :4] = [[np.inf, 1, 1], [big, big, big], [tiny[0], 0, 0], [0.0, -0.0, 0.0]]
    p["velocity"][2, 4:8, 0] = [0.0, -0.0, tiny[3], big]
    p["direct"][3, :4, 3] = [0.0, -0.0, tiny[0], big]
    p["direct"][3, 4, 0] = np.inf
    p["depth"][3, 8:] = 1.0
    p["depth"][0, 8] = 1.0
    p["depth"][0, 9:11] = [tiny[0], 0.0]
    assert not any(np.isnan(v.astype(np.float32)).any() for v in p.values())
    halves, _ = TYPESETS[kind]
    staged = {k: (v if k in halves else v.astype(np.float32)) for k, v in p.items()}
    wide = {k: v.astype(np.float32) for k, v in p.items()}
    a = Context(W, H)
    a.stage_aov(staged)
    a.stage_flip()
    got = slots_of(a)
    a.close()
    bg = wide["depth"] == 1.0
    assert int(bg.sum()) == 9
    assert (got[1][bg] == CLEAR).all() and (got[2][bg] == CLEAR).all()
    assert not (got[1][~bg] == CLEAR).all(-1).any()
    assert_same(got, reference(W, H, wide), kind)


def test_bands_and_row_tiles():
    """3. Two calls over rows [0, 40) and [40, 54) give what one call gives.  A row tile (96 x 54, tile rows 20..37, halo 4) handed whole-frame
    planes keeps, in every slot, the rows it holds of the whole-frame result, and copies exactly the bytes the row rule names: DEPTH's plane for
    the whole band, every other plane for band ∩ the slot's rows.  A tile of a 97-wide frame starts its segments at texels that are no multiple
    of four."""
    from rfx_amd.context import Context
    abi = _abi()
    W, H = 96, 54
    staged, wide = typed(base_planes(W, H), *TYPESETS["typed"])
    want = reference(W, H, wide)
    a = Context(W, H)
    for r0, n in ((0, 40), (40, 14)):
        a.stage_aov({k: v[r0:r0 + n] for k, v in staged.items()}, r0, n)
    a.stage_flip()
    assert_same(slots_of(a), want, "two bands")
    a.close()
    for (W, H, y0, rows, halo), kind in (((96, 54, 20, 18, 4), "typed"), ((97, 55, 21, 17, 4), "mix"), ((97, 55, 0, 21, 2), "f32"), ((97, 55, 41, 14, 3), "f16")):
        staged, wide = typed(base_planes(W, H), *TYPESETS[kind])
        want = reference(W, H, wide)
        t = Context(W, H, tile_y0=y0, tile_rows=rows, halo_rows=halo)
        h0, hn = t.held_rows(abi.TEX_GBUFFER)
        assert (h0, hn) == (max(y0 - halo, 0), min(y0 + rows + halo, H) - max(y0 - halo, 0)) and t.held_rows(abi.TEX_DEPTH) == (0, H)
        rule = sum(v.dtype.itemsize * (v.size // (W * H)) * W * (H if k == "depth" else hn) for k, v in staged.items())
        assert t.aov_stage_bytes(staged) == rule
        # ... and of a band that only touches the held rows from below
        part = {k: v[:h0 + 2] for k, v in staged.items()}
        if h0 > 0:
            assert t.aov_stage_bytes(part, 0, h0 + 2) == sum(v.dtype.itemsize * (v.size // (W * H)) * W * ((h0 + 2) if k == "depth" else 2) for k, v in staged.items())
        t.stage_aov(staged)
        t.stage_flip()
        for tex, full in zip(_slots(), want):
            r0, n = t.held_rows(tex)
            assert t.download(tex).tobytes() == full[r0:r0 + n].tobytes(), (abi.TEX_NAMES[tex], W, H, y0)
        t.close()


def test_chain_from_staged_typed_frames():
    """4. Three frames at 160 x 90 through SSGIEffect: frame n + 1 is staged as a typed AOV frame from pinned planes while frame n draws; COMPOSE,
    DENOISE_B0, TEMPORAL1 and SSGI equal the same (half-rounded) frames through the synchronous AOV path bit for bit, no fetch left a held band,
    and a pageable frame is accepted."""
    from rfx_amd.context import Context
    from rfx_amd.effect import SSGIEffect
    from rfx_amd.scene import AnalyticScene
    abi = _abi()
    W, H, N = 160, 90, 3
    halves, _ = TYPESETS["typed"]
    gen = AnalyticScene(1234)
    frames = []
    for i in range(N):
        f = gen.render(W, H, i, aov=True)
        p = dict(f.aov, depth=f.depth, direct=f.direct)
        staged, wide = typed(p, halves)
        frames.append((f.camera, staged, wide))

    def namespace(camera, p, static):
        return types.SimpleNamespace(camera=camera, static=static, depth=p["depth"], direct=p["direct"], gbuffer=None, velocity=None,
                                     aov={k: v for k, v in p.items() if k not in ("depth", "direct")})

    def run(streamed):
        ctx = Context(W, H)
        scene = types.SimpleNamespace(frame=None)
        cam = types.SimpleNamespace(**vars(frames[0][0]))
        fx = SSGIEffect(None, scene, cam, dict(width=W, height=H, steps=10, refineSteps=2), seeds=dict(ssgi=3, denoise=4), half_store_rtz=True)
        if streamed:
            sets = [{k: ctx.host_alloc(v.shape, v.dtype) for k, v in frames[0][1].items()} for _ in range(2)]

            def load(i):
                st = sets[i & 1]
                for k in st:
                    st[k][...] = frames[i][1][k]
                return namespace(frames[i][0], st, "resident")
            cur = load(0)
            ctx.stage_frame(cur)
            ctx.stage_flip()
        for i in range(N):
            if streamed:
                nxt = load(i + 1) if i + 1 < N else None
                if nxt is not None:
                    ctx.stage_frame(nxt)
                scene.frame = cur
            else:
                scene.frame = namespace(frames[i][0], frames[i][2], False)
            for k, v in vars(frames[i][0]).items():
                setattr(cam, k, v)
            fx.update(ctx, None)
            if streamed:
                ctx.stage_flip()
                cur = nxt
        out = [ctx.download(t) for t in (abi.TEX_COMPOSE, abi.TEX_DENOISE_B0, abi.TEX_TEMPORAL1, abi.TEX_SSGI)]
        assert ctx.halo_violations() == 0
        if streamed:
            ctx.stage_aov(frames[0][1])  # pageable: simply not asynchronous
            ctx.stage_flip()
            assert ctx.download(abi.TEX_DEPTH).tobytes() == frames[0][2]["depth"].tobytes()
            assert ctx.download(abi.TEX_DIRECT_LIGHT).tobytes() == frames[0][2]["direct"].tobytes()
        ctx.close()
        return out

    a, b = run(False), run(True)
    assert any(x.any() for x in a)
    for name, x, y in zip(("compose", "denoise_b0", "temporal1", "ssgi"), a, b):
        assert x.tobytes() == y.tobytes(), name


def test_mixed_batch_with_stage_upload():
    """5. One batch, one flip: the packed G-buffer and velocity through stage_upload, depth and direct alone through stage_aov — and the other
    way round in the next batch (a slot stage_aov does not name keeps what stage_upload staged)."""
    from rfx_amd.context import Context
    abi = _abi()
    W, H = 97, 55
    staged, wide = typed(base_planes(W, H), *TYPESETS["typed"])
    want = reference(W, H, wide)
    c = Context(W, H)
    c.stage_upload(abi.TEX_GBUFFER, want[1])
    c.stage_upload(abi.TEX_VELOCITY, want[2])
    c.stage_aov(dict(depth=staged["depth"], direct=staged["direct"]))
    c.stage_flip()
    assert_same(slots_of(c), want, "packed + aov")
    zeros = np.zeros((H, W, 4), np.float32)
    c.stage_aov({k: v for k, v in staged.items() if k != "direct"})
    c.stage_upload(abi.TEX_DIRECT_LIGHT, zeros)
    c.stage_flip()
    assert_same(slots_of(c), [want[0], want[1], want[2], zeros], "aov + packed direct")
    # velocity and normal alone (with the depth every frame carries): VELOCITY and DEPTH are written, GBUFFER keeps the frame before
    c.stage_aov(dict(velocity=staged["velocity"], normal=staged["normal"], depth=np.ascontiguousarray(wide["depth"][::-1])))
    c.stage_flip()
    got = slots_of(c)
    assert got[1].tobytes() == want[1].tobytes() and got[0].tobytes() == wide["depth"][::-1].tobytes() and got[2].tobytes() != want[2].tobytes()
    c.close()


def test_errors_leave_the_context_usable():
    """6. Every RFX_EINVAL and RFX_ESTATE case of the contract; rfx_aov_stage_bytes answers 0 for the same frames; after each, a good frame is
    staged and flipped and arrives."""
    from rfx_amd.context import Context, RfxError
    abi = _abi()
    W, H = 5, 3
    staged, wide = typed(base_planes(W, H), *TYPESETS["typed"])
    want = reference(W, H, wide)
    c = Context(W, H)

    def good():
        c.stage_aov(staged)
        c.stage_flip()
        assert_same(slots_of(c), want, "after an error")

    def refused(code, planes, row0=None, rows=None, mutate=None, rows_arg=None):
        f, r0, n, keep = c._aov_frame(planes, row0, rows)
        n = n if rows_arg is None else rows_arg
        if mutate:
            mutate(f)
        assert c.lib.rfx_aov_stage_bytes(c._h, C.byref(f), r0, n) == 0
        rc = c.lib.rfx_stage_aov(c._h, C.byref(f), r0, n)
        assert rc == code, (rc, c.lib.rfx_last_error(c._h))
        assert b"rfx_stage_aov" in c.lib.rfx_last_error(c._h)
        good()

    good()
    without = lambda *names: {k: v for k, v in staged.items() if k not in names}  # noqa: E731
    refused(abi.RFX_EINVAL, staged, mutate=lambda f: setattr(f.depth, "type", 2))          # a bad type
    refused(abi.RFX_EINVAL, staged, mutate=lambda f: setattr(f.emissive, "type", -1))
    for name, ch in (("normal", 4), ("velocity", 3), ("depth", 2), ("diffuse", 2), ("direct", 1), ("roughness", 3), ("metalness", 0), ("emissive", 4), ("direct", 5)):
        refused(abi.RFX_EINVAL, staged, mutate=lambda f, name=name, ch=ch: setattr(getattr(f, name), "channels", ch))  # a bad channel count
    refused(abi.RFX_EINVAL, without("depth"))                                                # no depth
    for name in ("diffuse", "normal", "roughness", "metalness", "emissive"):                 # a partial G-buffer set
        refused(abi.RFX_EINVAL, without(name, "velocity"))
    refused(abi.RFX_EINVAL, dict(depth=staged["depth"], normal=staged["normal"]))
    refused(abi.RFX_EINVAL, dict(depth=staged["depth"], velocity=staged["velocity"]))        # velocity without normal
    refused(abi.RFX_EINVAL, staged, rows_arg=0)                                              # a band outside DEPTH's rows
    refused(abi.RFX_EINVAL, staged, rows_arg=-2)
    one_row = {k: v[:1] for k, v in staged.items()}
    refused(abi.RFX_EINVAL, one_row, row0=-1, rows=1)
    refused(abi.RFX_EINVAL, one_row, row0=H, rows=1)
    four = {k: np.concatenate([v, v[:1]]) for k, v in staged.items()}
    refused(abi.RFX_EINVAL, four, row0=0, rows=H + 1)
    with pytest.raises(RfxError, match=r"\(-1\)"):
        c.stage_aov(without("depth"))
    with pytest.raises(TypeError):
        c.stage_aov(dict(staged, depth=wide["depth"].astype(np.float64)))
    # RFX_ESTATE: a slot the frame would write lives in a caller's buffer
    other = Context(W, H)
    c.bind_external(abi.TEX_VELOCITY, other.device_ptr(abi.TEX_VELOCITY))
    f, r0, n, keep = c._aov_frame(staged, None, None)
    assert c.lib.rfx_stage_aov(c._h, C.byref(f), r0, n) == abi.RFX_ESTATE
    c.stage_aov(without("velocity"))  # ... a frame that does not name it is still staged
    c.stage_flip()
    got = slots_of(c)
    assert [g.tobytes() for g in (got[0], got[1], got[3])] == [w.tobytes() for w in (want[0], want[1], want[3])]
    c.close()
    other.close()
