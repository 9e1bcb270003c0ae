"""rfx.h "AOV conventions" (rfx_set_aov_conventions; the kernel: k0_import.hip k0_aov_pack with conventions in use) on the device, held byte
for byte to tests/aov_convention_ref.py's restatement followed by the C restatement's packers — with the header's rule for a non-finite
velocity (aov_convention_cases.differing).  No case skips on a missing symbol: without rfx_set_aov_conventions they fail.

Runs on the device (-m gpu) and on the host simulator (--hostsim; tests/test_aov_conventions_cpu.py spawns that run)."""
import types

import numpy as np
import pytest

import aov_cases as AC
import aov_convention_cases as CC

pytestmark = pytest.mark.gpu


def _tex():
    from rfx_amd import abi
    return (abi.TEX_DEPTH, abi.TEX_GBUFFER, abi.TEX_VELOCITY, abi.TEX_DIRECT_LIGHT)


def slots_of(ctx):
    return [ctx.download(t) for t in _tex()]


def context(W, H, tile=None):
    from rfx_amd.context import Context
    return Context(W, H) if tile is None else Context(W, H, tile_y0=tile[0], tile_rows=tile[1], halo_rows=tile[2])


def staged_slots(W, H, tile, conv, staged, bands=None):
    ctx = context(W, H, tile)
    assert ctx.has_aov_conventions
    ctx.set_aov_conventions(CC.host(conv))
    for r0, n in bands or [(0, H)]:
        ctx.stage_aov({k: v[r0:r0 + n] for k, v in staged.items()}, r0, n)
    ctx.stage_flip()
    got = slots_of(ctx)
    ctx.close()
    return got


# ---------------------------------------------------------------- 1. every combination, plane form, camera and shape
@pytest.mark.parametrize("dk,vk,ns", CC.COMBINATIONS, ids=["%s-%s-%s" % (CC.DEPTH_KINDS[d], CC.VELOCITY_KINDS[v], CC.NORMAL_SPACES[n]) for d, v, n in CC.COMBINATIONS])
def test_every_combination(dk, vk, ns):
    """depth kind x velocity kind x normal space, each over {F32, F16, typed} planes x {perspective, orthographic} x the shapes at which the
    coordinate stepping can go wrong: 3 x 1 (tail only), 64 x 4 (no tail), 37 x 5 (tail 1, groups that wrap a row), a 5 x 7 row tile (rows
    2..4, halo 1) whose whole-frame band gives all three segments.  (0, 0, 0) is the default: the setting is set and nothing changes.)"""
    bad = []
    for perspective in (True, False):
        conv = CC.setting(dk, vk, ns, perspective)
        for W, H, tile in CC.SHAPES:
            frame = CC.engine_frame(W, H, conv, 0x500 + 16 * W + H)
            for form in CC.FORMS:
                staged = CC.stage(frame, form)
                want = CC.cut(CC.reference(staged, conv, W, H), H, tile)
                got = staged_slots(W, H, tile, conv, staged)
                bad += ["%s %dx%d %s %s: %s" % ("perspective" if perspective else "orthographic", W, H, tile, form, m) for m in CC.differing(got, want)]
    assert not bad, "\n".join(bad[:8])


def test_bands_of_a_row_tile_in_any_order():
    """the 5 x 7 row tile again, the frame staged as three bands out of order (each band its own segments and its own first frame row), under
    the two kinds that read the texel's frame coordinates"""
    W, H, tile = 5, 7, (2, 3, 1)
    for dk in (0, 1):
        conv = CC.setting(dk, 2, 1)
        staged = CC.stage(CC.engine_frame(W, H, conv, 0x77), "f32")
        want = CC.cut(CC.reference(staged, conv, W, H), H, tile)
        got = staged_slots(W, H, tile, conv, staged, bands=[(4, 3), (0, 2), (2, 2)])
        assert not CC.differing(got, want), CC.differing(got, want)


# ---------------------------------------------------------------- 2. coverage edges
@pytest.mark.parametrize("perspective", [True, False], ids=["perspective", "orthographic"])
@pytest.mark.parametrize("dk", [1, 2], ids=["view_z", "position"])
def test_coverage_edges(dk, perspective):
    """+-inf and NaN position or Z, Z = 0, a negative Z, a point behind the camera, beyond far, in front of near, the background position: the
    first seven texels of a 16 x 2 frame (aov_convention_cases.engine_frame).  Each reads as not covered — depth 1, the clear colour in GBUFFER
    and VELOCITY — and the frame equals the restatement."""
    W, H = 16, 2
    conv = CC.setting(dk, 2, 0, perspective)
    for form in ("f32", "f16"):
        staged = CC.stage(CC.engine_frame(W, H, conv, 0x33), form)
        want = CC.reference(staged, conv, W, H)
        got = staged_slots(W, H, None, conv, staged)
        assert not CC.differing(got, want), CC.differing(got, want)
        for slots in (got, want):
            assert (slots[0].reshape(-1)[:7] == 1.0).all(), slots[0].reshape(-1)[:7]
            assert (AC.bits(slots[1]).reshape(-1, 4)[:7] == AC.CLEAR).all() and (AC.bits(slots[2]).reshape(-1, 4)[:7] == AC.CLEAR).all()
        covered = got[0].reshape(-1) < 1.0
        assert covered[7:].any() and not covered[:7].any()


# ---------------------------------------------------------------- 3. set, then reset
def test_set_then_reset_gives_the_default_bytes():
    W, H = 37, 5
    staged = AC.stage(AC.random_planes(W, H, 0x91), AC.TYPED)
    from rfx_amd.context import Context
    a = Context(W, H)
    a.stage_aov(staged)
    a.stage_flip()
    never = slots_of(a)
    a.close()
    b = Context(W, H)
    b.set_aov_conventions(CC.host(CC.setting(2, 2, 1)))
    b.set_aov_conventions(None)
    b.stage_aov(staged)
    b.stage_flip()
    reset = slots_of(b)
    b.set_aov_conventions(CC.host(CC.setting(0, 0, 0)))  # every kind the default: the default
    b.stage_aov(staged)
    b.stage_flip()
    default = slots_of(b)
    b.close()
    for x, y, z in zip(never, reset, default):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_refusals():
    from rfx_amd import abi
    from rfx_amd.context import Context, RfxError
    W, H = 8, 2
    ctx = Context(W, H)

    def refused(conv=None, planes=None, mutate=None):
        c = CC.host(conv).to_abi()
        if mutate:
            mutate(c)
        with pytest.raises(RfxError) as e:
            ctx.set_aov_conventions(c)
            ctx.stage_aov(planes)
        assert "(%d)" % abi.RFX_EINVAL in str(e.value), str(e.value)

    ok = CC.setting(1, 1, 0)
    refused(ok, mutate=lambda c: setattr(c, "depth_kind", 3))
    refused(ok, mutate=lambda c: setattr(c, "velocity_kind", -1))
    refused(ok, mutate=lambda c: setattr(c, "normal_space", 2))
    refused(ok, mutate=lambda c: c.velocity_scale.__setitem__(1, float("inf")))
    refused(ok, mutate=lambda c: c.projectionMatrix.__setitem__(2, 0.25))   # P[0][2]
    refused(ok, mutate=lambda c: c.projectionMatrix.__setitem__(7, 0.25))   # P[1][3]
    refused(CC.setting(0, 2, 0), mutate=lambda c: setattr(c, "near_", c.far_))
    for dk, vk in ((2, 0), (0, 2), (1, 2)):
        conv = CC.setting(dk, vk, 0)
        frame = CC.stage(CC.engine_frame(W, H, conv, 5), "f32")
        wrong = dict(frame)
        if vk == 2:
            wrong["velocity"] = np.zeros((H, W, 2), np.float32)            # a velocity plane under CAMERAS
        else:
            wrong["depth"] = np.ascontiguousarray(frame["depth"][..., 0])  # one channel under POSITION
        refused(conv, wrong)
    ctx.set_aov_conventions(None)
    with pytest.raises(RfxError):
        ctx.stage_aov(dict(depth=np.zeros((H, W, 3), np.float32)))         # a position plane without the setting
    # ... and the context still works
    conv = CC.setting(2, 2, 0)
    staged = CC.stage(CC.engine_frame(W, H, conv, 5), "f32")
    ctx.set_aov_conventions(CC.host(conv))
    assert ctx.aov_stage_bytes(staged) == sum(v.nbytes for v in staged.values())
    ctx.stage_aov(dict({k: v for k, v in staged.items() if k != "depth"}, position=staged["depth"]))  # `position` in place of `depth`
    ctx.stage_flip()
    assert not CC.differing(slots_of(ctx), CC.reference(staged, conv, W, H))
    ctx.close()


# ---------------------------------------------------------------- 4. the EXR entry points
def _exr_channels(staged, conv):
    """the staged planes as the channels of an AOV EXR (imageio.AOV_LAYOUT, the depth plane as position.* / depth.Z) -> (channels, half names, names=)"""
    from rfx_amd import imageio
    ch, half = {}, set()
    dk = CC.DEPTH_KINDS[conv["depth_kind"]]
    names = {} if dk == "fragcoord" else {dk: None}
    layout = dict(imageio.AOV_LAYOUT)
    if dk != "fragcoord":
        layout["depth"] = imageio.ENGINE_DEPTH_LAYOUT[dk]
    for k, v in staged.items():
        v3 = v.reshape(v.shape[0], v.shape[1], -1)
        for j in range(v3.shape[2]):
            ch[layout[k][j]] = v3[..., j]
            if v.dtype == np.float16:
                half.add(layout[k][j])
    return ch, half, names


@pytest.mark.parametrize("form", ["f16", "typed"])
def test_stage_exr_aov_with_a_position_layer(tmp_path, form):
    """a ZIP scanline file with position.X/.Y/.Z stored HALF (f16) and FLOAT (typed) through rfx_stage_exr_aov, POSITION + CAMERAS + VIEW"""
    from rfx_amd import imageio
    W, H = 37, 21
    conv = CC.setting(2, 2, 1)
    staged = CC.stage(CC.engine_frame(W, H, conv, 0x41), form)
    ch, half, names = _exr_channels(staged, conv)
    path = str(tmp_path / "engine.exr")
    imageio.write_exr(path, ch, "zip", half=half)
    data = open(path, "rb").read()
    layout = imageio.exr_aov_layout(data, names)
    assert layout.planes["depth"] == (3, "half" if form == "f16" else "float")
    ctx = context(W, H)
    ctx.set_aov_conventions(CC.host(conv))
    assert ctx.exr_aov_stage_bytes(data, layout) > 0
    ctx.stage_exr_aov(data, layout)
    ctx.stage_flip()
    assert ctx.exr_aov_status() == (0, -1, 0)
    got = slots_of(ctx)
    ctx.set_aov_conventions(None)
    assert ctx.exr_aov_stage_bytes(data, layout) == 0  # three depth components without the setting: refused, as ever
    ctx.close()
    assert not CC.differing(got, CC.reference(staged, conv, W, H))


@pytest.mark.parametrize("way", ["tiled", "piz"])
def test_stage_exr_blocks_with_engine_planes(tmp_path, way):
    """a tiled ZIP file through rfx_stage_exr_blocks and a PIZ scanline file through rfx_stage_exr_blocks_piz: VIEW_Z + SCALED + VIEW"""
    from rfx_amd import imageio
    W, H = 45, 37
    conv = CC.setting(1, 1, 1)
    staged = CC.stage(CC.engine_frame(W, H, conv, 0x42), "typed")
    ch, half, names = _exr_channels(staged, conv)
    path = str(tmp_path / "engine.exr")
    if way == "tiled":
        imageio.write_exr(path, ch, "zip", half=half, tiles=(16, 16))
    else:
        imageio.write_exr(path, ch, "piz", half=half)
    data = open(path, "rb").read()
    ctx = context(W, H)
    assert way != "piz" or ctx.has_exr_piz
    ctx.stage_exr_device(data, names, piz=way == "piz", conventions=CC.host(conv))
    ctx.stage_flip()
    assert ctx.exr_aov_status() == (0, -1, 0)
    got = slots_of(ctx)
    ctx.close()
    assert not CC.differing(got, CC.reference(staged, conv, W, H))


@pytest.mark.parametrize("dk", [1, 2], ids=["view_z", "position"])
def test_a_corrupt_block_reads_as_not_covered(tmp_path, dk):
    """one ZIP chunk with a flipped Adler-32 byte: its 16 rows read as not covered — a non-finite view Z or position is staged there, which the
    conversion turns into depth 1 — and the rest of the frame equals the restatement"""
    from rfx_amd import imageio
    W, H = 24, 40
    conv = CC.setting(dk, 2, 0)
    staged = CC.stage(CC.engine_frame(W, H, conv, 0x43, edges=False), "f32")
    ch, half, names = _exr_channels(staged, conv)
    path = str(tmp_path / "engine.exr")
    imageio.write_exr(path, ch, "zip", half=half)
    d = bytearray(open(path, "rb").read())
    layout = imageio.exr_aov_layout(bytes(d), names)
    rec = layout.chunks[1]  # scanlines 16..31 from the top = frame rows 8..23
    d[int(rec["offset"]) + int(rec["packed_bytes"]) - 1] ^= 0x10
    data = bytes(d)
    ctx = context(W, H)
    ctx.set_aov_conventions(CC.host(conv))
    ctx.stage_exr_aov(data, layout)
    ctx.stage_flip()
    bad, first, code = ctx.exr_aov_status()
    got = slots_of(ctx)
    ctx.close()
    assert (bad, first) == (1, 1) and code != 0
    want = CC.reference(staged, conv, W, H)
    lo, hi = H - (int(rec["y"]) + int(rec["rows"])), H - int(rec["y"])
    assert (got[0][lo:hi] == 1.0).all()
    assert (AC.bits(got[1])[lo:hi] == AC.CLEAR).all() and (AC.bits(got[2])[lo:hi] == AC.CLEAR).all()
    assert (want[0][lo:hi] < 1.0).any()
    keep = np.r_[0:lo, hi:H]
    assert not CC.differing([a[keep] for a in got], [a[keep] for a in want])


# ---------------------------------------------------------------- 5. end to end
def test_chain_from_engine_planes():
    """Three 96 x 54 frames (a moving camera) through SSGIEffect from engine planes — float world position, no velocity plane, camera-space
    normals: POSITION + CAMERAS + VIEW — staged with the frame's conventions, against the reference-form planes the host conversion
    (imageio.aov_to_reference_conventions) makes of them through the synchronous importer: every stage output byte-identical."""
    from rfx_amd import abi, imageio
    from rfx_amd.context import Context
    from rfx_amd.conventions import AovConventions
    from rfx_amd.effect import SSGIEffect
    from rfx_amd.scene import AnalyticScene
    W, H, N = 96, 54, 3
    gen = AnalyticScene(1234)
    frames = []
    for i in range(1, N + 1):
        f = gen.render(W, H, i, aov=True, engine=True)
        conv = AovConventions.from_cameras(f.camera, f.prev_camera, depth_kind="position", velocity_kind="cameras", normal_space="view", background_position=(0.0, 0.0, 0.0))
        eng = {k: f.aov[k] for k in ("diffuse", "roughness", "metalness", "emissive")}
        eng.update(normal=f.engine["view_normal"], position=f.engine["position"], direct=f.direct)
        frames.append((f.camera, conv, eng, imageio.aov_to_reference_conventions(eng, conv)))

    def run(engine):
        ctx = Context(W, H)
        scene = types.SimpleNamespace(frame=None)
        cam = types.SimpleNamespace(**vars(frames[0][0]))
        fx = SSGIEffect(None, scene, cam, dict(width=W, height=H, steps=10, refineSteps=2), seeds=dict(ssgi=3, denoise=4), half_store_rtz=True)
        for camera, conv, eng, ref in frames:
            if engine:
                ctx.set_aov_conventions(conv)
                ctx.stage_aov(eng)
                ctx.stage_flip()
            p = eng if engine else ref
            scene.frame = types.SimpleNamespace(camera=camera, static="resident" if engine else False, depth=ref["depth"], direct=p["direct"], gbuffer=None, velocity=None,
                                                aov={k: v for k, v in p.items() if k not in ("depth", "position", "direct")})
            for k, v in vars(camera).items():
                setattr(cam, k, v)
            fx.update(ctx, None)
        out = [ctx.download(t) for t in (abi.TEX_DEPTH, abi.TEX_GBUFFER, abi.TEX_VELOCITY, abi.TEX_SSGI, abi.TEX_TEMPORAL1, abi.TEX_DENOISE_B0, abi.TEX_COMPOSE)]
        assert ctx.halo_violations() == 0
        ctx.close()
        return out

    a, b = run(False), run(True)
    assert any(x.any() for x in a[3:])
    moved = AC.bits(a[2])[..., :2].view(np.float32)
    assert (np.abs(moved) > 1e-4).any()  # the camera moved: the velocities are not all zero
    for name, x, y in zip(("depth", "gbuffer", "velocity", "ssgi", "temporal1", "denoise_b0", "compose"), a, b):
        assert x.tobytes() == y.tobytes(), name
