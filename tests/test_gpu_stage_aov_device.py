"""rfx.h "device planes" (rfx_stage_aov_device; the kernels: k0_import.hip k0_aov_pack_strided, and k0_aov_pack on the caller's pointers where a
segment is tight).  The reference everywhere is the merged host path — the same element values as contiguous host arrays through
Context.stage_aov on a second context — and the check is equality of bytes over the held rows of DEPTH, GBUFFER, VELOCITY and DIRECT_LIGHT:
both paths call the same packing device functions on the same widened values, so there is nothing to tolerate.  No case skips on a missing
symbol: without rfx_stage_aov_device they fail.

Runs on the device (-m gpu) and on the host simulator (--hostsim; tests/test_stage_aov_device_cpu.py spawns that run), where "device" memory is
host memory and the planes are abi.DevicePlane records over numpy arrays."""
import ctypes as C
import types

import numpy as np
import pytest

import aov_cases as AC
import aov_convention_cases as CC
import aov_device_cases as D

pytestmark = pytest.mark.gpu
_REF = {}


def reference(W, H, kind, seed, const=False, subset=AC.NAMES, diffuse_ch=4, direct_ch=4, tile=None):
    """(staged whole-frame planes, the host path's slots), computed once per key"""
    key = (W, H, kind, seed, const, subset, diffuse_ch, direct_ch, tile)
    if key not in _REF:
        staged = AC.stage(D.frame(W, H, seed), D.TYPES[kind], diffuse_ch, direct_ch, subset)
        if const:
            staged = D.constant(staged)
        for v in staged.values():
            v.setflags(write=False)
        _REF[key] = (staged, D.host_reference(W, H, staged, tile))
    return _REF[key]


def staged_device(W, H, calls, tile=None, conv=None, before=None):
    """calls: [(planes, row0, rows)] of abi.DevicePlane dicts, one batch, one flip -> the slots"""
    ctx = D.context(W, H, tile, conv)
    assert ctx.has_stage_aov_device
    if before:
        before(ctx)
    for planes, r0, n in calls:
        ctx.stage_aov_device(planes, r0, n)
    ctx.stage_flip()
    got = D.slots_of(ctx)
    ctx.close()
    return got


# ---------------------------------------------------------------- 1. layouts x sizes x types
def _combinations():
    """every layout at every size (60), the plane types dealt out in turn: every type meets every layout and every size"""
    kinds = list(D.TYPES)
    out = []
    for i, layout in enumerate(D.LAYOUTS):
        for j, (W, H) in enumerate(D.SIZES):
            out.append((layout, W, H, kinds[(i + j) % 3]))
    assert {c[0] for c in out} == set(D.LAYOUTS) and {c[1:3] for c in out} == set(D.SIZES) and {c[3] for c in out} == set(kinds)
    for layout in D.LAYOUTS:
        assert len({c[3] for c in out if c[0] == layout}) == 3
    return out


@pytest.mark.parametrize("layout,W,H,kind", _combinations(), ids=lambda v: str(v))
def test_layouts_sizes_types(layout, W, H, kind):
    """(1, 1): no group at all; (3, 2): only a tail; (4, 3): exactly one group per row; (5, 4), (66, 5), (97, 55): W mod 4 = 1, 2, 1 with odd
    rows and, at 97 x 55, more than one workgroup along the rows."""
    staged, want = reference(W, H, kind, 0x300 + W, const=layout == "broadcast")
    arena = D.Arena()
    got = staged_device(W, H, [(D.device_planes(arena, staged, layout), 0, H)])
    bad = D.same_bytes(got, want)
    assert not bad, "\n".join(bad)


def test_layouts_differ_per_plane():
    """one frame, another layout for every plane (seeded), at 66 x 5 and 97 x 55"""
    rng = np.random.RandomState(0xd1)
    for W, H in ((66, 5), (97, 55)):
        staged, want = reference(W, H, "mix", 0x300 + W)
        arena = D.Arena()
        pool = [la for la in D.LAYOUTS if la != "broadcast"]
        planes = {k: D.plane(arena, v, pool[int(rng.randint(len(pool)))]) for k, v in staged.items()}
        arena.ready()
        bad = D.same_bytes(staged_device(W, H, [(planes, 0, H)]), want)
        assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- 2. plane sets
@pytest.mark.parametrize("subset,ch", [("depth", 4), ("depth_direct", 4), ("depth_velocity_normal", 4), ("all", 3)])
def test_plane_sets(subset, ch):
    """depth only; depth + direct; velocity + normal + depth without a G-buffer; 3-channel diffuse and direct — a slot the frame does not name
    keeps the frame before (staged first, through the host path, on both contexts)"""
    for (W, H), layout in (((5, 4), "planar_pitch"), ((97, 55), "pitch1"), ((97, 55), "pitch4")):
        first, _ = reference(W, H, "typed", 0x411)
        staged, _ = reference(W, H, "mix", 0x400 + W, subset=AC.SUBSETS[subset], diffuse_ch=ch, direct_ch=ch)
        ref = D.context(W, H)
        ref.stage_aov(dict(first))
        ref.stage_flip()
        ref.stage_aov(dict(staged))
        ref.stage_flip()
        want = D.slots_of(ref)
        ref.close()
        arena = D.Arena()
        ctx = D.context(W, H)
        ctx.stage_aov(dict(first))
        ctx.stage_flip()
        ctx.stage_aov_device(D.device_planes(arena, staged, layout))
        ctx.stage_flip()
        got = D.slots_of(ctx)
        ctx.close()
        bad = D.same_bytes(got, want)
        assert not bad, "%s %dx%d %s: %s" % (subset, W, H, layout, "\n".join(bad))


# ---------------------------------------------------------------- 3. bands and batches
def test_bands_and_mixed_batches():
    """row0 > 0; two calls with different layouts over two bands before one flip; one batch mixing stage_upload, stage_aov and stage_aov_device"""
    from rfx_amd import abi
    W, H = 97, 55
    staged, want = reference(W, H, "typed", 0x500)
    arena = D.Arena()
    lower, upper = D.device_planes(arena, staged, "planar_pitch", 0, 21), D.device_planes(arena, staged, "top", 21, 34)
    bad = D.same_bytes(staged_device(W, H, [(upper, 21, 34), (lower, 0, 21)]), want)
    assert not bad, "\n".join(bad)
    # a band with row0 > 0 alone: the rows below keep what their buffer held (another frame, staged twice: both buffers of every slot hold it)
    other, other_want = reference(W, H, "f32", 0x501)
    ctx = D.context(W, H)
    for _ in range(2):
        ctx.stage_aov(dict(other))
        ctx.stage_flip()
    ctx.stage_aov_device(D.device_planes(arena, staged, "pitch5", 30, 25), 30, 25)
    ctx.stage_flip()
    got = D.slots_of(ctx)
    for g, a, b in zip(got, other_want, want):
        assert g[:30].tobytes() == a[:30].tobytes() and g[30:].tobytes() == b[30:].tobytes()
    # one batch: the packed G-buffer through stage_upload, velocity + normal + depth of the lower band from device planes, the upper band's
    # depth and the direct plane through stage_aov
    ctx.stage_upload(abi.TEX_GBUFFER, want[1])
    vel = {k: staged[k] for k in ("velocity", "normal", "depth")}
    ctx.stage_aov_device(D.device_planes(arena, vel, "mirror_x", 0, 40), 0, 40)
    ctx.stage_aov_device(D.device_planes(arena, vel, "planar", 40, 15), 40, 15)
    ctx.stage_aov(dict(depth=staged["depth"][10:], direct=staged["direct"][10:]), 10, 45)
    ctx.stage_aov_device(D.device_planes(arena, dict(depth=staged["depth"], direct=staged["direct"]), "pitch4", 0, 10), 0, 10)
    ctx.stage_flip()
    bad = D.same_bytes(D.slots_of(ctx), want)
    ctx.close()
    assert not bad, "\n".join(bad)


def test_row_tiles():
    """H = 55 in three tiles with halo 4, whole-frame planes staged on each: every slot's held rows equal the reference's"""
    W, H = 97, 55
    staged, want = reference(W, H, "mix", 0x600)
    arena = D.Arena()
    for (y0, n), layout in (((0, 19), "planar_pitch"), ((19, 18), "pitch1"), ((37, 18), "top")):
        tile = (y0, n, 4)
        got = staged_device(W, H, [(D.device_planes(arena, staged, layout), 0, H)], tile)
        r0, rows = CC.held(H, tile)
        assert got[1].shape[0] == rows and got[0].shape[0] == H
        bad = D.same_bytes(got, CC.cut(want, H, tile))
        assert not bad, "%s: %s" % (tile, "\n".join(bad))
    # ... and a tight frame on a tile: the flat kernel on the caller's pointers, segment by segment
    got = staged_device(W, H, [(D.device_planes(arena, staged, "tight"), 0, H)], (19, 18, 4))
    assert not D.same_bytes(got, CC.cut(want, H, (19, 18, 4)))


# ---------------------------------------------------------------- 4. conventions
@pytest.mark.parametrize("dk,vk,ns", [(2, 2, 1), (1, 1, 0), (0, 2, 0)], ids=["position-cameras-view", "view_z-scaled", "fragcoord-cameras"])
def test_conventions(dk, vk, ns):
    """at 97 x 55 and 5 x 4, planar top-down (the element form at these widths), planar with padded rows bottom-up and top-down and interleaved
    with padded rows top-down (the vector forms, with a negative stride_y too), in every plane type set; the host path under the same setting is
    the reference"""
    bad = []
    for W, H in ((97, 55), (5, 4)):
        conv = CC.setting(dk, vk, ns)
        frame = CC.engine_frame(W, H, conv, 0x700 + W)
        for kind, mask in D.TYPES.items():
            staged = {k: np.ascontiguousarray(v if mask & AC.BIT[k] else v.astype(np.float32)) for k, v in frame.items()}
            want = D.host_reference(W, H, staged, conv=CC.host(conv))
            for layout in ("planar_top", "planar_pitch", "planar_pitch_top", "pitch4_top"):
                arena = D.Arena()
                got = staged_device(W, H, [(D.device_planes(arena, staged, layout), 0, H)], conv=CC.host(conv))
                bad += ["%dx%d %s %s: %s" % (W, H, kind, layout, m) for m in D.same_bytes(got, want)]
            assert (want[0] < 1.0).any() and (want[0] == 1.0).any()
    assert not bad, "\n".join(bad[:8])


# ---------------------------------------------------------------- 5. the chain
def test_chain_from_device_planes():
    """Three frames at 96 x 54 through SSGIEffect, each staged from device planes (planar top-down) through Context.stage_frame: every stage
    output is byte-identical to the run staged through stage_aov"""
    from rfx_amd import abi
    from rfx_amd.effect import SSGIEffect
    from rfx_amd.scene import AnalyticScene
    W, H, N = 96, 54, 3
    halves, _ = (frozenset(AC.NAMES) - {"velocity", "depth"}, False)
    gen = AnalyticScene(1234)
    frames = []
    for i in range(N):
        f = gen.render(W, H, i, aov=True)
        p = dict(f.aov, depth=f.depth, direct=f.direct)
        frames.append((f.camera, {k: np.ascontiguousarray(v.astype(np.float16) if k in halves else v) for k, v in p.items()}))

    def run(device):
        ctx = D.context(W, H)
        arena = D.Arena()
        scene = types.SimpleNamespace(frame=None)
        cam = types.SimpleNamespace(**vars(frames[0][0]))
        fx = SSGIEffect(None, scene, cam, dict(width=W, height=H, steps=10, refineSteps=2), seeds=dict(ssgi=3, denoise=4), half_store_rtz=True)
        for i in range(N):
            p = D.device_planes(arena, frames[i][1], "planar_top") if device else frames[i][1]
            frame = types.SimpleNamespace(camera=frames[i][0], static="resident", depth=p["depth"], direct=p["direct"], gbuffer=None, velocity=None,
                                          aov={k: v for k, v in p.items() if k not in ("depth", "direct")})
            ctx.stage_frame(frame)
            ctx.stage_flip()
            scene.frame = frame
            for k, v in vars(frames[i][0]).items():
                setattr(cam, k, v)
            fx.update(ctx, None)
        out = [ctx.download(t) for t in (abi.TEX_DEPTH, abi.TEX_GBUFFER, abi.TEX_VELOCITY, abi.TEX_DIRECT_LIGHT, abi.TEX_SSGI, abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1,
                                         abi.TEX_DENOISE_A0, abi.TEX_DENOISE_B0, abi.TEX_COMPOSE)]
        assert ctx.halo_violations() == 0
        ctx.close()
        return out

    a, b = run(False), run(True)
    assert any(x.any() for x in a[4:])
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), i


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_batch_as_it_was():
    """each refusal returns its code and names the entry point; a valid staging plus flip right after gives the right bytes"""
    from rfx_amd import abi
    from rfx_amd.context import Context
    W, H = 5, 4
    staged, want = reference(W, H, "typed", 0xa00)
    arena = D.Arena()
    good_planes = D.device_planes(arena, staged, "planar_pitch")
    c = Context(W, H)

    def good():
        c.stage_aov_device(good_planes)
        c.stage_flip()
        bad = D.same_bytes(D.slots_of(c), want)
        assert not bad, "\n".join(bad)

    def refused(code, planes=None, mutate=None, row0=0, rows=H):
        f, _, _ = c._aov_device_frame(dict(good_planes) if planes is None else planes, 0, H)
        if mutate:
            mutate(f)
        rc = c.lib.rfx_stage_aov_device(c._h, C.byref(f), row0, rows, None)
        msg = c.lib.rfx_last_error(c._h)
        assert rc == code and b"rfx_stage_aov_device" in msg, (rc, msg)
        good()

    good()
    without = lambda *names: {k: v for k, v in good_planes.items() if k not in names}  # noqa: E731
    E = abi.RFX_EINVAL
    refused(E, mutate=lambda f: setattr(f.depth, "type", 2))
    refused(E, mutate=lambda f: setattr(f.emissive, "type", -1))
    for name, ch in (("normal", 4), ("velocity", 3), ("depth", 2), ("depth", 3), ("diffuse", 2), ("direct", 5), ("roughness", 3), ("metalness", 0), ("emissive", 4)):
        refused(E, mutate=lambda f, name=name, ch=ch: setattr(getattr(f, name), "channels", ch))
    refused(E, without("depth"))
    for name in ("diffuse", "normal", "roughness", "metalness", "emissive"):
        refused(E, without(name, "velocity"))
    refused(E, dict(depth=good_planes["depth"], velocity=good_planes["velocity"]))
    for r0, n in ((0, 0), (0, -2), (-1, 1), (H, 1), (0, H + 1)):
        refused(E, row0=r0, rows=n)
    # an address that is not a multiple of the element size: a float plane, a half plane
    refused(E, mutate=lambda f: setattr(f.depth, "data", f.depth.data + 2))
    refused(E, mutate=lambda f: setattr(f.normal, "data", f.normal.data + 1))
    # extents beyond 62 bits of bytes, with strides whose products overflow 64 bits
    refused(E, mutate=lambda f: setattr(f.depth, "stride_y", 2 ** 62))
    refused(E, mutate=lambda f: setattr(f.depth, "stride_x", -2 ** 63))
    refused(E, mutate=lambda f: setattr(f.diffuse, "stride_c", 2 ** 60))
    refused(E, mutate=lambda f: (setattr(f.direct, "stride_x", 2 ** 58), setattr(f.direct, "stride_y", -2 ** 59)))
    # a velocity plane under CAMERAS, a 1-channel depth under POSITION
    c.set_aov_conventions(CC.host(CC.setting(0, 2, 0)))
    rc = c.lib.rfx_stage_aov_device(c._h, C.byref(c._aov_device_frame(dict(good_planes), 0, H)[0]), 0, H, None)
    assert rc == E and b"rfx_stage_aov_device" in c.lib.rfx_last_error(c._h)
    c.set_aov_conventions(CC.host(CC.setting(2, 0, 0)))
    rc = c.lib.rfx_stage_aov_device(c._h, C.byref(c._aov_device_frame(dict(good_planes), 0, H)[0]), 0, H, None)
    assert rc == E
    c.set_aov_conventions(None)
    good()
    # a producer stream is not taken in this version
    f = c._aov_device_frame(dict(good_planes), 0, H)[0]
    assert c.lib.rfx_stage_aov_device(c._h, C.byref(f), 0, H, C.c_void_p(4096)) == abi.RFX_EUNSUPPORTED and b"rfx_stage_aov_device" in c.lib.rfx_last_error(c._h)
    good()
    # RFX_ESTATE: a slot the frame would write lives in a caller's buffer
    other = Context(W, H)
    c.bind_external(abi.TEX_VELOCITY, other.device_ptr(abi.TEX_VELOCITY))
    f = c._aov_device_frame(dict(good_planes), 0, H)[0]
    assert c.lib.rfx_stage_aov_device(c._h, C.byref(f), 0, H, None) == abi.RFX_ESTATE and b"rfx_stage_aov_device" in c.lib.rfx_last_error(c._h)
    c.stage_aov_device(without("velocity"))  # ... a frame that does not name it is still staged
    c.stage_flip()
    got = D.slots_of(c)
    assert [g.tobytes() for g in (got[0], got[1], got[3])] == [w.tobytes() for w in (want[0], want[1], want[3])]
    c.close()
    other.close()
