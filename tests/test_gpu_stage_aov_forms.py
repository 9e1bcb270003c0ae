"""rfx_stage_aov / k0_aov_pack (k0_import.hip) over every plane form, every half value and the segment shapes its plan can produce, held to
a reference that shares no code with the device functions (tests/aov_cases.py `reference`: the C restatement's packers on the widened planes).

Every case asserts, and reports separately so that a failure names the side:
  (a) stage_aov + stage_flip == the synchronous importer (pack_gbuffer + pack_velocity + upload on the widened planes), byte for byte;
  (b) the synchronous importer == the reference, byte for byte, on the domain aov_cases states;
  (c) hence stage_aov == the reference.
Not held to the restatement: negative colour inputs and a +inf emissive.  Their float -> unsigned conversion saturates on the device and is
undefined in C; those stay under (a) alone in tests/test_gpu_stage_aov.py test_half_edge_values.

Runs on the device (-m gpu) and on the host simulator (--hostsim; tests/test_stage_aov_forms_cpu.py spawns that run and asserts the
generators' premises)."""
import functools

import numpy as np
import pytest

import aov_cases as AC

pytestmark = pytest.mark.gpu


def _tex():
    from rfx_amd import abi
    return (abi.TEX_DEPTH, abi.TEX_GBUFFER, abi.TEX_VELOCITY, abi.TEX_DIRECT_LIGHT)


def slots_of(ctx):
    return [ctx.download(t) for t in _tex()]


def held_of(ctx):
    return [ctx.held_rows(t) for t in _tex()]


def cut(full, rows):
    """the rows each slot holds of whole-frame slot arrays"""
    return [None if a is None else a[r0:r0 + n] for a, (r0, n) in zip(full, rows)]


_EXPECT = {}


def expect(key, W, H, wide):
    """-> (the synchronous importer's slots on a whole-frame context, the reference's), None for a slot the planes do not name; computed
    once per key and only read afterwards"""
    if key not in _EXPECT:
        from rfx_amd.context import Context
        c = Context(W, H)
        AC.sync_import(c, wide)
        sync = [a if w else None for a, w in zip(slots_of(c), AC.written(wide))]
        c.close()
        _EXPECT[key] = (sync, AC.reference(wide))
    return _EXPECT[key]


class Report:
    """collects the three comparisons of a test's cases"""

    def __init__(self):
        self.a, self.b, self.c, self.seen = [], [], [], set()

    def importer(self, key, sync, ref):
        if key not in self.seen:
            self.seen.add(key)
            self.b += ["%s: %s" % (key, m) for m in AC.differing(sync, ref)]

    def staged(self, what, got, sync, ref):
        self.a += ["%s: %s" % (what, m) for m in AC.differing(got, sync)]
        self.c += ["%s: %s" % (what, m) for m in AC.differing(got, ref)]

    def done(self):
        text = "".join("\n(%s) %s: %d differences%s" % (tag, title, len(v), "".join("\n    " + m for m in v[:6]))
                       for tag, title, v in (("a", "stage_aov != the synchronous importer", self.a), ("b", "the synchronous importer != the reference", self.b),
                                             ("c", "stage_aov != the reference", self.c)) if v)
        assert not text, text


def prime(ctx, seed=77):
    """known junk in the front buffers of the four slots (what a slot no call writes must keep) -> the slots"""
    from rfx_amd import abi
    rs = np.random.RandomState(seed)
    for t in _tex():
        ch = abi.TEX_FORMAT[t][1]
        _, n = ctx.held_rows(t)
        ctx.upload(t, rs.rand(*((n, ctx.W, ch) if ch > 1 else (n, ctx.W))).astype(np.float32))
    return slots_of(ctx)


@functools.lru_cache(maxsize=None)
def _random(W, H, seed):
    return AC.random_planes(W, H, seed)


# ---------------------------------------------------------------- 1. every half value through every role
@functools.lru_cache(maxsize=None)
def _every(layout):
    return AC.every_half_frame(layout)


@pytest.mark.parametrize("layout", AC.LAYOUTS)
@pytest.mark.parametrize("kind", list(AC.EVERY_KINDS))
def test_every_half_value_through_every_role(kind, layout):
    """256 x 256, pixel p carries half pattern p (aov_cases.every_half_frame): every finite non-negative half and -0 through the diffuse,
    roughness and metalness bytes, every finite positive half — every power of two from 2^-24 to 2^15 among them — as the emissive maximum in
    r, g or b, +-0 and every other finite half as the normal's z, every non-NaN pattern through velocity, depth and direct.  Staged as halves
    (SET 2), as the typed set (SET 1) and widened (SET 0).  The one pixel whose depth pattern is 0x3c00 is background."""
    from rfx_amd.context import Context
    mask = AC.EVERY_KINDS[kind]
    assert AC.select(AC.ALL, mask) == {"f16": 2, "typed": 1, "f32": 0}[kind]
    staged = AC.stage(_every(layout), mask)
    wide = AC.widen(staged)
    assert {k for k, v in staged.items() if v.dtype == np.float16} == set(AC.names_of(mask)) and not any(np.isnan(v).any() for v in wide.values())
    sync, ref = expect(("every", layout), AC.EVERY_W, AC.EVERY_H, wide)
    ctx = Context(AC.EVERY_W, AC.EVERY_H)
    ctx.stage_aov(staged)
    ctx.stage_flip()
    got = slots_of(ctx)
    ctx.close()
    bg = wide["depth"] == 1.0
    assert int(bg.sum()) == 1
    assert (got[1][bg] == AC.CLEAR).all() and (got[2][bg] == AC.CLEAR).all(), "a background texel without the clear colour"
    assert not (got[1][~bg] == AC.CLEAR).all(-1).any(), "a foreground texel with the clear colour"
    r = Report()
    r.importer("layout %d" % layout, sync, ref)
    r.staged("%s layout %d" % (kind, layout), got, sync, ref)
    r.done()


# ---------------------------------------------------------------- 2. every plane form
def _form_expect(f, d, q):
    wide = AC.widen(AC.stage(AC.form_frame(f), 0, d, q))
    return expect(("form", f, d, q), AC.FORM_W, AC.FORM_H, wide)


@pytest.mark.parametrize("group", AC.FORM_GROUPS)
def test_every_plane_form(group):
    """7 x 3 (five groups and a tail of one) on one context, case after case (aov_cases.form_cases): the channel counts of diffuse and direct,
    all 256 half masks, and every plane subset under every mask over its planes.  Three frames of halves alternate, so the back buffer a case
    writes holds another frame's texels, and a slot the case does not name must keep the texels of the case before."""
    from rfx_amd.context import Context
    W, H = AC.FORM_W, AC.FORM_H
    ctx = Context(W, H)
    held_s = prime(ctx)
    held_r = list(held_s)
    r = Report()
    sets = set()
    for i, (subset, mask, d, q) in enumerate(AC.form_cases()[group]):
        f = i % 3
        staged = AC.stage(AC.form_frame(f), mask, d, q, AC.SUBSETS[subset])
        sets.add(AC.select(AC.mask_of(staged), mask))
        sync, ref = _form_expect(f, d, q)
        r.importer("frame %d diffuse %d direct %d" % (f, d, q), sync, ref)
        for k, w in enumerate(AC.written(staged)):
            if w:
                held_s[k], held_r[k] = sync[k], ref[k]
        assert ctx.aov_stage_bytes(staged) == sum(v.nbytes for v in staged.values())
        ctx.stage_aov(staged)
        ctx.stage_flip()
        r.staged("%s mask %02x diffuse %d direct %d" % (subset, mask, d, q), slots_of(ctx), held_s, held_r)
    assert ctx.halo_violations() == 0
    ctx.close()
    assert sets == ({0, 2} if group == "depth" else {0, 1, 2})
    r.done()


@pytest.mark.parametrize("frame", AC.DIFFUSE3_FRAMES, ids=lambda f: "%dx%d%s" % (f[0], f[1], "-tile%d" % f[2][0] if f[2] else ""))
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_three_channel_diffuse(kind, frame):
    """a 3-channel diffuse (alpha 1) through the group path and the tail: 97 x 55 (tail 3), 5 x 3, and row tiles of a 97-wide frame, whose
    segments start at texels that are no multiple of four"""
    from rfx_amd.context import Context
    W, H, tile = frame
    staged = AC.stage(_random(W, H, 0x3d), AC.EVERY_KINDS[kind], 3, 4)
    wide = AC.widen(staged)
    assert staged["diffuse"].shape == (H, W, 3) and staged["diffuse"].dtype == (np.float16 if kind == "f16" else np.float32)
    sync, ref = expect(("diffuse3", W, H), W, H, wide)
    ctx = Context(W, H) if tile is None else Context(W, H, tile_y0=tile[0], tile_rows=tile[1], halo_rows=tile[2])
    rows = held_of(ctx)
    if tile is not None:
        assert rows[1] == AC.held(H, *tile) and rows[0] == (0, H)
    ctx.stage_aov(staged)
    ctx.stage_flip()
    got = slots_of(ctx)
    assert ctx.halo_violations() == 0
    ctx.close()
    fg = wide["depth"][rows[1][0]:rows[1][0] + rows[1][1]] < 1.0
    assert fg.any() and ((got[1][..., 0] >> 24)[fg] == 254).all(), "alpha 1 packs to the byte 254 (min(1 + 1e-4, 0.999999) * 255)"
    r = Report()
    r.importer("%d x %d" % (W, H), sync, ref)
    r.staged("%s %s" % (kind, frame), got, cut(sync, rows), cut(ref, rows))
    r.done()


# ---------------------------------------------------------------- 3. segment shapes
def test_tiny_segments():
    """whole frames of 1 x 1, 3 x 1, 1 x 3 (tail only) and 2 x 2 (one group, no tail), and a width-1 frame on a row tile whose three
    segments have three pixels each"""
    from rfx_amd.context import Context
    r = Report()
    forms = [(m, ch) for m in (0, AC.TYPED, AC.ALL) for ch in (3, 4)]
    for W, H in AC.TINY_FRAMES:
        ctx = Context(W, H)
        for i, (mask, ch) in enumerate(forms):
            staged = AC.stage(_random(W, H, 0x100 + i % 3), mask, ch, ch)
            sync, ref = expect(("tiny", W, H, i % 3, ch), W, H, AC.widen(staged))
            r.importer("%d x %d frame %d channels %d" % (W, H, i % 3, ch), sync, ref)
            assert ctx.aov_stage_bytes(staged) == sum(v.nbytes for v in staged.values())
            ctx.stage_aov(staged)
            ctx.stage_flip()
            r.staged("%d x %d mask %02x channels %d" % (W, H, mask, ch), slots_of(ctx), sync, ref)
        ctx.close()
    W, H, y0, n, halo = AC.TINY_TILE
    ctx = Context(W, H, tile_y0=y0, tile_rows=n, halo_rows=halo)
    rows = held_of(ctx)
    assert rows[1] == (3, 3) and W * 3 < 4
    for i, (mask, ch) in enumerate(forms):
        staged = AC.stage(_random(W, H, 0x110 + i % 3), mask, ch, ch)
        sync, ref = expect(("tiny", W, H, i % 3, ch), W, H, AC.widen(staged))
        r.importer("%d x %d frame %d channels %d" % (W, H, i % 3, ch), sync, ref)
        ctx.stage_aov(staged)
        ctx.stage_flip()
        r.staged("tile %d x %d mask %02x channels %d" % (W, H, mask, ch), slots_of(ctx), cut(sync, rows), cut(ref, rows))
    assert ctx.halo_violations() == 0
    ctx.close()
    r.done()


@pytest.mark.parametrize("kind", ["typed", "f16"])
def test_band_outside_the_held_rows(kind):
    """a row tile (13 x 20, rows 8..11, halo 2: the slots but DEPTH hold rows 6..13) handed bands that miss its held rows: DEPTH changes for
    exactly the band's rows, GBUFFER, VELOCITY and DIRECT_LIGHT keep their bytes, and only the depth rows are copied.  (The tile is staged
    twice with frame A first, so that both buffers of every slot hold A.)  typed: depth is float32 (SET 0); f16: a half (SET 2)."""
    from rfx_amd.context import Context
    W, H, y0, n, halo = 13, 20, 8, 4, 2
    mask = AC.EVERY_KINDS[kind]
    A, B = AC.stage(_random(W, H, 0xa), mask), AC.stage(_random(W, H, 0xb), mask)
    sync, ref = expect(("outside", kind), W, H, AC.widen(A))
    ctx = Context(W, H, tile_y0=y0, tile_rows=n, halo_rows=halo)
    rows = held_of(ctx)
    assert rows == [(0, H), (6, 8), (6, 8), (6, 8)]
    r = Report()
    r.importer("frame A", sync, ref)
    for r0, rn in ((0, 5), (14, 6), (2, 3), (0, 6)):
        for _ in range(2):
            ctx.stage_aov(A)
            ctx.stage_flip()
        before = slots_of(ctx)
        r.staged("frame A before the band %d+%d" % (r0, rn), before, cut(sync, rows), cut(ref, rows))
        band = {k: v[r0:r0 + rn] for k, v in B.items()}
        assert ctx.aov_stage_bytes(band, r0, rn) == band["depth"].nbytes
        ctx.stage_aov(band, r0, rn)
        ctx.stage_flip()
        got = slots_of(ctx)
        want = AC.widen(A)["depth"].copy()
        want[r0:r0 + rn] = AC.widen(B)["depth"][r0:r0 + rn]
        assert (want != AC.widen(A)["depth"]).any()
        assert got[0].tobytes() == want.tobytes(), "DEPTH after the band %d+%d" % (r0, rn)
        for k in (1, 2, 3):
            assert got[k].tobytes() == before[k].tobytes(), "%s changed by the band %d+%d" % (AC.SLOTS[k], r0, rn)
    assert ctx.halo_violations() == 0
    ctx.close()
    r.done()


def test_staging_area_grows_within_a_batch():
    """one batch stages a 2-row band, then the remaining 52 rows of a 96 x 54 typed frame (the staging area is freed and allocated anew while
    the first band's copies and kernel may be in flight), then flips: the one-call result.  Again on the same context with an all-float32
    frame, whose 52-row band needs a larger area still."""
    from rfx_amd.context import Context
    W, H = 96, 54
    ctx, one = Context(W, H), Context(W, H)
    r = Report()
    for seed, mask in ((0x51, AC.TYPED), (0x52, 0)):
        staged = AC.stage(_random(W, H, seed), mask)
        sync, ref = expect(("growth", seed), W, H, AC.widen(staged))
        r.importer("frame %x" % seed, sync, ref)
        sizes = [ctx.aov_stage_bytes({k: v[r0:r0 + n] for k, v in staged.items()}, r0, n) for r0, n in ((0, 2), (2, 52))]
        assert sizes[0] < sizes[1] and sum(sizes) == sum(v.nbytes for v in staged.values())
        for r0, n in ((0, 2), (2, 52)):
            ctx.stage_aov({k: v[r0:r0 + n] for k, v in staged.items()}, r0, n)
        ctx.stage_flip()
        got = slots_of(ctx)
        one.stage_aov(staged)
        one.stage_flip()
        assert not AC.differing(got, slots_of(one)), "two bands differ from one call"
        r.staged("frame %x in two bands" % seed, got, sync, ref)
    ctx.close()
    one.close()
    r.done()


def test_front_buffers_stay_intact_while_the_next_frame_is_staged():
    """stage and flip frame A; stage frame B, in which every plane differs, without flipping: the four slots still download as A, and as B
    after the flip"""
    from rfx_amd.context import Context
    W, H = 37, 11
    A, B = AC.stage(_random(W, H, 0xa1), AC.TYPED, 3, 4), AC.stage(_random(W, H, 0xb1), AC.ALL, 4, 3)
    assert all((AC.widen(A)[k] != AC.widen(B)[k]).any() for k in AC.NAMES)
    ea, eb = expect(("front", "A"), W, H, AC.widen(A)), expect(("front", "B"), W, H, AC.widen(B))
    assert len(AC.differing(ea[0], eb[0])) == 4  # every slot differs between the two frames
    r = Report()
    r.importer("A", *ea)
    r.importer("B", *eb)
    ctx = Context(W, H)
    ctx.stage_aov(A)
    ctx.stage_flip()
    r.staged("A", slots_of(ctx), *ea)
    ctx.stage_aov(B)
    r.staged("A while B is staged", slots_of(ctx), *ea)
    ctx.stage_flip()
    r.staged("B", slots_of(ctx), *eb)
    ctx.close()
    r.done()


def test_random_tilings():
    """aov_cases.random_tilings: frames of up to 70 x 40 on a random row tile, the frame's rows cut into 1..4 bands staged in a random order
    (bands outside the held rows among them), a random half mask, channel counts and plane subset.  Every slot holds its rows of the
    whole-frame result, a slot the subset does not name keeps what it held, and the calls copy exactly the bytes of the row rule."""
    from rfx_amd.context import Context
    from test_stage_aov_cpu import row_rule
    r = Report()
    for i, t in enumerate(AC.random_tilings()):
        W, H = t["W"], t["H"]
        staged = AC.stage(AC.random_planes(W, H, t["seed"]), t["mask"], t["diffuse_ch"], t["direct_ch"], AC.SUBSETS[t["subset"]])
        sync, ref = expect(("tiling", i), W, H, AC.widen(staged))
        r.importer("tiling %d" % i, sync, ref)
        ctx = Context(W, H, tile_y0=t["y0"], tile_rows=t["rows"], halo_rows=t["halo"])
        rows = held_of(ctx)
        assert rows[1] == AC.held(H, t["y0"], t["rows"], t["halo"]) and rows[0] == (0, H)
        kept = prime(ctx, 100 + i)
        ty = {k: int(v.dtype == np.float16) for k, v in staged.items()}
        ch = {k: v.size // (W * H) for k, v in staged.items()}
        copied = rule = 0
        for r0, n in t["bands"]:
            band = {k: v[r0:r0 + n] for k, v in staged.items()}
            copied += ctx.aov_stage_bytes(band, r0, n)
            rule += row_rule(W, H, rows[1][0], rows[1][1], ty, ch, r0, n)[1]
            ctx.stage_aov(band, r0, n)
        ctx.stage_flip()
        assert copied == rule, (t, copied, rule)
        want_s = [k if w is None else w for w, k in zip(cut(sync, rows), kept)]
        want_r = [k if w is None else w for w, k in zip(cut(ref, rows), kept)]
        r.staged("tiling %d %s" % (i, t), slots_of(ctx), want_s, want_r)
        assert ctx.halo_violations() == 0
        ctx.close()
    r.done()
