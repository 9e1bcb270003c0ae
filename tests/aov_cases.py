"""Test helper (pure Python + numpy): the frames, the case lists and the reference of the streamed AOV import's form tests
(tests/test_gpu_stage_aov_forms.py on the device and under --hostsim, tests/test_stage_aov_forms_cpu.py for the premises).

The reference is INDEPENDENT of the device functions: `reference` packs the widened planes with the C restatement (oracle/rfx_oracle.c
rfxo_pack_gbuffer / rfxo_pack_velocity), which shares no code with k0_import.hip.  Every frame here is drawn as HALVES (float16 arrays of
full channel count), so that one set of values serves every plane form: `stage` turns it into what a host hands rfx_stage_aov for a half
mask, channel counts and a plane subset, `widen` into the float32 planes the synchronous importer and the reference are given.

The domain on which the synchronous importer is held to the restatement (what the generators keep to): colour inputs (diffuse, roughness,
metalness) finite and >= 0 or -0, emissive finite with a positive maximum or black, normals finite and not the zero vector, no NaN anywhere.
A negative colour or a +inf emissive reaches a float -> unsigned conversion that saturates on the device and is undefined in C: such inputs
stay with tests/test_gpu_stage_aov.py test_half_edge_values, under the fused-against-synchronous check alone."""
import itertools

import numpy as np

NAMES = ("diffuse", "normal", "roughness", "metalness", "emissive", "velocity", "depth", "direct")  # rfx_aov_frame's order: bit i of a half mask
CHANNELS = dict(diffuse=4, normal=3, roughness=1, metalness=1, emissive=3, velocity=2, depth=1, direct=4)
BIT = {k: 1 << i for i, k in enumerate(NAMES)}
ALL = 0xff
TYPED = ALL & ~(BIT["velocity"] | BIT["depth"])  # the 44 B/px frame
GBUFFER_PLANES = ("diffuse", "normal", "roughness", "metalness", "emissive")
SLOTS = ("depth", "gbuffer", "velocity", "direct_light")  # abi.TEX_DEPTH .. abi.TEX_DIRECT_LIGHT, the order of every slot list below
CLEAR = np.array([0, 0, 0, 0x3f800000], np.uint32)
# the plane subsets rfx_stage_aov accepts that the form tests run
SUBSETS = {
    "all": NAMES,
    "depth": ("depth",),
    "depth_direct": ("depth", "direct"),
    "depth_velocity_normal": ("depth", "velocity", "normal"),
    "gbuffer_depth": GBUFFER_PLANES + ("depth",),
    "no_direct": tuple(k for k in NAMES if k != "direct"),
}
F16, F32 = np.float16, np.float32


def mask_of(names):
    return sum(BIT[k] for k in set(names))


def names_of(mask):
    return tuple(k for k in NAMES if mask & BIT[k])


def submasks(given):
    """every half mask over the planes of `given` (a mask), ascending"""
    return [m for m in range(256) if not m & ~given]


def select(given, halves):
    """rfx_launch_k0_aov's rule restated, for the segment that reads every plane the frame gives (masks over NAMES): no half plane -> SET 0;
    exactly the given planes but velocity and depth -> SET 1; any other mix -> SET 2.  (A row tile's segments outside the held rows read depth
    alone: SET 0 or 2 by depth's type.)"""
    halves &= given
    if halves == 0:
        return 0
    if halves == given & ~(BIT["velocity"] | BIT["depth"]):
        return 1
    return 2


def written(names):
    """which of SLOTS a frame with these planes writes (include/rfx.h "streamed AOV frames")"""
    s = set(names)
    return (True, set(GBUFFER_PLANES) <= s, "velocity" in s, "direct" in s)


# ---------------------------------------------------------------- staged / widened planes, the reference, the synchronous importer
def stage(halves, mask=0, diffuse_ch=4, direct_ch=4, subset=NAMES):
    """`halves`: {name: float16 array of full channel count} -> what is staged: the planes of `subset`, float16 where `mask` says so and the
    same values as float32 elsewhere, diffuse / direct cut to their channel counts"""
    out = {}
    for k in subset:
        v = halves[k]
        assert v.dtype == F16
        ch = dict(diffuse=diffuse_ch, direct=direct_ch).get(k, CHANNELS[k])
        v = v[..., :ch] if v.ndim == 3 else v
        out[k] = np.ascontiguousarray(v if mask & BIT[k] else v.astype(F32))
    return out


def widen(staged):
    """the staged planes as float32 planes of full channel count: a 3-channel diffuse or direct gets alpha 1"""
    out = {}
    for k, v in staged.items():
        w = v.astype(F32)
        if k in ("diffuse", "direct") and w.shape[-1] == 3:
            w = np.concatenate([w, np.ones(w.shape[:2] + (1,), F32)], -1)
        out[k] = np.ascontiguousarray(w)
    return out


def reference(planes):
    """widened float32 planes -> [DEPTH, GBUFFER, VELOCITY, DIRECT_LIGHT] as the C restatement packs them (None: the planes do not name the slot)"""
    import rfx_oracle as O
    p = widen(planes)
    assert all(v.dtype == F32 for v in planes.values())
    w = written(p)
    return [p["depth"], O.pack_gbuffer(p, p["depth"]) if w[1] else None, O.pack_velocity(p, p["depth"]) if w[2] else None, p["direct"] if w[3] else None]


def sync_import(ctx, wide):
    """the synchronous importer (rfx_pack_gbuffer + rfx_pack_velocity + rfx_upload) on whole-frame float32 planes, for the slots the planes
    name and the rows the context holds of each"""
    from rfx_amd import abi
    r0, n = ctx.held_rows(abi.TEX_GBUFFER)
    band = {k: v[r0:r0 + n] for k, v in wide.items()}
    w = written(wide)
    if w[1]:
        ctx.pack_gbuffer(band, band["depth"], r0, n)
    if w[2]:
        ctx.pack_velocity(band, band["depth"], r0, n)
    ctx.upload(abi.TEX_DEPTH, wide["depth"])
    if w[3]:
        ctx.upload(abi.TEX_DIRECT_LIGHT, band["direct"], r0, n)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def differing(got, want):
    """[messages], one per slot whose bytes differ; `want` entries that are None are not compared"""
    out = []
    for i, (a, b) in enumerate(zip(got, want)):
        if b is None:
            continue
        a, b = bits(a), bits(b)
        if a.shape != b.shape:
            out.append("%s: shape %s != %s" % (SLOTS[i], a.shape, b.shape))
            continue
        bad = (a != b).reshape(a.shape[0], a.shape[1], -1).any(-1)
        if bad.any():
            y, x = (int(v[0]) for v in np.nonzero(bad))
            out.append("%s: %d texels differ, first at row %d x %d: got %s want %s" % (
                SLOTS[i], int(bad.sum()), y, x, ["%08x" % v for v in np.atleast_1d(a[y, x])], ["%08x" % v for v in np.atleast_1d(b[y, x])]))
    return out


# ---------------------------------------------------------------- 1. every half value through every role
EVERY_W = EVERY_H = 256
LAYOUTS = (0, 1, 2)  # the emissive maximum in r, g, b; each layout also moves the one background pixel
_MULT = (1, 40503, 25173, 13849, 30893, 52429, 9377)   # odd: p -> (p * m + a) mod 2^16 permutes the bit patterns
_ADD = (0, 0x1234, 0x8765, 0x4321, 0x0f0f, 0x3c3c, 0x5a5a)
_EXP = 0x7c00


def _perm(j):
    p = np.arange(65536, dtype=np.uint32)
    return ((p * _MULT[j] + _ADD[j]) & 0xffff).astype(np.uint16)


def is_finite(b):
    return (b & _EXP) != _EXP


def is_nan(b):
    return ((b & _EXP) == _EXP) & ((b & 0x3ff) != 0)


def colour_domain(b):
    """finite and non-negative, or -0"""
    return is_finite(b) & (((b & 0x8000) == 0) | (b == 0x8000))


def emissive_domain(b):
    """finite and > 0"""
    return is_finite(b) & ((b & 0x8000) == 0) & (b != 0)


def _half(b):
    return np.ascontiguousarray(b, np.uint16).view(F16)


def every_half_frame(layout=0):
    """256 x 256 halves, pixel p = 256 y + x carries the bit pattern p (and fixed permutations of it in the further channels):
    diffuse, roughness, metalness: the pattern where it is in colour_domain, else 0.5; emissive: maximum half(p) where p is in emissive_domain, with
    half(p) / 2 (computed in half) and 0 beside it, rotated by `layout`, black elsewhere; normal: three finite halves (an inf / NaN pattern has
    its top exponent bit cleared), (1, y, z) where all three are zero; velocity, depth, direct: every non-NaN pattern (NaN: 0.5).  The depth
    plane is a permutation that depends on the layout, so the one background pixel (pattern 0x3c00) hides another pixel in each."""
    assert layout in LAYOUTS
    shape = (EVERY_H, EVERY_W)
    col = lambda j: np.where(colour_domain(_perm(j)), _half(_perm(j)), F16(0.5))   # noqa: E731
    raw = lambda j: np.where(is_nan(_perm(j)), F16(0.5), _half(_perm(j)))           # noqa: E731
    fin = lambda j: _half(np.where(is_finite(_perm(j)), _perm(j), _perm(j) & 0xbfff))  # noqa: E731
    p = _perm(0)
    mx = np.where(emissive_domain(p), _half(p), F16(0))
    em = [mx, mx * F16(0.5), np.zeros_like(mx)]
    em = em[-layout:] + em[:-layout] if layout else em
    n = np.stack([fin(2), fin(3), fin(0)], -1)
    n[(n == 0).all(-1), 0] = 1
    out = dict(diffuse=np.stack([col(j) for j in range(4)], -1), normal=n, roughness=col(0), metalness=col(1), emissive=np.stack(em, -1),
               velocity=np.stack([raw(0), raw(1)], -1), depth=raw(4 + layout), direct=np.stack([raw(j) for j in range(4)], -1))
    out = {k: np.ascontiguousarray(v.astype(F16).reshape(shape + v.shape[1:])) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


EVERY_KINDS = {"f16": ALL, "typed": TYPED, "f32": 0}  # SET 2 (depth and velocity are halves too), SET 1, SET 0


# ---------------------------------------------------------------- random frames of halves (sections 2 and 3)
def random_planes(W, H, seed):
    """a frame inside the domain: colours in [0, 1), emissive black on a quarter of the texels, about one texel in seven background (at
    least one of each kind where the frame has two texels)"""
    rng = np.random.RandomState(seed)
    h = lambda *s: rng.rand(*s).astype(F16)  # noqa: E731
    p = dict(diffuse=h(H, W, 4), normal=h(H, W, 3) - F16(0.5), roughness=h(H, W), metalness=h(H, W),
             emissive=(rng.rand(H, W, 3) * np.array([6, 3, 1])).astype(F16), velocity=h(H, W, 2) - F16(0.5),
             depth=h(H, W) * F16(0.5) + F16(0.25), direct=(rng.rand(H, W, 4) * np.array([4, 2, 1, 1])).astype(F16))
    p["normal"][(p["normal"] == 0).all(-1), 0] = 1
    p["emissive"][rng.rand(H, W) < 0.25] = 0
    p["depth"][rng.rand(H, W) < 0.15] = 1
    if W * H >= 2:
        d = p["depth"].reshape(-1)
        d[(W * H - 1) // 2] = 1
        d[-1] = 0.5  # (the last pixel — a tail pixel where there is a tail — is foreground)
    for v in p.values():
        v.setflags(write=False)
    return p


# ---------------------------------------------------------------- 2. every plane form
FORM_W, FORM_H = 7, 3  # 21 pixels: five groups and a tail of one, in one workgroup
FORM_CHANNELS = list(itertools.product((3, 4), (3, 4)))  # (diffuse, direct)


def form_frame(i):
    """the two 7 x 3 frames the form cases alternate between (a slot a case does not name must keep the OTHER frame's bytes)"""
    return random_planes(FORM_W, FORM_H, 0x7a0 + i)


def form_cases():
    """{group: [(subset name, half mask, diffuse channels, direct channels)]}: the channel counts under the three plain masks; all 256 masks
    with 3 / 3 and with 4 / 4 channels; every plane subset under every mask over its planes, with 3 / 3 and with 4 / 4"""
    g = {"channels": [("all", m, d, q) for d, q in FORM_CHANNELS for m in (0, TYPED, ALL)]}
    for ch in (3, 4):
        g["masks_%d%d" % (ch, ch)] = [("all", m, ch, ch) for m in range(256)]
    for name, planes in SUBSETS.items():
        if name != "all":
            g[name] = [(name, m, ch, ch) for ch in (3, 4) for m in submasks(mask_of(planes))]
    return g


FORM_GROUPS = tuple(form_cases())
# diffuse with three channels on frames with other tails, and on the row tiles of test_gpu_stage_aov.test_bands_and_row_tiles (W, H, y0, rows, halo)
DIFFUSE3_FRAMES = [(97, 55, None), (5, 3, None), (96, 54, (20, 18, 4)), (97, 55, (21, 17, 4)), (97, 55, (0, 21, 2)), (97, 55, (41, 14, 3))]


# ---------------------------------------------------------------- 3. segment shapes
TINY_FRAMES = [(1, 1), (3, 1), (1, 3), (2, 2)]
TINY_TILE = (1, 9, 3, 3, 0)  # W, H, y0, rows, halo: three segments of three pixels


def held(H, y0, rows, halo):
    """the rows GBUFFER / VELOCITY / DIRECT_LIGHT hold on a row tile"""
    a = max(y0 - halo, 0)
    return a, min(y0 + rows + halo, H) - a


def random_tilings(n=60):
    """seeded cases: a frame, a row tile, the frame's rows cut into 1..4 bands staged in a random order, a half mask, channel counts, a subset"""
    rng = np.random.RandomState(0x0a0b)
    names = list(SUBSETS)
    out = []
    for i in range(n):
        W, H = int(rng.randint(1, 71)), int(rng.randint(2, 41))
        y0 = int(rng.randint(0, H))
        rows = int(rng.randint(1, H - y0 + 1))
        halo = int(rng.randint(0, 6))
        calls = int(rng.randint(1, min(4, H) + 1))
        cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, H), calls - 1, replace=False)) + [H]
        bands = [(a, b - a) for a, b in zip(cuts, cuts[1:])]
        bands = [bands[j] for j in rng.permutation(len(bands))]
        out.append(dict(W=W, H=H, y0=y0, rows=rows, halo=halo, bands=bands, mask=int(rng.randint(0, 256)), diffuse_ch=3 + int(rng.randint(2)),
                        direct_ch=3 + int(rng.randint(2)), subset=names[int(rng.randint(len(names)))], seed=0x900 + i))
    return out
