"""Test helper (numpy only): cameras, settings, engine-form frames and the comparison of the AOV convention tests
(tests/test_aov_conventions_cpu.py, tests/test_gpu_aov_conventions.py, tests/test_node_aov_conventions.py).

A setting is the plain dict tests/aov_convention_ref.py reads; `host` turns it into the product's rfx_amd.conventions.AovConventions.  The
cameras are built here in float64 (three.js makePerspective / makeOrthographic / lookAt), rounded to the float32 elements a host dumps, and
velocityMatrix = projectionMatrix x matrixWorldInverse is formed from those float32 elements in float64 in multiplyMatrices' order, then
rounded: `three_product` restates what rfx_amd.conventions.multiply_matrices must give."""
import itertools
import math

import numpy as np

import aov_cases as AC

F = np.float32
DEPTH_KINDS = ("fragcoord", "view_z", "position")
VELOCITY_KINDS = ("uv", "scaled", "cameras")
NORMAL_SPACES = ("world", "view")
COMBINATIONS = list(itertools.product(range(3), range(3), range(2)))
FORMS = {"f32": 0, "f16": AC.ALL, "typed": AC.TYPED}       # half masks over aov_cases.NAMES: SET 0, SET 2, SET 1
# (W, H, tile): tail only; no tail; tail 1 and groups that wrap a row; a row tile whose whole-frame band gives all three segments
SHAPES = [(3, 1, None), (64, 4, None), (37, 5, None), (5, 7, (2, 3, 1))]
BACKGROUND = (0.0, 0.0, 0.0)


def _col32(m):
    return np.ascontiguousarray(np.asarray(m, np.float64).T.reshape(16)).astype(F)


def three_product(a, b):
    """float32[16] x float32[16] (column-major) -> float32[16]: Matrix4.multiplyMatrices in float64, rounded once"""
    a, b = [float(v) for v in a], [float(v) for v in b]
    out = np.zeros(16, F)
    for col in range(4):
        for row in range(4):
            s = a[row] * b[4 * col] + a[4 + row] * b[4 * col + 1] + a[8 + row] * b[4 * col + 2] + a[12 + row] * b[4 * col + 3]
            out[4 * col + row] = F(s)
    return out


def camera(frame, perspective=True, aspect=16 / 9):
    """-> dict(P, Pi, C, V float32[16], near, far, perspective): an orbiting camera, another pose per frame"""
    ang = math.radians(25.0 + 2.0 * frame)
    eye = np.array([7.5 * math.cos(ang), 2.8 + 0.05 * frame, 7.5 * math.sin(ang)])
    z = eye - np.array([0.0, 0.8, 0.0])
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    mw = np.eye(4)
    mw[:3, 0], mw[:3, 1], mw[:3, 2], mw[:3, 3] = x, y, z, eye
    if perspective:
        n, f = 0.1, 60.0
        t = n * math.tan(math.radians(20.0))
        r = t * aspect
        p = np.array([[n / r, 0, 0, 0], [0, n / t, 0, 0], [0, 0, -(f + n) / (f - n), -2 * f * n / (f - n)], [0, 0, -1, 0]])
    else:
        n, f = 0.5, 20.0
        t = 3.0
        r = t * aspect
        p = np.array([[1 / r, 0, 0, 0], [0, 1 / t, 0, 0], [0, 0, -2 / (f - n), -(f + n) / (f - n)], [0, 0, 0, 1]])
    return dict(P=_col32(p), Pi=_col32(np.linalg.inv(p)), C=_col32(mw), V=_col32(np.linalg.inv(mw)), near=n, far=f, perspective=perspective)


def setting(depth_kind, velocity_kind, normal_space, perspective=True, frame=3, scale=(1.0 / 64, -1.0 / 32), background=BACKGROUND):
    cam, prev = camera(frame, perspective), camera(frame - 1, perspective)
    return dict(depth_kind=depth_kind, velocity_kind=velocity_kind, normal_space=normal_space, perspective=perspective,
                scale=tuple(float(F(s)) for s in scale), near=cam["near"], far=cam["far"], background=background,
                VM=three_product(cam["P"], cam["V"]), PVM=three_product(prev["P"], prev["V"]), P=cam["P"], Pi=cam["Pi"], C=cam["C"], camera=cam, prev_camera=prev)


def host(conv):
    """the setting as the product's hosts take it"""
    from rfx_amd.conventions import AovConventions
    return AovConventions(depth_kind=DEPTH_KINDS[conv["depth_kind"]], velocity_kind=VELOCITY_KINDS[conv["velocity_kind"]],
                          normal_space=NORMAL_SPACES[conv["normal_space"]], perspective=conv["perspective"], velocity_scale=conv["scale"],
                          near=conv["near"], far=conv["far"], velocityMatrix=conv["VM"], prevVelocityMatrix=conv["PVM"], projectionMatrix=conv["P"],
                          projectionMatrixInverse=conv["Pi"], cameraMatrixWorld=conv["C"], background_position=conv["background"])


def _world_from_view(cam, pv):
    c = cam["C"].astype(np.float64).reshape(4, 4).T
    return pv @ c[:3, :3].T + c[:3, 3]


def engine_frame(W, H, conv, seed, edges=True):
    """A frame of HALVES (every value a half, so that one frame serves every plane form; aov_cases.stage picks the types) in the setting's
    conventions: aov_cases.random_planes with the depth plane as the kind wants it — a gl_FragCoord.z, a positive view distance, or a world
    position (H, W, 3) of a point in front of the camera —, no velocity plane under CAMERAS.  About one texel in seven is not covered.
    edges: the coverage edges are written over the first texels (as many as the frame has room for) — +inf, -inf, NaN, 0, a negative value,
    behind the camera, beyond far, in front of near, the background position."""
    rng = np.random.RandomState(seed)
    base = AC.random_planes(W, H, seed)
    p = {k: np.array(v) for k, v in base.items()}
    cam = conv["camera"]
    n, f = cam["near"], cam["far"]
    dist = n + (f - n) * rng.rand(H, W) ** 2 * 0.6 + 0.05      # the distance along the camera axis: inside (near, far)
    lateral = (rng.rand(H, W, 2) - 0.5) * (dist[..., None] * 0.5 if cam["perspective"] else 4.0)
    pv = np.concatenate([lateral, -dist[..., None]], -1)
    uncovered = np.array(base["depth"]).astype(F) == 1.0
    dk = conv["depth_kind"]
    edge_values = []
    if dk == 1:
        z = dist.astype(np.float16)
        z[uncovered] = np.inf
        edge_values = [np.inf, -np.inf, np.nan, 0.0, -2.0, f * 1.5, n * 0.25]
        flat = z.reshape(-1)
        for i, v in enumerate(edge_values[:max(0, flat.size - 2)] if edges else []):
            flat[i] = v
        p["depth"] = z
    elif dk == 2:
        w = _world_from_view(cam, pv).astype(np.float16)
        w[uncovered] = BACKGROUND
        flat = w.reshape(-1, 3)
        behind = _world_from_view(cam, np.array([0.3, 0.2, 2.0]))
        beyond = _world_from_view(cam, np.array([0.0, 0.0, -f * 1.5]))
        front = _world_from_view(cam, np.array([0.0, 0.0, -n * 0.25]))
        ok = flat[-1].astype(np.float64)
        edge_values = [(np.inf, ok[1], ok[2]), (ok[0], -np.inf, ok[2]), (ok[0], ok[1], np.nan), tuple(behind), tuple(beyond), tuple(front), BACKGROUND]
        for i, v in enumerate(edge_values[:max(0, flat.shape[0] - 2)] if edges else []):
            flat[i] = v
        p["depth"] = w
    # (FRAGCOORD: random_planes' own depth plane, 1.0 where not covered)
    if conv["velocity_kind"] == 2:
        del p["velocity"]
    elif conv["velocity_kind"] == 1:
        p["velocity"] = ((rng.rand(H, W, 2) - 0.5) * 40).astype(np.float16)  # pixels
    for v in p.values():
        v.setflags(write=False)
    return p


def stage(frame, form):
    """the frame as a host stages it: float16 where the form's half mask says so"""
    mask = FORMS[form]
    return {k: np.ascontiguousarray(v if mask & AC.BIT[k] else v.astype(F)) for k, v in frame.items()}


def reference(staged, conv, W, H):
    """staged engine-form planes of the whole frame -> [DEPTH, GBUFFER, VELOCITY, DIRECT_LIGHT]: the restatement's conversion, then the C
    restatement's packers (aov_cases.reference)"""
    import aov_convention_ref as R
    return AC.reference(R.convert(staged, conv, W, H))


def _nan_class(bits):
    """0: finite; 1: +inf; 2: -inf; 3: NaN"""
    e = (bits & 0x7f800000) == 0x7f800000
    nan = e & ((bits & 0x7fffff) != 0)
    return np.where(nan, 3, np.where(e, np.where(bits >> 31 != 0, 2, 1), 0))


def differing(got, want):
    """aov_cases.differing, with the header's rule for a non-finite velocity: the x and y words of a VELOCITY texel are equal when both are
    non-finite of the same class"""
    got, want = list(got), list(want)
    if got[2] is not None and want[2] is not None and np.shape(got[2]) == np.shape(want[2]):
        g, w = AC.bits(got[2]).copy(), AC.bits(want[2])
        for ch in (0, 1):
            cg, cw = _nan_class(g[..., ch]), _nan_class(w[..., ch])
            same = (cg == cw) & (cg != 0)
            g[..., ch] = np.where(same, w[..., ch], g[..., ch])
        got[2] = g
    return AC.differing(got, want)


def held(H, tile):
    """the rows GBUFFER / VELOCITY / DIRECT_LIGHT hold on a context with this tile (y0, rows, halo)"""
    if tile is None:
        return 0, H
    y0, n, halo = tile
    a, b = max(0, y0 - halo), min(H, y0 + n + halo)
    return a, b - a


def cut(full, H, tile):
    """whole-frame slots -> what the context holds of each: DEPTH whole, the others their held rows"""
    r0, n = held(H, tile)
    return [full[0]] + [None if a is None else a[r0:r0 + n] for a in full[1:]]
