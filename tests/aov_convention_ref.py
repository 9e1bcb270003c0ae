"""Test helper: the arithmetic of include/rfx.h "AOV conventions" restated — element-wise float32 numpy, every multiply and add written out in
the header's order, no matrix product.  It shares no code with the device functions (csrc/k0_import.hip k0_conv_*) or with the host conversion
(rfx_amd.imageio.aov_to_reference_conventions); both are held to it bit for bit.

A setting here is a plain dict (tests/aov_convention_cases.py builds them):
    depth_kind 0 / 1 / 2 (FRAGCOORD, VIEW_Z, POSITION), velocity_kind 0 / 1 / 2 (UV, SCALED, CAMERAS), normal_space 0 / 1 (WORLD, VIEW),
    perspective, scale (2 floats), near, far, background (3 floats or None),
    VM, PVM, P, Pi, C: float32[16], column-major — velocityMatrix, prevVelocityMatrix, projectionMatrix, its inverse, cameraMatrixWorld.
`convert` turns engine-form planes of a band into the reference-form depth / velocity / normal planes the packers take."""
import numpy as np

F = np.float32
HALF, TWO, ONE = F(0.5), F(2.0), F(1.0)


def _f32(a):
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float16), a.dtype
    return a.astype(F)  # (a half widens exactly)


def mul(M, x, y, z):
    """mul(M, p)_i = ((M[0][i] x + M[1][i] y) + M[2][i] z) + M[3][i]"""
    M = np.asarray(M, F)
    r0 = M[0] * x
    r0 = r0 + M[4] * y
    r0 = r0 + M[8] * z
    r0 = r0 + M[12]
    r1 = M[1] * x
    r1 = r1 + M[5] * y
    r1 = r1 + M[9] * z
    r1 = r1 + M[13]
    r2 = M[2] * x
    r2 = r2 + M[6] * y
    r2 = r2 + M[10] * z
    r2 = r2 + M[14]
    r3 = M[3] * x
    r3 = r3 + M[7] * y
    r3 = r3 + M[11] * z
    r3 = r3 + M[15]
    return r0, r1, r2, r3


def frag_coord_z(cz, cw):
    q = HALF * cz
    q = q / cw
    return q + HALF


def depth_to_view_z(depth, near, far, perspective):
    """three.js perspectiveDepthToViewZ / orthographicDepthToViewZ"""
    n, f = F(near), F(far)
    if perspective:
        num = n * f
        den = (f - n) * depth
        den = den - f
        return num / den
    t = depth * (n - f)
    return t - n


def view_position(P, Pi, u, v, view_z):
    """getViewPosition (ssgi_utils.frag:17-24): -> (x, y, view_z)"""
    P, Pi = np.asarray(P, F), np.asarray(Pi, F)
    clip_w = P[11] * view_z
    clip_w = clip_w + P[15]
    cx = (u - HALF) * TWO
    cx = cx * clip_w
    cy = (v - HALF) * TWO
    cy = cy * clip_w
    cz = (view_z - HALF) * TWO
    cz = cz * clip_w
    cw = ONE * clip_w
    x = Pi[0] * cx
    x = x + Pi[4] * cy
    x = x + Pi[8] * cz
    x = x + Pi[12] * cw
    y = Pi[1] * cx
    y = y + Pi[5] * cy
    y = y + Pi[9] * cz
    y = y + Pi[13] * cw
    return x, y, view_z


def convert(planes, conv, W, H, row0=0):
    """planes: name -> array of the band's rows (row `row0` of the W x H frame first), float32 or float16; the depth plane under "depth" whatever
    its kind.  -> the same dict with float32 reference-form "depth", "velocity" (where the kind gives one), "normal"; the rest widened."""
    out = {k: _f32(v) for k, v in planes.items()}
    d = out["depth"]
    dk, vk = conv["depth_kind"], conv["velocity_kind"]
    with np.errstate(all="ignore"):
        world = None
        view_z = None
        if dk == 2:
            assert d.ndim == 3 and d.shape[2] == 3
            x, y, z = d[..., 0], d[..., 1], d[..., 2]
            n0, n1, n2, n3 = mul(conv["VM"], x, y, z)
            fz = frag_coord_z(n2, n3)
            covered = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
            if conv.get("background") is not None:
                b = [F(t) for t in conv["background"]]
                covered = covered & ~((x == b[0]) & (y == b[1]) & (z == b[2]))
            covered = covered & (n3 > F(0)) & (fz >= F(0)) & (fz < ONE)
            depth = np.where(covered, fz, ONE).astype(F)
            world = (x, y, z)
        elif dk == 1:
            assert d.ndim == 2
            P = np.asarray(conv["P"], F)
            view_z = -d
            cz = P[10] * view_z
            cz = cz + P[14]
            cw = P[11] * view_z
            cw = cw + P[15]
            fz = frag_coord_z(cz, cw)
            covered = np.isfinite(d) & (d > F(0)) & (fz >= F(0)) & (fz < ONE)
            depth = np.where(covered, fz, ONE).astype(F)
        else:
            assert d.ndim == 2
            depth = d
        out["depth"] = np.ascontiguousarray(depth)
        rows = depth.shape[0]
        assert depth.shape[1] == W
        if vk == 1:
            v = out["velocity"]
            s = [F(t) for t in conv["scale"]]
            out["velocity"] = np.ascontiguousarray(np.stack([v[..., 0] * s[0], v[..., 1] * s[1]], -1).astype(F))
        elif vk == 2:
            assert "velocity" not in planes
            if world is None:
                if view_z is None:
                    view_z = depth_to_view_z(d, conv["near"], conv["far"], conv["perspective"])
                xs = np.arange(W).astype(F)
                ys = np.arange(row0, row0 + rows).astype(F)
                u = ((xs + HALF) / F(W))[None, :]
                v = ((ys + HALF) / F(H))[:, None]
                px, py, pz = view_position(conv["P"], conv["Pi"], u, v, view_z)
                w0, w1, w2, _ = mul(conv["C"], px, py, pz)
                world = (w0, w1, w2)
            n0, n1, n2, n3 = mul(conv["VM"], *world)
            p0, p1, p2, p3 = mul(conv["PVM"], *world)
            pos0x = (p0 / p3) * HALF
            pos0x = pos0x + HALF
            pos0y = (p1 / p3) * HALF
            pos0y = pos0y + HALF
            pos1x = (n0 / n3) * HALF
            pos1x = pos1x + HALF
            pos1y = (n1 / n3) * HALF
            pos1y = pos1y + HALF
            vel = np.stack([pos1x - pos0x, pos1y - pos0y], -1).astype(F)
            out["velocity"] = np.ascontiguousarray(np.broadcast_to(vel, (rows, W, 2)))
        if conv["normal_space"] == 1 and "normal" in out:
            n = out["normal"]
            C = np.asarray(conv["C"], F)
            nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
            wx = C[0] * nx
            wx = wx + C[4] * ny
            wx = wx + C[8] * nz
            wy = C[1] * nx
            wy = wy + C[5] * ny
            wy = wy + C[9] * nz
            wz = C[2] * nx
            wz = wz + C[6] * ny
            wz = wz + C[10] * nz
            out["normal"] = np.ascontiguousarray(np.stack([wx, wy, wz], -1).astype(F))
    return out
