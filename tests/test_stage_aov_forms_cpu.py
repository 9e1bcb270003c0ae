"""CPU (-m "not gpu") side of tests/test_gpu_stage_aov_forms.py: the premises of the generators of tests/aov_cases.py — the domains hold, every
half value and every power of two is where the device test says it is, the case lists reach every specialisation the selection rule allows,
the random tilings cover their frames once — and a run of the device file on the host simulator."""
import os
import subprocess
import sys

import numpy as np

import aov_cases as AC
from launch_plans import needs_hostsim
from rfx_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def test_every_half_frame_premises():
    every = np.arange(65536, dtype=np.uint16)
    finite_pos = every[AC.emissive_domain(every)]
    assert finite_pos.size == 0x7bff
    hidden = []
    for layout in AC.LAYOUTS:
        p = AC.every_half_frame(layout)
        assert set(p) == set(AC.NAMES) and all(v.dtype == np.float16 and v.shape[:2] == (256, 256) for v in p.values())
        assert all(v.shape[2:] == ((AC.CHANNELS[k],) if AC.CHANNELS[k] > 1 else ()) for k, v in p.items())
        wide = AC.widen(AC.stage(p))
        assert not any(np.isnan(v).any() for v in wide.values())  # no NaN is staged
        # colour inputs: finite and >= 0, or -0; every such half occurs in every channel
        colours = every[AC.colour_domain(every)]
        for k in ("diffuse", "roughness", "metalness"):
            planes = _bits(p[k]).reshape(65536, -1)
            assert AC.colour_domain(planes).all()
            for c in range(planes.shape[1]):
                assert np.array_equal(np.unique(planes[:, c]), colours), (k, c)
        assert 0x8000 in colours and 0x7bff in colours and 1 in colours and 0x8001 not in colours and 0x7c00 not in colours
        # emissive: black, or finite with a positive maximum in channel `layout`; every finite positive half is a maximum, the others are max / 2 and 0
        e = wide["emissive"].reshape(-1, 3)
        mx = e.max(-1)
        assert np.isfinite(e).all() and (e >= 0).all() and ((mx > 0) | (e == 0).all(-1)).all()
        lit = mx > 0
        assert (e[lit, layout] == mx[lit]).all()
        assert np.array_equal(np.unique(_bits(p["emissive"]).reshape(-1, 3)[lit, layout]), finite_pos)
        assert np.array_equal(np.sort(e[lit], -1)[:, 0], np.zeros(int(lit.sum()), np.float32))
        assert np.array_equal(np.sort(e[lit], -1)[:, 1], (mx[lit].astype(np.float16) * np.float16(0.5)).astype(np.float32))
        powers = np.array([2.0 ** k for k in range(-24, 16)], np.float32)
        assert np.isin(powers, mx).all() and powers.size == 40
        # normals: finite, never the zero vector; z takes every finite half, +-0 among them
        n = wide["normal"].reshape(-1, 3)
        assert np.isfinite(n).all() and (n != 0).any(-1).all()
        z = np.unique(_bits(p["normal"])[..., 2])
        assert np.array_equal(z, every[AC.is_finite(every)]) and 0 in z and 0x8000 in z
        # velocity, depth, direct: every pattern but the NaNs
        not_nan = every[~AC.is_nan(every)]
        for k in ("velocity", "depth", "direct"):
            planes = _bits(p[k]).reshape(65536, -1)
            for c in range(planes.shape[1]):
                assert np.array_equal(np.unique(planes[:, c]), not_nan), (k, c)
        bg = np.flatnonzero(_bits(p["depth"]).reshape(-1) == 0x3c00)
        assert bg.size == 1 and (wide["depth"] == 1.0).sum() == 1
        hidden.append(int(bg[0]))
    assert len(set(hidden)) == 3  # the background pixel hides another pixel's values in each layout
    # the three ways the frame is staged select the three specialisations, and `reference` runs
    assert [AC.select(AC.ALL, AC.EVERY_KINDS[k]) for k in ("f16", "typed", "f32")] == [2, 1, 0]
    ref = AC.reference(wide)
    assert [a.shape for a in ref] == [(256, 256), (256, 256, 4), (256, 256, 4), (256, 256, 4)] and ref[1].dtype == np.uint32
    at = np.unravel_index(hidden[-1], (256, 256))
    assert (ref[1][at] == AC.CLEAR).all() and (ref[2][at] == AC.CLEAR).all()
    assert int((ref[1] == AC.CLEAR).all(-1).sum()) == 1


def test_selection_rule_and_form_cases():
    B = AC.BIT
    assert AC.NAMES == abi.AOV_PLANES
    assert AC.select(AC.ALL, 0) == 0 and AC.select(AC.ALL, AC.TYPED) == 1 and AC.select(AC.ALL, AC.ALL) == 2
    assert AC.select(AC.ALL, AC.TYPED & ~B["normal"]) == 2 and AC.select(AC.ALL, B["depth"]) == 2
    assert AC.select(B["depth"], AC.ALL) == 2 and AC.select(B["depth"], AC.TYPED) == 0            # depth alone: SET 1 means SET 0
    assert AC.select(B["depth"] | B["direct"], B["direct"] | B["normal"]) == 1                      # a bit of a plane not given does not count
    groups = AC.form_cases()
    assert tuple(groups) == AC.FORM_GROUPS and set(groups) == {"channels", "masks_33", "masks_44"} | (set(AC.SUBSETS) - {"all"})
    assert {k: len(v) for k, v in groups.items()} == dict(channels=12, masks_33=256, masks_44=256, depth=4, depth_direct=8, depth_velocity_normal=16,
                                                          gbuffer_depth=128, no_direct=256)
    assert sorted(m for _, m, d, q in groups["masks_33"]) == list(range(256)) and {(d, q) for _, _, d, q in groups["channels"]} == set(AC.FORM_CHANNELS)
    for name, cases in groups.items():
        reached = set()
        for subset, mask, d, q in cases:
            given = AC.mask_of(AC.SUBSETS[subset])
            assert not mask & ~given and d in (3, 4) and q in (3, 4)
            staged = AC.stage(AC.form_frame(0), mask, d, q, AC.SUBSETS[subset])
            assert set(staged) == set(AC.SUBSETS[subset]) and {k for k, v in staged.items() if v.dtype == np.float16} == set(AC.names_of(mask))
            if "diffuse" in staged:
                assert staged["diffuse"].shape[-1] == d
            if "direct" in staged:
                assert staged["direct"].shape[-1] == q
            reached.add(AC.select(given, mask))
        # every subset reaches every SET the rule allows: with depth alone the typed set is empty, so SET 1 is SET 0
        assert reached == ({0, 2} if name == "depth" else {0, 1, 2}), name
        if name not in ("channels", "masks_33", "masks_44"):
            assert sorted(m for _, m, d, _ in cases if d == 3) == AC.submasks(AC.mask_of(AC.SUBSETS[name]))
    # the frame: five groups and a tail of one; the tail pixel and a group pixel are foreground, and three channels change their texels
    assert AC.FORM_W * AC.FORM_H == 21
    frames = [AC.form_frame(i) for i in range(3)]
    for i, f in enumerate(frames):
        d = f["depth"].reshape(-1).astype(np.float32)
        assert d[20] < 1.0 and (d[:20] == 1.0).any() and (d[:20] < 1.0).any()
        r4, r3 = (AC.reference(AC.widen(AC.stage(f, 0, ch, ch))) for ch in (4, 3))
        for k in (1, 3):
            differs = (AC.bits(r4[k]) != AC.bits(r3[k])).any(-1).reshape(-1)
            assert differs[20] and differs[:20].any(), (i, k)
        assert AC.bits(r4[0]).tobytes() == AC.bits(r3[0]).tobytes() and r4[2].tobytes() == r3[2].tobytes()
        for g in frames[:i]:
            assert len(AC.differing(AC.reference(AC.widen(AC.stage(f))), AC.reference(AC.widen(AC.stage(g))))) == 4
    # the subsets are frames rfx_stage_aov accepts
    for name, planes in AC.SUBSETS.items():
        w = AC.written(planes)
        assert "depth" in planes and w[0] and (w[1] or not set(planes) & (set(AC.GBUFFER_PLANES) - {"normal"}))
        assert ("normal" in planes) == (w[1] or w[2])
    assert [AC.written(AC.SUBSETS[k]) for k in ("depth", "depth_direct", "depth_velocity_normal", "gbuffer_depth", "no_direct")] == [
        (True, False, False, False), (True, False, False, True), (True, False, True, False), (True, True, False, False), (True, True, True, False)]


def test_random_planes_stay_in_the_domain():
    for W, H, seed in [(1, 1, 0x100), (2, 1, 3), (3, 1, 0x101), (7, 3, 0x7a0), (96, 54, 0x51), (97, 55, 0x3d)]:
        p = AC.random_planes(W, H, seed)
        wide = AC.widen(AC.stage(p))
        assert all(np.isfinite(v).all() for v in wide.values())
        assert all((wide[k] >= 0).all() for k in ("diffuse", "roughness", "metalness", "emissive"))
        assert (wide["normal"] != 0).any(-1).all()
        if W * H >= 2:
            assert (wide["depth"] == 1.0).any() and wide["depth"].reshape(-1)[-1] < 1.0
        if W * H > 100:
            assert (wide["emissive"] == 0).all(-1).any() and (wide["emissive"].max(-1) > 0).any()
        assert AC.widen(AC.stage(p, AC.ALL))["diffuse"].tobytes() == wide["diffuse"].tobytes()  # the mask changes the type, not the values
        d3 = AC.widen(AC.stage(p, AC.ALL, 3, 3))
        assert (d3["diffuse"][..., 3] == 1).all() and (d3["direct"][..., 3] == 1).all() and d3["diffuse"][..., :3].tobytes() == wide["diffuse"][..., :3].tobytes()
        assert [a is not None for a in AC.reference(AC.widen(AC.stage(p, 0, 4, 4, AC.SUBSETS["depth_velocity_normal"])))] == [True, False, True, False]


def test_segment_shape_premises():
    for W, H in AC.TINY_FRAMES:
        assert W * H < 4 or (W * H) % 4 == 0  # tail only, or one group and no tail
    W, H, y0, n, halo = AC.TINY_TILE
    h0, hn = AC.held(H, y0, n, halo)
    assert [W * r for r in (h0, hn, H - h0 - hn)] == [3, 3, 3]
    # the row tiles of the 3-channel diffuse: some segment starts at a texel that is no multiple of four
    tiles = [(W, H) + t for W, H, t in AC.DIFFUSE3_FRAMES if t]
    assert len(tiles) == 4 and sum((AC.held(H, y0, n, halo)[0] * W) % 4 != 0 for W, H, y0, n, halo in tiles) >= 2
    assert {(W * H) % 4 for W, H, t in AC.DIFFUSE3_FRAMES if not t} == {3}
    ts = AC.random_tilings()
    assert len(ts) == 60 and ts == AC.random_tilings()
    outside = 0
    seen_sets, seen_subsets, calls = set(), set(), set()
    for t in ts:
        W, H = t["W"], t["H"]
        assert 1 <= W <= 70 and 2 <= H <= 40 and 0 <= t["y0"] and t["rows"] >= 1 and t["y0"] + t["rows"] <= H and t["halo"] >= 0
        covered = np.zeros(H, int)
        h0, hn = AC.held(H, t["y0"], t["rows"], t["halo"])
        for r0, n in t["bands"]:
            assert n >= 1
            covered[r0:r0 + n] += 1
            outside += r0 + n <= h0 or r0 >= h0 + hn
        assert (covered == 1).all() and 1 <= len(t["bands"]) <= 4
        calls.add(len(t["bands"]))
        seen_sets.add(AC.select(AC.mask_of(AC.SUBSETS[t["subset"]]), t["mask"]))
        seen_subsets.add(t["subset"])
    assert outside >= 10 and calls == {1, 2, 3, 4} and seen_subsets == set(AC.SUBSETS) and {0, 2} <= seen_sets
    assert {t["diffuse_ch"] for t in ts} == {3, 4} and {t["direct_ch"] for t in ts} == {3, 4}
    assert any([b[0] for b in t["bands"]] != sorted(b[0] for b in t["bands"]) for t in ts)  # (bands out of order)


@needs_hostsim
def test_gpu_files_on_the_host_simulator():
    """tests/test_gpu_stage_aov_forms.py and the K0 AOV pack cases of tests/test_gpu_specialisations.py with the host simulator's library in
    place of the device's"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    env = {k: v for k, v in os.environ.items() if k not in ("RFX_HOSTSIM", "RFX_TEST_LIB")}
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "--hostsim", "-p", "no:cacheprovider",
                        os.path.join(HERE, "test_gpu_stage_aov_forms.py"), os.path.join(HERE, "test_gpu_specialisations.py") + "::test_k0_aov"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert " passed" in p.stdout and "skipped" not in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]
