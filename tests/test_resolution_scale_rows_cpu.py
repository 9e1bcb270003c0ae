"""CPU (-m "not gpu"): resolutionScale < 1 on row tiles without a device.  The row plan rfx_launch.h rfx_scaled_rows as the library computes it
(tests/scaled_rows_plan.py: the host-simulator build's rfx_internal_scaled_rows) against a brute force over the frame rows K2 stages, under
both vUv models; the halo term 2 + ceil(1 / (2 s)) of required_halo(resolution_scale=s) against the source row of every target row a tile
draws; the Python and the Node required_halo; and the default argument against the values of the parent commit."""
import json
import math
import os
import shutil
import subprocess

import pytest

import scaled_rows_plan as P
from rfx_amd import tiling

HERE = os.path.dirname(os.path.abspath(__file__))
JS = os.path.join(os.path.dirname(HERE), "realism-effects_amd", "js")
node = shutil.which("node")

SCALES = (0.5, 0.75, 0.25, 0.125, 0.3125)  # every one exact in binary: H * s is whole exactly when the product says so
HEIGHTS = range(16, 401)
AP = 2  # K2's apron (k2_temporal.hip): the rows its neighbourhood clamp reads around a tile


def _tilings(H):
    for n in range(2, 9):
        try:
            yield from tiling.split_rows(H, n)
        except ValueError:  # tiles of fewer than 2 rows
            return


def _k1_halo(s):
    return 2 + int(math.ceil(1.0 / (2.0 * s)))


@P.needs_hostsim
def test_scaled_rows_plan_equals_the_rows_k2_stages_and_the_halo_term_covers_their_sources():
    """For every H in 16..400, every scale with whole H * s, every tile of every split_rows tiling for 2..8 ranks and both vUv models:
    (a) [j0, j1) of the library is exactly the set of target rows iy(gy) = nearest(vUv.y(gy) * Hs) over the frame rows gy K2 stages for the
        tile, [y0 - 2, y1 - 1 + 2] clipped to the frame — no row missing (K2 would read an undrawn row), none extra (the slot is sized for the band);
    (b) the source row nearest(vUv_target.y(j) * H) of every drawn target row j — where K1 fetches the G-buffer and the direct light through the
        band views — lies inside the tile widened by 2 + ceil(1 / (2 s)) rows, the K1 term of required_halo, and required_halo returns at least that.
    W = 2 H: the reference GL's plane equation depends on the width too; both W * s and H * s are then whole together."""
    cases, want, checks = [], [], 0
    worst = {}
    for H in HEIGHTS:
        W = 2 * H
        for model in (P.UV_IDEAL, P.UV_REFERENCE_GL):
            vf = P.frag_v(model, W, H)
            for s in SCALES:
                if (H * s) != int(H * s):
                    continue
                Hs, Ws = int(H * s), int(W * s)
                iy = P.nearest_idx(vf, Hs).tolist()
                sy = P.nearest_idx(P.frag_v(model, Ws, Hs), H).tolist()
                k1 = _k1_halo(s)
                assert tiling.required_halo(0.0, 0.0, H, W, resolution_scale=s) >= k1
                for y0, rows in _tilings(H):
                    y1 = y0 + rows
                    staged = range(max(0, y0 - AP), min(H - 1, y1 - 1 + AP) + 1)
                    rows_read = sorted({iy[gy] for gy in staged})
                    assert rows_read == list(range(rows_read[0], rows_read[-1] + 1)), (H, s, model, y0, y1)  # no gap: a range describes it
                    cases.append((W, H, Hs, model, y0, y1, AP))
                    want.append((rows_read[0], rows_read[-1] + 1))
                    for j in rows_read:
                        d = max(max(0, y0 - AP) - sy[j], sy[j] - min(H - 1, y1 - 1 + AP), 0)  # rows beyond what K2 stages
                        worst[(s, model)] = max(worst.get((s, model), 0), d)
                        assert max(0, y0 - k1) <= sy[j] < min(H, y1 + k1), "H %d scale %g model %d tile [%d, %d): target row %d reads frame row %d, %d rows of halo" % (
                            H, s, model, y0, y1, j, sy[j], k1)
                        checks += 1
    got = P.scaled_rows(cases)
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, "%d of %d plans differ from the brute force, first (W, H, Hs, model, y0, y1, apron) -> library, brute force: %s" % (len(bad), len(cases), bad[:3])
    print("%d plans, %d source rows checked; rows beyond K2's staged range by (scale, model): %s" % (len(cases), checks, sorted(worst.items())))
    assert len(cases) > 5000


@P.needs_hostsim
def test_scaled_rows_plan_at_the_frame_edges_and_with_a_smaller_apron():
    """the whole frame as one tile draws every target row; apron 0 (a context without halo rows) draws what the tile's own rows address"""
    cases = [(400, 200, 100, m, 0, 200, a) for m in (0, 1) for a in (0, 2)] + [(264, 132, 33, m, 44, 88, 0) for m in (0, 1)]
    got = P.scaled_rows(cases)
    assert got[:4] == [(0, 100)] * 4
    for (W, H, Hs, m, y0, y1, a), g in zip(cases[4:], got[4:]):
        iy = P.nearest_idx(P.frag_v(m, W, H), Hs).tolist()
        assert g == (iy[y0], iy[y1 - 1] + 1)


# required_halo(radius, max |v_y|, H, W) of the parent commit (resolution_scale did not exist): the default leaves them as they were
PARENT_HALO = [((3.0, 0.0, 132, 200), 5), ((3.0, 0.01, 132, 200), 6), ((5.0, 0.0, 2160, 3840), 7), ((3.0, 0.02, 2160, 3840), 48), ((0.0, 0.0, 64, 64), 4),
               ((3.0, 0.0, 200, 120), 7), ((12.0, 0.0, 4320, 7680), 14), ((3.0, 0.0031, 4320, 7680), 18), ((1.0, 0.0, 16, None), 4),
               ((8.0, 0.05, 1080, None), 58)]


def test_required_halo_default_is_unchanged_and_the_scale_term_is_the_k1_term():
    for args, want in PARENT_HALO:
        assert tiling.required_halo(*args) == want, args
        assert tiling.required_halo(*args, resolution_scale=1.0) == want, args
    # the K1 term: 2 + ceil(1 / (2 s)); it decides only when it exceeds K2's 4 and K3's radius + 2
    assert [_k1_halo(s) for s in SCALES] == [3, 3, 4, 6, 4]
    assert tiling.required_halo(0.0, 0.0, 128, 256, resolution_scale=0.125) == 6
    assert tiling.required_halo(0.0, 0.0, 128, 256, resolution_scale=0.0625) == 10
    assert tiling.required_halo(3.0, 0.0, 132, 200, resolution_scale=0.5) == 5


@pytest.mark.skipif(node is None, reason="node not installed")
def test_node_required_halo_agrees_with_python():
    cases = [list(a) + [s] for a, _ in PARENT_HALO for s in (None, 1.0) + SCALES + (0.0625,)]
    js = ("const t=require(%r);const c=JSON.parse(process.argv[1]);"
          "console.log(JSON.stringify(c.map(a=>t.requiredHalo(a[0],a[1],a[2],a[3]===null?undefined:a[3],a[4]===null?undefined:a[4]))))" % os.path.join(JS, "tiling"))
    got = json.loads(subprocess.check_output([node, "-e", js, json.dumps(cases)], text=True))
    want = [tiling.required_halo(*c[:4]) if c[4] is None else tiling.required_halo(*c[:4], resolution_scale=c[4]) for c in cases]
    assert got == want
