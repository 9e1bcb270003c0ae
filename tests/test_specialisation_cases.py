"""CPU: the case tables of tests/test_gpu_specialisations.py against the launchers' full cross products (tests/specialisations.py).  Every
case's inputs must select the kernel the case is named after — K1's table layout and K3's tile plan asked of the library as built
(tests/launch_plans.py: the host-simulator build's rfx_internal_k1_table / rfx_internal_k3_tile) — and the keys of each table must be exactly
the cross product: a template argument added to a launcher, or a frame that no longer plans the way its case says, fails here."""
import pytest

import specialisations as SP
import test_gpu_specialisations as T
from launch_plans import k3_pass0_layouts, needs_hostsim


@pytest.fixture(scope="module")
def plans():
    """every plan the tables ask for, from two child processes"""
    p = SP.Plans()
    p.prime_k1(T.K1_FRAME.values())
    cases = []
    for key, frame, tag in T.K3_CASES + [(k, f, "") for k, f in T.K3_LAYOUT_CASES]:
        dp, W, H, _ = T.k3_inputs(key, frame, tag)
        cases.append((W, H, dp.radius, dp.inputIsTemporal, dp.textureCount))
    p.prime_k3(cases)
    return p


@needs_hostsim
def test_k1_cases_select_their_kernels_and_cover_the_cross_product(plans):
    keys = []
    for key in T.K1_CASES:
        sp, W, H, entry = T.k1_inputs(key)
        assert SP.k1_key(plans, sp, W, H, entry) == key
        keys.append(key)
    assert sorted(keys) == sorted(SP.K1_KEYS) and len(set(keys)) == 54
    # the frames are the ones the table layouts were made for: plain rows fit and padded rows do not (rfx_launch.h rfx_k1_table)
    W, H = T.K1_FRAME[0]
    t = plans.k1(W, H)
    assert (t["pow2"], t["cell_shift"], t["pitch"], t["cells_h"]) == (0, 4, (W + 15) // 16, 577) and 16 * t["cells_h"] > 9216
    y0, y1 = T.K1_WINDOW
    assert 0 < y0 < y1 < H and y0 % 8 != 0
    assert plans.k1(*T.K1_FRAME[1])["pow2"] == 1
    # the three projections are told apart by the matrix alone: the view offset moves elements 8 and 9 only
    centred, offset, ortho = (list(T.k1_inputs(("k1", p, 1, 0, "march"))[0].camera.projectionMatrix) for p in ("centred", "perspective", "general"))
    assert [i for i in range(16) if centred[i] != offset[i]] == [8, 9] and centred[8] == centred[9] == 0.0
    assert ortho[11] == 0.0 and ortho[15] == 1.0


def test_k2_cases_select_their_kernels_and_cover_the_cross_product():
    keys = []
    for key in T.K2_CASES:
        tp, whole = T.k2_inputs(key)
        assert SP.k2_key(tp, whole) == key
        assert tp.textureCount == (2 if tp.inputType == 0 else 1)  # the three (inputType, textureCount) pairs rfx_launch_k2 accepts
        keys.append(key)
    assert sorted(keys) == sorted(SP.K2_KEYS) and len(set(keys)) == 24


def test_k0_aov_cases_select_their_kernels_and_cover_the_cross_product():
    keys = []
    for key in T.K0_AOV_CASES:
        staged = T.k0_aov_inputs(key)
        assert SP.k0_aov_key(staged) == key and len(staged) == 8  # (a whole frame: every plane is given)
        keys.append(key)
    assert sorted(keys) == sorted(SP.K0_AOV_KEYS) and len(set(keys)) == 3
    assert [SP.key_id(k) for k in SP.K0_AOV_KEYS] == ["k0_aov-set0", "k0_aov-set1", "k0_aov-set2"]


@needs_hostsim
def test_k3_cases_select_their_kernels_and_cover_the_cross_product(plans):
    keys = set()
    for key, frame, tag in T.K3_CASES:
        dp, W, H, whole = T.k3_inputs(key, frame, tag)
        assert SP.k3_key(plans, dp, W, H, whole) == key, (key, frame, tag)
        keys.add(key)
    assert keys == set(SP.K3_KEYS) and len(keys) == 44
    assert sorted(k for k, _, tag in T.K3_CASES if not tag) == sorted(SP.K3_KEYS)  # one unnamed case per kernel
    # one more case per pitch on a frame with an interior tile column
    wide = [(k, f) for k, f, tag in T.K3_CASES if tag == "wide"]
    assert {k[3] for k, _ in wide} == set(SP.PITCHES) and all(f[0] >= 130 for _, f in wide)
    # a row-tiled case must leave its two tiles bands, not the frame: the halo the test draws with stays under the other tile's rows
    from rfx_amd import tiling
    assert sorted(k for k, _, tag in T.K3_CASES if tag == "tiles") == sorted(SP.K3_GENERIC_KEYS)  # k3_generic on row tiles: the same kernel, rebased rows
    for key, (W, H, radius), tag in T.K3_CASES:
        if (key[0] == "k3_tiled" and key[4] == 0) or tag == "tiles":
            assert all(rows + tiling.required_halo(radius, 0.0, H, W) < H for _, rows in tiling.split_rows(H, 2))


@needs_hostsim
def test_k3_layout_cases_are_every_layout_the_sweep_selects(plans):
    """frames of up to 260 x 200 texels, radii 0 ... 8, through rfx_internal_k3_tile: the (pitch, skip) pairs that come back are the cases"""
    swept = k3_pass0_layouts(**SP.LAYOUT_SWEEP)
    keys = set()
    for key, frame in T.K3_LAYOUT_CASES:
        dp, W, H, whole = T.k3_inputs(key, frame)
        assert (dp.inputIsTemporal, dp.textureCount, whole) == (1, 2, True)
        assert SP.k3_layout(plans, dp, W, H) == key, (key, frame)
        keys.add(key)
    assert keys == {("layout", p, s) for p, s in swept} and len(keys) == len(T.K3_LAYOUT_CASES)
    assert {p for p, _ in swept} == set(SP.PITCHES) and {s for _, s in swept} == {0, 2, 4}  # (an odd skip never survives the alignment loop)
