"""CPU (-m "not gpu"): the premises of tests/test_gpu_export_edges.py.  K7's launch plan, as built, at the pixel counts of
export_cases.EDGE_SIZES — the tails of 1 and 2 pixels, no body at all, and at 1025 pixels the tail's lane alone in a second block — and the
share of bytes the margin rule excuses on those inputs, with the fp32 emulation of tests/test_export_cpu.py held to the rule."""
import numpy as np
import pytest

import export_cases as X
from rfx_amd import abi
from test_export_cpu import BLOCK, _fp32_chain, _plan


def test_edge_sizes_are_the_tails_the_suite_lacked():
    assert [w * h for (w, h) in X.EDGE_SIZES] == [1, 2, 6, 1025, 1025]
    assert [w * h % 4 for (w, h) in X.EDGE_SIZES] == [1, 2, 2, 1, 1]
    assert {w * h % 4 for (w, h) in X.SIZES} == {3, 0}  # what tests/test_gpu_export.py runs


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("fmt", [abi.EXPORT_F32, abi.EXPORT_F16, abi.EXPORT_U8_SRGB])
def test_export_plan_at_the_edge_sizes(fmt, ch):
    for pixels, groups, blocks, tail in ((1, 0, 1, 1), (2, 0, 1, 2), (6, 1, 1, 2), (1025, 256, 2, 1)):
        p = _plan(pixels, fmt, ch)
        assert (p.groups, p.blocks, p.tail_pixels, p.tail_start) == (groups, blocks, tail, 4 * groups), pixels
        assert p.bytes == pixels * p.pixel_bytes == groups * p.group_bytes + tail * p.pixel_bytes
    p = _plan(1025, fmt, ch)
    assert p.blocks == 2 and p.tail_pixels == 1
    assert p.groups % BLOCK == 0 and p.groups // BLOCK == p.blocks - 1  # lane t == groups is lane 0 of the last block, alone in it
    assert _plan(1024, fmt, ch).blocks == 1 and _plan(1027, fmt, ch).blocks == 2


@pytest.mark.parametrize("case", X.edge_u8_cases(), ids=X.case_id)
def test_share_excused_by_the_margin_rule(case):
    W, H, channels, family, exposure, operator = case
    a = X.linear_input(W, H, family, planted=W * H >= 64)
    v, ref = X.reference_v(a, channels, operator, exposure)
    share = float(X.excluded(v).mean())
    print("%s: excused share %.5f of %d bytes" % (X.case_id(case), share, v.size))
    assert share <= X.SHARE_CAP  # (a frame of 1, 2 or 6 pixels holds 3 to 24 bytes: the cap holds there because none is excused)
    if W * H < 64:
        assert share == 0.0
    X.check_margin(_fp32_chain(a, channels, operator, exposure), v, ref)


def test_f16_edge_inputs_hold_planted_values():
    for (W, H) in X.EDGE_SIZES:
        a = X.f16_edge_input(W, H)
        assert a.shape == (H, W, 4) and a.dtype == np.float32
        assert np.isnan(a.reshape(-1)[0]) and np.isinf(a.reshape(-1)[1])  # the first texel, whichever lane stores it
