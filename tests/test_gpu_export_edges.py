"""GPU (-m gpu; also under --hostsim): K7 at the edges of its launch plan.  tests/test_gpu_export.py runs 15, 5335 and 9216 pixels (pixels mod 4
= 3, 3 and 0); here the frames of export_cases.EDGE_SIZES leave a tail of one or two pixels behind the dword-store body (the u8 and f16
element-wide stores), have no body at all (1 and 2 pixels), or put the tail's lane alone into a second block (1025 pixels: groups == 256).
The three checks are the ones of tests/test_gpu_export.py: F32 bit for bit, F16 against numpy, U8_SRGB under the margin rule, cap included."""
import numpy as np
import pytest

import export_cases as X
from rfx_amd import abi
from rfx_amd.context import Context
from test_gpu_export import SOURCES, _bits

pytestmark = pytest.mark.gpu

SIZE_IDS = ["%dx%d" % s for s in X.EDGE_SIZES]


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size", X.EDGE_SIZES, ids=SIZE_IDS)
def test_f32_is_the_sources_bits(size, channels):
    W, H = size
    ctx = Context(W, H)
    for k, src in enumerate(SOURCES):
        ctx.upload(src, _bits(W, H, 300 + k))
    for src in SOURCES:
        got = ctx.export(src, "f32", channels)
        assert got.dtype == np.float32 and got.shape == (H, W, channels)
        assert ctx.export_bytes(ctx.export_params(src, "f32", channels)) == got.nbytes == W * H * channels * 4
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ctx.download(src)[..., :channels]).view(np.uint32)), abi.TEX_NAMES[src]
    ctx.close()


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size", X.EDGE_SIZES, ids=SIZE_IDS)
def test_f16_rounds_like_numpy(size, channels):
    W, H = size
    a = X.f16_edge_input(W, H)
    ctx = Context(W, H)
    ctx.upload(abi.TEX_EFFECT_INPUT, a)
    got = ctx.export(abi.TEX_EFFECT_INPUT, "f16", channels)
    ctx.close()
    assert got.shape == (H, W, channels)
    X.check_f16(got, a, channels)


@pytest.mark.parametrize("case", X.edge_u8_cases(), ids=X.case_id)
def test_u8_srgb_meets_the_margin_rule(case):
    """the cap of 1 % holds on these inputs down to one pixel (tests/test_export_edges_cpu.py: no byte of the three smallest frames lies
    within DELTA of a boundary), so the rule is export_cases.check_margin's, unchanged"""
    W, H, channels, family, exposure, operator = case
    a = X.linear_input(W, H, family, planted=W * H >= 64)
    v, ref = X.reference_v(a, channels, operator, exposure)
    ctx = Context(W, H)
    ctx.upload(abi.TEX_FINAL, a)
    got = ctx.export(abi.TEX_FINAL, "u8_srgb", channels, operator, exposure)
    ctx.close()
    X.check_margin(got, v, ref)
