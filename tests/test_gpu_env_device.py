"""scene.environment kept on the device (include/rfx.h "the environment kept on the device"): K10's tables and sums against the host builder, bit for
bit, over the sizes and contents of tests/env_cases.py; rfx_set_environment_cube against the two-call form, level by level; K1 on the golden MIS
frame with device-built tables; a sequence of environment updates with a draw after each and no host synchronisation between them, the old and
the new entry points mixed; the error returns.  Runs on the device and under --hostsim."""
import functools
import struct

import numpy as np
import pytest

import env_cases as E
import golden_util as G
from rfx_amd import abi
from rfx_amd.context import Context, RfxError
from rfx_amd.envmap import build_importance
from rfx_amd.scene import synthetic_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(16, 16)
    assert c.has_env_device
    yield c
    c.close()


def same_bits(got, want, what):
    for name, g, w in zip(("marginal", "conditional"), got[:2], want[:2]):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %s differs in %d entries" % (what, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()))
    assert struct.pack("<d", got[2]) == struct.pack("<d", want[2]), "%s: totalSumValue %r != %r" % (what, got[2], want[2])
    assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes(), "%s: whole / decimal %r %r != %r %r" % (what, got[3], got[4], want[3], want[4])


@pytest.mark.parametrize("size", E.SIZES, ids=lambda s: "%dx%d" % s)
def test_tables_and_sums_equal_the_host_builder(ctx, size):
    W, H = size
    for content in E.CONTENTS:
        for half in (True, False):
            ctx.set_environment(E.texels(W, H, content), half_float_type=half, half_store_rtz=True)
            assert ctx.download_environment(0, size).tobytes() == E.stored(W, H, content, half).tobytes()  # K10's input: no second conversion
            for flip in (0, 1):
                ctx.build_environment_importance(bool(flip))
                same_bits(ctx.download_environment_importance(), E.reference(W, H, content, half, flip), "%dx%d %s half=%s flipY=%d" % (W, H, content, half, flip))


def cube(seed, size):
    """six faces of seeded HDR values"""
    rs = np.random.RandomState(seed)
    return (10.0 ** rs.uniform(-3.0, 2.0, (6, size, size, 4))).astype(np.float32)


@pytest.mark.parametrize("mipmaps", [True, False])
@pytest.mark.parametrize("which", ["cube_32", "5x5"])
def test_cube_path_equals_the_two_call_form(ctx, which, mipmaps):
    faces, size = (np.ascontiguousarray(G.load("cube_32")["faces"], np.float32), (128, 64)) if which == "cube_32" else (cube(5, 5), (32, 16))
    ctx.set_environment(ctx.cube_to_equirect(faces, size[0], size[1], generate_mipmaps=mipmaps), half_float_type=False, half_store_rtz=False)
    n = ctx.environment_levels()
    want = [ctx.download_environment(l, size) for l in range(n)]
    ctx.set_environment(None)
    mine = faces.copy()
    ctx.set_environment_cube(mine, size[0], size[1], generate_mipmaps=mipmaps)
    mine[:] = -1.0  # the caller may reuse the buffer on return
    assert ctx.environment_levels() == n == int(np.log2(size[0])) + 1
    for l in range(n):
        assert ctx.download_environment(l, size).tobytes() == want[l].tobytes(), "level %d" % l
    assert (want[0] != 0).any()


def ssgi_params(cam, steps, refine, index):
    return abi.SsgiParams(camera=abi.Camera.from_scene(cam), steps=steps, refineSteps=refine, mode=0, useDirectLight=1, rayDistance=10, thickness=10, envBlur=0.5,
                          blueNoiseIndex=index, useEnvMap=1, importanceSampling=1)


def test_chain_k1_with_device_built_tables():
    """the golden MIS frame's inputs: K1's output with K10's tables is K1's output with the host's"""
    g = G.load(G.GOLDEN_ENVMIS)
    W, H = int(g["width"]), int(g["height"])
    envimg = np.ascontiguousarray(g["environment"], np.float32)
    f = G.frame(g, 0)
    sp = ssgi_params(f.camera, int(g["steps"]), int(g["refineSteps"]), int(g["f0_ssgi_index"]))
    c = Context(W, H)
    c.set_environment(envimg, half_float_type=True, half_store_rtz=True)
    c.upload_frame(f)
    c.upload(abi.TEX_COMPOSE, np.zeros((H, W, 4), np.float32))
    c.set_environment_importance(*build_importance(c.download_environment(0, envimg.shape[1::-1])))
    c.ssgi_march(sp)
    want = c.download(abi.TEX_SSGI)
    c.clear(abi.TEX_SSGI)
    c.build_environment_importance(False)
    c.ssgi_march(sp)
    got = c.download(abi.TEX_SSGI)
    m, cw, total, _, _ = c.download_environment_importance()
    c.close()
    assert got.tobytes() == want.tobytes() and (want != 0).any()
    assert m.tobytes() == np.ascontiguousarray(g["marginalWeights"], np.float32).tobytes() and total == float(g["totalSumValue"])
    assert cw.tobytes() == np.ascontiguousarray(g["conditionalWeights"], np.float32).tobytes()


# ---- a sequence of updates, a draw after each
FW, FH, BAND = 64, 40, 8
SEQUENCE = [(11, (64, 32)), (12, (64, 32)), (13, (64, 32)), (14, (128, 64)), (11, (64, 32))]  # (cube seed, target): three maps, a larger one, the first again


@functools.lru_cache(maxsize=None)
def frame_and_history():
    return synthetic_frame(FW, FH, 0), np.random.RandomState(4).rand(FH, FW, 4).astype(np.float32)


def prepared_context():
    f, hist = frame_and_history()
    c = Context(FW, FH)
    c.upload_frame(f)
    c.upload(abi.TEX_COMPOSE, hist)
    return c, ssgi_params(f.camera, 8, 2, 321)


@functools.lru_cache(maxsize=None)
def old_way(seed, size):
    """the draw of a fresh context given that environment by the blocking calls and the host builder"""
    c, sp = prepared_context()
    eq = c.cube_to_equirect(cube(seed, 8), size[0], size[1], generate_mipmaps=True)
    c.set_environment(eq, half_float_type=False, half_store_rtz=False)
    c.set_environment_importance(*build_importance(eq))
    c.ssgi_march(sp)
    out = c.download(abi.TEX_SSGI)
    c.close()
    assert (out != 0).any()
    out.setflags(write=False)
    return out


def set_old(c, seed, size, tables):
    eq = c.cube_to_equirect(cube(seed, 8), size[0], size[1], generate_mipmaps=True)
    c.set_environment(eq, half_float_type=False, half_store_rtz=False)
    if tables == "host":
        c.set_environment_importance(*build_importance(eq))
    else:
        c.build_environment_importance(False)


def set_new(c, seed, size, tables):
    c.set_environment_cube(cube(seed, 8), size[0], size[1], generate_mipmaps=True)
    if tables == "host":
        c.set_environment_importance(*build_importance(c.download_environment(0, size)))
    else:
        c.build_environment_importance(False)


@pytest.mark.parametrize("plan", ["device", "mixed"])
def test_update_sequence(plan):
    """Every update is followed by a draw of its own band of rows (rfx_set_row_window), so that all five results are read at the end: in the
    `device` plan nothing between the first update and the last draw synchronises with the host."""
    steps = {"device": [(set_new, "device")] * 5,
             "mixed": [(set_new, "device"), (set_old, "host"), (set_new, "host"), (set_old, "device"), (set_new, "device")]}[plan]
    c, sp = prepared_context()
    c.sync()
    for k, ((seed, size), (setter, tables)) in enumerate(zip(SEQUENCE, steps)):
        setter(c, seed, size, tables)
        c.set_row_window(k * BAND, (k + 1) * BAND)
        c.ssgi_march(sp)
    got = c.download(abi.TEX_SSGI)
    c.close()
    for k, (seed, size) in enumerate(SEQUENCE):
        rows = slice(k * BAND, (k + 1) * BAND)
        assert got[rows].tobytes() == old_way(seed, size)[rows].tobytes(), "draw %d (%s)" % (k, plan)
    assert old_way(*SEQUENCE[0]).tobytes() != old_way(*SEQUENCE[1]).tobytes()  # the environments do light the frame differently


def test_errors():
    c, sp = prepared_context()
    with pytest.raises(RfxError, match=r"\(%d\)" % abi.RFX_ESTATE):
        c.build_environment_importance()
    faces = cube(3, 4)
    for w, h in ((96, 32), (64, 48), (0, 32), (64, 0), (32768, 64)):
        with pytest.raises(RfxError, match=r"\(%d\)" % abi.RFX_EINVAL):
            c.set_environment_cube(faces, w, h)
    assert c.lib.rfx_set_environment_cube(c._h, faces.ctypes.data, 0, 1, 64, 32) == abi.RFX_EINVAL
    assert c.lib.rfx_set_environment_cube(c._h, faces.ctypes.data, 8193, 1, 64, 32) == abi.RFX_EINVAL
    assert c.lib.rfx_set_environment_cube(c._h, None, 4, 1, 64, 32) == abi.RFX_EINVAL
    assert c.environment_levels() == 0  # nothing was set by the refused calls
    c.set_environment_cube(faces, 64, 32)
    c.build_environment_importance()
    c.ssgi_march(sp)
    c.set_environment_cube(faces, 64, 32)  # a new map invalidates the tables
    with pytest.raises(RfxError, match=r"\(%d\)" % abi.RFX_ESTATE):
        c.ssgi_march(sp)
    with pytest.raises(RfxError, match=r"\(%d\)" % abi.RFX_ESTATE):
        c.download_environment_importance()
    c.build_environment_importance()
    c.ssgi_march(sp)
    c.set_environment(None)
    with pytest.raises(RfxError, match=r"\(%d\)" % abi.RFX_ESTATE):
        c.build_environment_importance()
    c.close()
