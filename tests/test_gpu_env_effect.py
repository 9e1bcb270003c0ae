"""SSGIEffect(..., env_on_device=True) through the Python host: the composed output of a 96 x 54 three-frame run — a cube environment that is
replaced before the second frame; a HalfFloatType equirectangular map with flipY — is byte-identical to the default (host) path's, and the
environment updates did go the device's way."""
import pytest

import env_effect_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["cube", "equirect_flipY"])
def test_env_on_device_equals_the_default_path(kind):
    host, host_calls = C.python_run(kind, False)
    dev, dev_calls = C.python_run(kind, True)
    for name, _ in C.OUTPUTS:
        assert dev[name].tobytes() == host[name].tobytes(), name
        assert (host[name] != 0).any(), name
    if kind == "cube":
        assert host_calls == ("cube_to_equirect", "set_environment_importance") * 2
        assert dev_calls == ("set_environment_cube", "build_environment_importance") * 2
    else:
        assert host_calls == ("set_environment_importance",) and dev_calls == ("build_environment_importance",)


def test_the_environments_matter():
    """the two cubes light the frame differently, and so does the map's flipY (or the comparisons above would be vacuous)"""
    import types

    from rfx_amd import abi, effect
    from rfx_amd.context import Context
    f = C.frames()[0]
    outs = []
    for env in (dict(isCubeTexture=True, faces=C.cube_faces(0)), dict(isCubeTexture=True, faces=C.cube_faces(1)), dict(data=C.equirect(), flipY=True), dict(data=C.equirect())):
        scene = types.SimpleNamespace(frame=f, environment=env)
        fx = effect.SSGIEffect(None, scene, types.SimpleNamespace(**vars(f.camera)), dict(C.OPTIONS), seeds=dict(C.SEEDS), half_store_rtz=True, env_on_device=True)
        ctx = Context(C.W, C.H)
        fx.update(ctx, None)
        outs.append(ctx.download(abi.TEX_SSGI))
        ctx.close()
    assert outs[0].tobytes() != outs[1].tobytes() and outs[2].tobytes() != outs[3].tobytes()
