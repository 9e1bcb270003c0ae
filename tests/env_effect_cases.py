"""What tests/test_gpu_env_effect.py and tests/test_node_env_device.py share: a 96 x 54 three-frame sequence whose scene.environment is either a
cube that is replaced before the second frame or a HalfFloatType equirectangular map with flipY, driven by the Python host with and without
env_on_device.  The Python runs are computed once per process."""
import functools
import types

import numpy as np

from rfx_amd import abi, effect
from rfx_amd.context import Context
from rfx_amd.scene import synthetic_frame

W, H, FRAMES = 96, 54, 3
OPTIONS = dict(width=W, height=H, steps=8, refineSteps=2)
SEEDS = dict(ssgi=11, denoise=22)
CUBE_SIZE, EQUIRECT = 8, (64, 32)
OUTPUTS = (("compose", abi.TEX_COMPOSE), ("ssgi", abi.TEX_SSGI), ("final", abi.TEX_FINAL))


@functools.lru_cache(maxsize=None)
def frames():
    return tuple(synthetic_frame(W, H, i) for i in range(FRAMES))


@functools.lru_cache(maxsize=None)
def cube_faces(k):
    """two different cubes of seeded HDR values: k = 0 lights frame 0, k = 1 frames 1 and 2"""
    a = (10.0 ** np.random.RandomState(50 + k).uniform(-2.0, 1.5, (6, CUBE_SIZE, CUBE_SIZE, 4))).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def equirect():
    a = (10.0 ** np.random.RandomState(60).uniform(-3.0, 2.0, (EQUIRECT[1], EQUIRECT[0], 4))).astype(np.float32)
    a[:EQUIRECT[1] // 2] *= np.float32(0.05)  # a dim lower half: the lossy un-flip of flipY changes the tables
    a.setflags(write=False)
    return a


def environment(kind, frame_index):
    """the scene.environment the frame is drawn with: a NEW object where it changes, None where the previous one stays"""
    if kind == "cube":
        return dict(isCubeTexture=True, faces=cube_faces(frame_index)) if frame_index < 2 else None
    return dict(data=equirect(), flipY=True) if frame_index == 0 else None


@functools.lru_cache(maxsize=None)
def python_run(kind, on_device):
    """{name: array} of the last frame, and the number of environment updates that went each way"""
    fs = frames()
    scene = types.SimpleNamespace(frame=fs[0], environment=None)
    cam = types.SimpleNamespace(**vars(fs[0].camera))
    fx = effect.SSGIEffect(None, scene, cam, dict(OPTIONS), seeds=dict(SEEDS), half_store_rtz=True, env_on_device=on_device)
    ctx = Context(W, H)
    calls = []
    for name in ("set_environment_cube", "build_environment_importance", "cube_to_equirect", "set_environment_importance"):
        def spy(*a, _f=getattr(ctx, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        setattr(ctx, name, spy)
    for i, f in enumerate(fs):
        scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        env = environment(kind, i)
        if env is not None:
            scene.environment = env
        fx.update(ctx, None)
    ctx.final_compose(fx.uniforms)
    out = {name: ctx.download(tex) for name, tex in OUTPUTS}
    ctx.close()
    return out, tuple(calls)
