"""The N-API addon's marshalling of the seven parameter structs, on the CPU: `paramBytes(kind, object)` returns the struct exactly as the
corresponding call passes it to the C ABI (napi/rfx_napi.c: one field table per struct, one reader).

  full object      every field set to a distinct value that is no default -> the bytes of the rfx_amd.abi ctypes struct filled with the same
                   values: names, order, types and sizes against the Python host (which test_abi_and_host pins to include/rfx.h)
  smallest object  what the call needs at least (its cameras, motionBlur's `resolution`) -> a struct built from DEFAULTS, the literal table below:
                   the third arguments of the prop_num calls the addon had before it read the structs from tables

One node process serves every case.
"""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess

import pytest

from rfx_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
node = shutil.which("node")
pytestmark = pytest.mark.skipif(node is None, reason="node not installed")
ADDON = os.path.join(HERE, "..", "realism-effects_amd", "napi", "rfx_napi.node")

STRUCTS = {"ssgi": abi.SsgiParams, "temporal": abi.TemporalParams, "denoise": abi.DenoiseParams, "compose": abi.ComposeParams, "final": abi.FinalParams,
           "motionBlur": abi.MotionBlurParams, "export": abi.ExportParams}
CAMERA_JS = {"near_": "near", "far_": "far", "isPerspective": "isPerspectiveCamera"}  # the camera object carries three's names
CAMERA_REQUIRED = ("projectionMatrix", "projectionMatrixInverse", "matrixWorld", "matrixWorldInverse", "position")
NAN_SIGNED = 0xFFC00000  # the bits of the host's 0.0 / 0.0 as a float
# every field the object may leave out, with what the struct then holds (a float given as an int: the bits of the float)
DEFAULTS = {
    "camera": dict(near_=0.1, far_=1000.0, isPerspective=1),
    "ssgi": dict(steps=20, refineSteps=5, mode=0, useDirectLight=0, missedRays=0, importanceSampling=0, useEnvMap=0, rayDistance=10.0, thickness=10.0,
                 envBlur=0.5, blueNoiseIndex=0, resolutionScale=1.0, historySource=0),
    "temporal": dict(textureCount=2, inputType=0, reprojectSpecular=(0, 0), neighborhoodClamp=(0, 0), logTransform=0, fullAccumulate=0, confidencePower=0.75,
                     neighborhoodClampIntensity=1.0, maxBlend=1.0, keepData=1.0, historySource=0, targetHalf=0, halfStoreRTZ=1, inputWidth=0, inputHeight=0),
    "denoise": dict(radius=3.0, phi=0.5, lumaPhi=5.0, depthPhi=2.0, normalPhi=3.25, roughnessPhi=NAN_SIGNED, specularPhi=NAN_SIGNED, textureCount=2,
                    isTextureSpecular=(0, 0), blueNoiseIndex=0, inputIsTemporal=1, writeToB=0, halfStoreRTZ=0),
    "compose": dict(inputType=0, giSource=0, writeHistoryRGB=0),
    "final": dict(isDebug=0, inputSource=0, fogMode=0, fogColor=(0.0, 0.0, 0.0), fogNear=0.0, fogFar=0.0, fogDensity=0.0),
    "motionBlur": dict(source=abi.TEX_FINAL, center=-1, centerAlphaOne=0, samples=16, intensity=1.0, jitter=1.0, deltaTime=0.0, frame=0, targetHalf=0,
                       halfStoreRTZ=1),
    "export": dict(source=abi.TEX_FINAL, format=abi.EXPORT_U8_SRGB, channels=3, tonemap=0, exposure=1.0),
}


def _put(s, name, ctype, value):
    """s.name = value; an int for a float field is the float's bits"""
    if isinstance(value, tuple):
        getattr(s, name)[:] = value
    elif ctype is C.c_float and isinstance(value, int):
        C.memmove(C.addressof(s) + getattr(type(s), name).offset, struct.pack("<I", value), 4)
    else:
        setattr(s, name, value)


def _fill(cls, required_only=False, start=100):
    """-> (a `cls` struct, the JS object that says the same, the next unused number).  Every leaf gets its own number from `start` on — an
    int field n, a float field n + 0.25 — or, with required_only, only what the addon insists on while the rest holds DEFAULTS."""
    s, js, n = cls(), {}, start
    defaults = DEFAULTS["camera" if cls is abi.Camera else next(k for k, v in STRUCTS.items() if v is cls)]
    for name, ctype in cls._fields_:
        key = CAMERA_JS.get(name, name) if cls is abi.Camera else name
        if issubclass(ctype, C.Structure):
            sub, js[key], n = _fill(ctype, required_only, n)
            setattr(s, name, sub)
        elif required_only and name in defaults:
            _put(s, name, ctype, defaults[name])
        elif issubclass(ctype, C.Array):
            step = 0.25 if ctype._type_ is C.c_float else 0
            js[key] = [n + k + step for k in range(ctype._length_)]
            getattr(s, name)[:] = js[key]
            n += ctype._length_
        else:
            js[key] = n + (0.25 if ctype is C.c_float else 0)
            setattr(s, name, js[key])
            n += 1
    return s, js, n


@pytest.fixture(scope="module")
def cases():
    """{kind: ((full struct, smallest struct), (the addon's bytes for the two objects))} from one node process"""
    want, objects = {}, {}
    for kind, cls in STRUCTS.items():
        full, full_js, _ = _fill(cls)
        least, least_js, _ = _fill(cls, required_only=True)
        want[kind], objects[kind] = (full, least), (full_js, least_js)
    script = ("const addon = require(process.argv[1]), cases = JSON.parse(process.argv[2]), out = {};"
              "for (const k in cases) out[k] = cases[k].map(o => addon.paramBytes(k, o).toString('hex'));"
              "console.log(JSON.stringify(out))")
    got = json.loads(subprocess.check_output([node, "-e", script, ADDON, json.dumps(objects)], text=True))
    return {k: (want[k], tuple(bytes.fromhex(h) for h in got[k]), objects[k]) for k in STRUCTS}


def test_the_defaults_table_names_every_optional_field():
    for kind, cls in list(STRUCTS.items()) + [("camera", abi.Camera)]:
        required = set(CAMERA_REQUIRED) if kind == "camera" else {n for n, t in cls._fields_ if issubclass(t, C.Structure)} | ({"resolution"} if kind == "motionBlur" else set())
        assert set(DEFAULTS[kind]) == {n for n, _ in cls._fields_} - required, kind


@pytest.mark.parametrize("kind", list(STRUCTS))
def test_full_object_equals_the_python_hosts_struct(cases, kind):
    (full, _), (got, _), (obj, _) = cases[kind]
    values = []
    walk = lambda o: [walk(v) for v in o.values()] if isinstance(o, dict) else [walk(v) for v in o] if isinstance(o, list) else values.append(o)
    walk(obj)
    assert len(set(values)) == len(values) == C.sizeof(full) // 4 and min(values) >= 100  # one distinct value per 4-byte leaf, none a default
    assert got == bytes(full)


@pytest.mark.parametrize("kind", list(STRUCTS))
def test_smallest_object_gets_the_defaults(cases, kind):
    (_, least), (_, got), (_, obj) = cases[kind]
    cameras = [n for n, t in STRUCTS[kind]._fields_ if t is abi.Camera]
    assert sorted(obj) == sorted(cameras + (["resolution"] if kind == "motionBlur" else []))  # an empty object where the struct has neither
    assert all(sorted(obj[c]) == sorted(CAMERA_REQUIRED) for c in cameras)
    assert got == bytes(least)
