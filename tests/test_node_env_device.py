"""`run_dump.js --envOnDevice true` through the Node host (N-API setEnvironmentCube / buildEnvironmentImportance): the same 96 x 54 three-frame runs
as tests/test_gpu_env_effect.py — `--envCube` with %d in the name, a new cube before the second frame; a half equirectangular map with flipY —
leave the bytes of the default path, which are the Python host's; Renderer.downloadEnvironmentImportance returns js/envmap.js's tables."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import env_effect_cases as C
from rfx_amd.dump import write_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason="node not installed")]


def run_node(tmp_path, kind, on_device):
    dirs = []
    for i, f in enumerate(C.frames()):
        d = str(tmp_path / ("dump%d" % i))
        if not os.path.isdir(d):
            write_dump(d, f)
        dirs.append(d)
    if kind == "cube":
        for k in range(2):  # frames 0 and 1 have a file: frame 2 keeps frame 1's cube
            C.cube_faces(k).tofile(str(tmp_path / ("cube_%d.bin" % k)))
        env = ["--envCube", json.dumps(str(tmp_path / "cube_%d.bin")), "--envCubeSize", str(C.CUBE_SIZE)]
    else:
        C.equirect().tofile(str(tmp_path / "env.bin"))
        env = ["--env", json.dumps(str(tmp_path / "env.bin")), "--envWidth", str(C.EQUIRECT[0]), "--envHeight", str(C.EQUIRECT[1]), "--envFlipY", "true"]
    out = str(tmp_path / ("out_%s_%d" % (kind, on_device)))
    subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--steps", str(C.OPTIONS["steps"]), "--refineSteps", str(C.OPTIONS["refineSteps"])]
                            + env + (["--envOnDevice", "true"] if on_device else []), text=True, timeout=300)
    return {name: open(os.path.join(out, name + ".bin"), "rb").read() for name, _ in C.OUTPUTS}


@pytest.mark.parametrize("kind", ["cube", "equirect_flipY"])
def test_node_env_on_device_equals_the_default_path_and_the_python_host(tmp_path, kind):
    host, dev = run_node(tmp_path, kind, False), run_node(tmp_path, kind, True)
    py, _ = C.python_run(kind, False)
    for name, _ in C.OUTPUTS:
        assert dev[name] == host[name], name
        assert dev[name] == py[name].tobytes(), name + " (Python host)"


TABLES = r"""
const rfx = require(process.argv[1] + "/index"), { buildImportance } = require(process.argv[1] + "/envmap")
const fs = require("fs")
const b = fs.readFileSync(process.argv[2]), w = +process.argv[3], h = +process.argv[4]
const data = new Float32Array(b.buffer, b.byteOffset, b.length / 4)
const R = new rfx.Renderer(16, 16)
if (!R.hasEnvDevice) throw new Error("no hasEnvDevice")
R.setEnvironment(data, w, h, false, false)
R.buildEnvironmentImportance(false)
const got = R.downloadEnvironmentImportance(), want = buildImportance(data, w, h, false)
const same = (a, c) => Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(c.buffer, c.byteOffset, c.byteLength))
let refused = false
R.setEnvironmentCube(new Float32Array(6 * 4 * 4 * 4).fill(0.5), 4, 32, 16, true)
try { R.downloadEnvironmentImportance() } catch (e) { refused = /-4/.test(String(e.message)) }
console.log(JSON.stringify({ marginal: same(got.marginalWeights, want.marginalWeights), conditional: same(got.conditionalWeights, want.conditionalWeights),
  total: got.totalSumValue === want.totalSumValue, whole: got.whole === Math.fround(Math.trunc(want.totalSumValue)),
  decimal: got.decimal === Math.fround(want.totalSumValue - Math.trunc(want.totalSumValue)), refused }))
"""


def test_node_download_environment_importance(tmp_path):
    """the N-API read-back, on a map with negative texels too: the Node host builder's probe sequence is the kernel's"""
    import env_cases as E
    t = E.texels(128, 64, "negative")
    t.tofile(str(tmp_path / "neg.bin"))
    res = subprocess.check_output([node, "-e", TABLES, JS, str(tmp_path / "neg.bin"), "128", "64"], text=True, timeout=120)
    assert json.loads(res.strip().splitlines()[-1]) == dict(marginal=True, conditional=True, total=True, whole=True, decimal=True, refused=True)
