"""`run_dump.js --stream true` over unpacked dump directories (rfx.h "streamed AOV frames" through the N-API addon: Renderer.stageFrame ->
addon.stageAov): typed directories (half planes, three-channel direct) and all-float ones.  Every output file equals the plain run's over the
same directories, and the typed and the all-float outputs are equal when the float planes are the widened halves."""
import json
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
W, H, FRAMES = 128, 72, 3
HALF = ("diffuse", "normal", "roughness", "metalness", "emissive", "direct")
OUTPUTS = ("final", "compose", "denoise_b0", "denoise_b1", "temporal0", "ssgi")


def _run(dirs, out, stream):
    cmd = [node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", out, "--steps", "10", "--refineSteps", "2"] + (["--stream", "true"] if stream else [])
    res = subprocess.check_output(cmd, text=True, timeout=300)
    info = json.loads(res.strip().splitlines()[-1])
    assert info["frames"] == FRAMES and info["haloViolations"] == 0
    return {n: open(os.path.join(out, n + ".bin"), "rb").read() for n in OUTPUTS}


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node not installed")
def test_run_dump_streams_unpacked_and_typed_dumps(tmp_path):
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import AnalyticScene
    gen = AnalyticScene(1234)
    typed_dirs, float_dirs = [], []
    for i in range(FRAMES):
        f = gen.render(W, H, i, aov=True)
        # the values both kinds of directory carry: halves where the typed one stores halves
        aov = {k: (v.astype(np.float16).astype(np.float32) if k in HALF else v) for k, v in f.aov.items()}
        direct = f.direct.astype(np.float16).astype(np.float32)
        direct[..., 3] = 1.0  # (the typed directory stores rgb: alpha 1)
        fr = types.SimpleNamespace(width=W, height=H, camera=f.camera, prev_camera=getattr(f, "prev_camera", f.camera), depth=f.depth, aov=aov, direct=direct)
        d = str(tmp_path / ("float%d" % i))
        write_dump(d, fr, packed=False)
        float_dirs.append(d)
        fr.direct = direct[..., :3]
        d = str(tmp_path / ("typed%d" % i))
        write_dump(d, fr, packed=False, half=HALF)
        typed_dirs.append(d)
    assert os.path.exists(os.path.join(typed_dirs[0], "aov_normal.f16.bin")) and os.path.getsize(os.path.join(typed_dirs[0], "direct.f16.bin")) == W * H * 6
    runs = {(kind, stream): _run(dirs, str(tmp_path / ("out_%s_%d" % (kind, stream))), stream)
            for kind, dirs in (("typed", typed_dirs), ("float", float_dirs)) for stream in (False, True)}
    assert any(runs[("float", False)]["compose"]) and len(runs[("float", False)]["final"]) == W * H * 16
    for kind in ("typed", "float"):
        for n in OUTPUTS:
            assert runs[(kind, True)][n] == runs[(kind, False)][n], (kind, n)
    for n in OUTPUTS:
        assert runs[("typed", True)][n] == runs[("float", True)][n], n
