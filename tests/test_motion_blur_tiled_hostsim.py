"""GPU-marked, host simulator only (pytest -m gpu --hostsim): MotionBlurEffect on row tiles with the exchange BEHIND THE C ABI
(rfx_motion_blur_gather over tests/hostsim/fakerccl.c), one process per tile, against the single context; and the Node twin, run_dump.js."""
import json
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
JS = os.path.join(os.path.dirname(HERE), "realism-effects_amd", "js")
node = shutil.which("node")
W, H, FRAMES = 97, 55, 3
# the synthetic orbit is slow (|v.y| <= 0.0047 of the frame, a quarter of a row): with this intensity half a streak is 0.5 * 0.255 * 250 * 0.6 = 19
# rows, more than the 12-row tiles of four ranks
INTENSITY = 250.0


def _single_context():
    from rfx_amd import abi
    from rfx_amd.context import Context
    from rfx_amd.effect import MotionBlurEffect, SSGIEffect
    from rfx_amd.scene import synthetic_frame

    frames = [synthetic_frame(W, H, i) for i in range(FRAMES)]
    ctx = Context(W, H)
    scene, cam = types.SimpleNamespace(frame=None), frames[0].camera
    fx = SSGIEffect(None, scene, cam, dict(width=W, height=H, denoiseIterations=1), seeds=dict(ssgi=5, denoise=9))
    mb = MotionBlurEffect(None, {"samples": 8, "intensity": INTENSITY})
    out, finals = [], []
    for f in frames:
        scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        fx.update(ctx, None)
        mb.update(ctx, fx.mainImage(ctx), 1 / 60)
        assert mb.mainImage(ctx) == abi.TEX_MOTION_BLUR
        out.append(mb.output(ctx).copy())
        finals.append(ctx.download(abi.TEX_FINAL).copy())
    ctx.close()
    return np.stack(out), np.stack(finals)


_REF = []


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("RFX_HOSTSIM") != "1", reason="the C ABI's exchanges between processes without RCCL: pytest --hostsim")
@pytest.mark.parametrize("world", [2, 3, 4])
def test_comm_tiled_motion_blur_is_bit_identical_to_one_context(tmp_path, world):
    """Three frames of SSGIEffect then MotionBlurEffect (source: the effect's final image) through CommTiledRenderer, one process per tile
    (tests/motion_blur_tile_worker.py): every rank's rows of the blurred frame equal the single context's, it never receives more than the
    other tiles' rows, and no fetch left a held band."""
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "motion_blur_tile_worker.py"), str(r), str(world), str(tmp_path), str(W), str(H), str(FRAMES),
                               str(INTENSITY)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    try:
        outs = [p.communicate(timeout=300)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    if not _REF:
        _REF.append(_single_context())
    ref, finals = _REF[0]
    assert not np.array_equal(ref, finals)  # (the frame is blurred)
    travelled = 0
    for rank in range(world):
        z = np.load(os.path.join(str(tmp_path), "mb%d.npz" % rank))
        y0, rows = int(z["y0"]), int(z["rows"])
        assert z["blurred"].tobytes() == ref[:, y0:y0 + rows].tobytes(), "rank %d of %d: blurred rows differ" % (rank, world)
        assert len(z["blur_bytes"]) == FRAMES and (z["blur_bytes"] <= (H - rows) * W * 16).all(), z["blur_bytes"]
        assert int(z["halo_violations"]) == 0
        travelled += int(z["blur_bytes"].sum())
        print("rank %d of %d receives %s bytes of blur source per frame (the other tiles' rows: %d)" % (rank, world, list(z["blur_bytes"]), (H - rows) * W * 16))
    assert travelled > 0  # (streaks do cross tiles here: the exchange is exercised)


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("RFX_HOSTSIM") != "1", reason="one Node process per tile without RCCL / without N GPUs: pytest --hostsim")
@pytest.mark.skipif(node is None, reason="node not installed")
@pytest.mark.parametrize("ranks", [2, 3])
def test_node_row_tiled_motion_blur_equals_single_process(tmp_path, ranks):
    """`run_dump.js --ranks N --motionBlur`: every rank gathers the source texels its streaks reach (rfx_motion_blur_gather through the N-API
    addon), writes its rows of the blurred frame, the parent stitches them: the same bytes as `--ranks 1`."""
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    dirs = []
    for i in range(FRAMES):
        d = str(tmp_path / ("dump%d" % i))
        write_dump(d, synthetic_frame(W, H, i))
        dirs.append(d)
    env = dict(os.environ, RFX_ONE_GPU="1")
    common = ["--steps", "12", "--refineSteps", "3", "--motionBlur", json.dumps(dict(samples=8, intensity=INTENSITY))]
    one, many = str(tmp_path / "one"), str(tmp_path / "many")
    subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", one] + common, text=True, env=env, timeout=300)
    res = subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", many, "--ranks", str(ranks)] + common, text=True, env=env, timeout=300)
    info = json.loads(res.strip().splitlines()[-1])
    assert info["ranks"] == ranks and info["haloViolations"] == 0 and info["frames"] == FRAMES
    for name in ("motion_blur", "final", "compose"):
        a, b = open(os.path.join(one, name + ".bin"), "rb").read(), open(os.path.join(many, name + ".bin"), "rb").read()
        assert a == b and len(a) == W * H * 16, name
    assert open(os.path.join(one, "motion_blur.bin"), "rb").read() != open(os.path.join(one, "final.bin"), "rb").read()
    assert not [f for f in os.listdir(many) if ".rank" in f]
