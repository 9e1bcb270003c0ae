"""resolutionScale < 1 on row tiles, one process per tile, on the host simulator's library (tests/hostsim: the kernel sources on the CPU, its
stand-in RCCL over unix sockets).  The Python flow (tests/scaled_tile_worker.py: CommTiledRenderer behind the C ABI, history_gather "all" and
"bounded") is a CPU test: the workers load the simulator whatever pytest was started with.  The Node flow (run_dump.js --ranks N
--resolutionScale S) is marked gpu and runs under `pytest -m gpu --hostsim`, like the other Node tiled runs."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from launch_plans import needs_hostsim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JS = os.path.join(ROOT, "realism-effects_amd", "js")
node = shutil.which("node")
W, H, FRAMES, SCALE = 200, 132, 3, 0.5
CHAIN = ("temporal0", "temporal1", "denoise_b0", "denoise_b1", "compose")
_ONE = {}


def _sim_env():
    """what `pytest --hostsim` gives the processes its tests spawn (tests/conftest.py), for these workers alone"""
    sim = os.path.join(ROOT, "tests", "hostsim")
    subprocess.check_call(["make", "-s", "-C", sim])
    from conftest import hostsim_child_env
    env = dict(os.environ, **hostsim_child_env(sim))
    env["LD_LIBRARY_PATH"] = os.path.join(sim, "_build", "fakerccl") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    return env


def _run(world, mode, outdir):
    os.makedirs(outdir, exist_ok=True)
    env = _sim_env()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "scaled_tile_worker.py"), str(r), str(world), outdir, str(W), str(H), str(FRAMES), mode, str(SCALE)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(world)]
    try:
        outs = [p.communicate(timeout=300)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    return [np.load(os.path.join(outdir, "s%d.npz" % r)) for r in range(world)]


@needs_hostsim
@pytest.mark.parametrize("world,mode", [(2, "all"), (3, "all"), (2, "bounded"), (3, "bounded")])
def test_scaled_comm_tiled_run_equals_a_one_rank_run(tmp_path, world, mode):
    """Three frames of SSGIEffect at resolutionScale 0.5 through CommTiledRenderer on 2 and 3 ranks, 200 x 132 (ragged tiles at 3), with the
    whole-frame all-gather of the composed GI and with the bounded gather (rfx_gather_history_rows after a scaled trace): every rank's rows of
    every chain slot and its rows of the K1 target equal the one-rank run's, and no fetch left a held band.  (history_gather "peer" maps the
    peers' planes through HIP IPC, which the simulator has between contexts of one process only: tests/test_gpu_resolution_scale_tiled.py.)"""
    if not _ONE:
        _ONE["z"] = _run(1, "all", str(tmp_path / "one"))[0]
    one = _ONE["z"]
    assert int(one["j0"]) == 0 and one["target"].shape == (int(H * SCALE), int(W * SCALE), 4) and (one["target"] != 0).any()
    covered = np.zeros(int(H * SCALE), bool)
    for rank, z in enumerate(_run(world, mode, str(tmp_path / "many"))):
        y0, rows, j0 = int(z["y0"]), int(z["rows"]), int(z["j0"])
        for name in CHAIN:
            assert z[name].tobytes() == one[name][y0:y0 + rows].tobytes(), "rank %d of %d: %s differs" % (rank, world, name)
        assert z["target"].tobytes() == one["target"][j0:j0 + len(z["target"])].tobytes(), "rank %d of %d: target rows from %d differ" % (rank, world, j0)
        covered[j0:j0 + len(z["target"])] = True
        assert int(z["halo_violations"]) == 0
        if mode == "bounded":  # never more than the all-gather would deliver (the other tiles' rows of the RGB twin), once per frame
            assert len(z["history_bytes"]) == FRAMES and (z["history_bytes"] <= (H - rows) * W * 12).all(), z["history_bytes"]
    assert covered.all()


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("RFX_HOSTSIM") != "1", reason="one Node process per tile without RCCL / without N GPUs: pytest --hostsim")
@pytest.mark.skipif(node is None, reason="node not installed")
@pytest.mark.parametrize("ranks,gather", [(2, "all"), (3, "bounded")])
def test_node_row_tiled_scaled_run_equals_single_process(tmp_path, ranks, gather):
    """`run_dump.js --ranks N --resolutionScale 0.5`: the parent stitches the tiles; every output — ssgi.bin is the stitched (W*s) x (H*s)
    target, each rank contributing the rows whose nearest full-resolution row it owns — holds the same bytes as `--ranks 1`."""
    from rfx_amd.dump import write_dump
    from rfx_amd.scene import synthetic_frame
    dirs = []
    for i in range(FRAMES):
        d = str(tmp_path / ("dump%d" % i))
        write_dump(d, synthetic_frame(W, H, i))
        dirs.append(d)
    env = dict(os.environ, RFX_ONE_GPU="1")
    common = ["--steps", "12", "--refineSteps", "3", "--resolutionScale", str(SCALE)]
    one, many = str(tmp_path / "one"), str(tmp_path / "many")
    subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", one] + common, text=True, env=env, timeout=300)
    res = subprocess.check_output([node, os.path.join(JS, "run_dump.js")] + dirs + ["--out", many, "--ranks", str(ranks), "--historyGather", json.dumps(gather)] + common,
                                  text=True, env=env, timeout=300)
    info = json.loads(res.strip().splitlines()[-1])
    assert info["ranks"] == ranks and info["haloViolations"] == 0 and info["frames"] == FRAMES
    for name in ("ssgi", "final", "compose", "denoise_b0", "denoise_b1", "temporal0"):
        a, b = open(os.path.join(one, name + ".bin"), "rb").read(), open(os.path.join(many, name + ".bin"), "rb").read()
        assert a == b, name
        assert len(a) == (int(W * SCALE) * int(H * SCALE) * 16 if name == "ssgi" else W * H * (8 if name.startswith("denoise") else 16)), name
    assert any(open(os.path.join(one, "ssgi.bin"), "rb").read())
    assert not [f for f in os.listdir(many) if ".rank" in f]
