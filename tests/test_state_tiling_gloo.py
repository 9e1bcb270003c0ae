"""Checkpoints and row tiling, CPU, over gloo (the per-tile compute is the oracle double of tests/test_tiling_gloo.py; the exchange, the
save and the load are the product's): a checkpoint saved at world 1 resumes at world 2 and 3, one saved at world 3 — every rank writing
its own rows of the whole-frame planes, rank 0 the header — resumes at world 1.  The plane files of the two saves are byte-identical and
the frames after the resume equal the uninterrupted run's, draw parameters and texels."""
import json
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, FRAMES, CUT = 96, 64, 4, 2
SEEDS = dict(ssgi=5, denoise=9)


def _effect(scene, cam, seeds):
    from rfx_amd.effect import SSGIEffect
    return SSGIEffect(None, scene, cam, dict(width=W, height=H, denoiseIterations=1), seeds=seeds)


def _advance(fx, renderer, scene, cam, frames):
    for f in frames:
        scene.frame = f
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        fx.update(renderer, None)


def _stream(calls):
    """The draws' parameters, without what only a tiled run adds (row windows, the trace half of K1) and with the strips of one windowed
    draw counted once."""
    out = []
    for c in calls:
        if c[0] in ("ssgi", "temporal", "denoise", "compose") and (not out or out[-1] != c):
            out.append(c)
    return out


def _setup(rank, world, port):
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401  (sys.path setup)
    from rfx_amd import tiling
    from rfx_amd.scene import synthetic_frame
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    frames = [synthetic_frame(W, H, i) for i in range(FRAMES)]
    vmax = max(float(np.abs(f.velocity[..., 1].view(np.float32)).max()) for f in frames)
    halo = tiling.required_halo(3.0, vmax, H, W)
    y0, rows = tiling.split_rows(H, world)[rank]
    return frames, halo, y0, rows


def _load_worker(rank, world, port, ckdir, outdir):
    """world ranks over torch.distributed (TiledRenderer): fresh effects, load, the remaining frames"""
    frames, halo, y0, rows = _setup(rank, world, port)
    from oracle_renderer import OracleRenderer
    from rfx_amd import abi, state, tiling
    inner = OracleRenderer(W, H, y0, rows, halo)
    tensors = {}
    for tex in tiling.EXCHANGED + (abi.TEX_COMPOSE_RGB,):
        b0, n = inner.held_rows(tex)
        tensors[tex] = torch.from_numpy(inner.tex[tex][b0:b0 + n])
    r = tiling.TiledRenderer(inner, tensors, rank, world)
    scene, cam = types.SimpleNamespace(frame=None), types.SimpleNamespace(**vars(frames[CUT].camera))
    fx = _effect(scene, cam, None)
    exchanges = r.exchange_count
    state.load_state(ckdir, r, [fx])
    assert r.exchange_count == exchanges  # every tile took the rows it holds, halo included: nothing travelled
    _advance(fx, r, scene, cam, frames[CUT:])
    r.sync()
    np.savez(os.path.join(outdir, "load%d_%d.npz" % (world, rank)), y0=y0, rows=rows, calls=json.dumps(_stream(inner.calls)),
             **{abi.TEX_NAMES[t]: inner.tex[t][y0:y0 + rows] for t in (abi.TEX_SSGI, abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1, abi.TEX_DENOISE_A0, abi.TEX_DENOISE_B0,
                                                                     abi.TEX_DENOISE_B1, abi.TEX_COMPOSE)})
    dist.barrier()
    dist.destroy_process_group()


def _save_worker(rank, world, port, ckdir, outdir):
    """world ranks through CommTiledRenderer on a context whose exchanges run over gloo at comm_wait (tests/test_tiling_gloo.py): the first
    frames, then every rank saves — with an overlapped all-gather of the composed GI still in flight when save_state is called"""
    frames, halo, y0, rows = _setup(rank, world, port)
    from oracle_renderer import OracleRenderer
    from rfx_amd import state, tiling

    class LazyCommCtx(OracleRenderer):
        def __init__(self, *a):
            super().__init__(*a)
            self.queue = []

        def comm_init(self, uid, r, n):
            pass

        def halo_exchange(self, tex, up, down):
            self.queue.append(("halo", tex, up, down))

        def allgather_history(self, tex):
            self.queue.append(("gather", tex))

        def comm_wait(self):
            q, self.queue = self.queue, []
            for op in q:
                if op[0] == "halo":
                    _, tex, up, down = op
                    t = torch.from_numpy(self.tex[tex])
                    ops = []
                    for peer, send, recv in tiling.halo_plan(self.H, world, rank, self.halo):
                        if (peer > rank and up < 0) or (peer < rank and down < 0):
                            continue
                        if send:
                            ops.append(dist.P2POp(dist.isend, t[send[0]:send[1]].contiguous(), peer))
                        if recv:
                            ops.append(dist.P2POp(dist.irecv, t[recv[0]:recv[1]], peer))
                    for w in dist.batch_isend_irecv(ops):
                        w.wait()
                else:
                    t = torch.from_numpy(self.tex[op[1]])
                    for r_, (ty0, tn) in enumerate(tiling.split_rows(self.H, world)):
                        dist.broadcast(t[ty0:ty0 + tn], src=r_)

    inner = LazyCommCtx(W, H, y0, rows, halo)
    r = tiling.CommTiledRenderer(inner, rank, world, b"\0" * 128)
    scene, cam = types.SimpleNamespace(frame=None), types.SimpleNamespace(**vars(frames[0].camera))
    fx = _effect(scene, cam, SEEDS)
    _advance(fx, r, scene, cam, frames[:CUT])
    assert r._pending  # the composed GI of the last frame is still being gathered: the save lets it land first
    header = state.save_state(ckdir, r, [fx])
    assert not inner.queue and not r._pending
    with open(os.path.join(outdir, "header%d.json" % rank), "w") as f:
        json.dump(header, f)
    dist.barrier()
    dist.destroy_process_group()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.timeout(600)
def test_checkpoints_move_between_world_sizes(tmp_path):
    from oracle_renderer import OracleRenderer
    from rfx_amd import abi, state
    from rfx_amd.scene import synthetic_frame
    frames = [synthetic_frame(W, H, i) for i in range(FRAMES)]
    ck1, ck3, out = str(tmp_path / "world1"), str(tmp_path / "world3"), str(tmp_path)
    # world 1: the first frames, save, the rest = the uninterrupted run
    ref = OracleRenderer(W, H)
    scene, cam = types.SimpleNamespace(frame=None), types.SimpleNamespace(**vars(frames[0].camera))
    fx = _effect(scene, cam, SEEDS)
    _advance(fx, ref, scene, cam, frames[:CUT])
    header1 = state.save_state(ck1, ref, [fx])
    n0 = len(ref.calls)
    _advance(fx, ref, scene, cam, frames[CUT:])
    want_calls = json.loads(json.dumps(_stream(ref.calls[n0:])))
    stages = (abi.TEX_SSGI, abi.TEX_TEMPORAL0, abi.TEX_TEMPORAL1, abi.TEX_DENOISE_A0, abi.TEX_DENOISE_B0, abi.TEX_DENOISE_B1, abi.TEX_COMPOSE)
    # saved at world 1, loaded at world 2 and 3
    for world in (2, 3):
        mp.spawn(_load_worker, args=(world, _port(), ck1, out), nprocs=world, join=True)
        for rank in range(world):
            z = np.load(os.path.join(out, "load%d_%d.npz" % (world, rank)))
            y0, rows = int(z["y0"]), int(z["rows"])
            assert json.loads(str(z["calls"])) == want_calls, "world %d rank %d" % (world, rank)
            for t in stages:
                assert np.array_equal(z[abi.TEX_NAMES[t]], ref.tex[t][y0:y0 + rows]), "world %d rank %d %s" % (world, rank, abi.TEX_NAMES[t])
    # saved at world 3 (each rank its own rows, rank 0 the header): the same files ...
    mp.spawn(_save_worker, args=(3, _port(), ck3, out), nprocs=3, join=True)
    header3 = json.load(open(os.path.join(ck3, "state.json")))
    assert header3 == json.loads(json.dumps(header1))
    for rank in range(3):
        assert json.load(open(os.path.join(out, "header%d.json" % rank))) == header3  # what save_state returned on every rank
    for p in header1["planes"]:
        assert open(os.path.join(ck1, p["file"]), "rb").read() == open(os.path.join(ck3, p["file"]), "rb").read(), p["slot"]
    assert sorted(os.listdir(ck3)) == sorted(["state.json"] + [p["file"] for p in header3["planes"]])
    # ... loaded at world 1
    one = OracleRenderer(W, H)
    scene, cam = types.SimpleNamespace(frame=None), types.SimpleNamespace(**vars(frames[CUT].camera))
    fx = _effect(scene, cam, None)
    state.load_state(ck3, one, [fx])
    _advance(fx, one, scene, cam, frames[CUT:])
    assert json.loads(json.dumps(_stream(one.calls))) == want_calls
    for t in stages:
        assert np.array_equal(one.tex[t], ref.tex[t]), abi.TEX_NAMES[t]
