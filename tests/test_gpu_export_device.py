"""rfx.h "device images and stream ordering": rfx_export_device (the kernels: k7_export.hip k7_export_strided, and k7_export on the caller's
pointer where the image is tight), rfx_queue_wait_stream and rfx_stream_wait_queue.  The reference everywhere is Context.export — the merged
host path — on the SAME context, and the check is equality of bytes: both paths run the same k7_encode on the same texels, so there is
nothing to tolerate.  An image is written into a backing array pre-filled with PAD and the WHOLE array is compared with the reference laid
out the same way: the values and every padding byte at once.  No case skips on a missing symbol: without rfx_export_device they fail.

Runs on the device (-m gpu) and on the host simulator (--hostsim; tests/test_export_device_cpu.py spawns that run), where "device" memory is
host memory, every stream is immediate and the tests' own HIP calls are memmoves (export_device_cases.Streams)."""
import ctypes as C
import threading
import types

import numpy as np
import pytest

import aov_device_cases as D
import export_device_cases as X

pytestmark = pytest.mark.gpu
_CTX = {}


def tex():
    from rfx_amd import abi
    return abi.TEX_EFFECT_INPUT


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for ctx, _ in _CTX.values():
        ctx.close()
    _CTX.clear()


def state(W, H):
    """one context per size with export_device_cases.input_frame in RFX_TEX_EFFECT_INPUT, and its references: spec -> Context.export's array,
    computed once and read-only"""
    if (W, H) not in _CTX:
        ctx = D.context(W, H)
        assert ctx.has_export_device
        ctx.upload(tex(), X.input_frame(W, H))
        _CTX[(W, H)] = (ctx, {})
    return _CTX[(W, H)]


def reference(W, H, k):
    ctx, refs = state(W, H)
    if k not in refs:
        fmt, ch, tm, ex = X.SPECS[k]
        refs[k] = ctx.export(tex(), fmt, ch, tm, ex)
        refs[k].setflags(write=False)
    return ctx, refs[k]


def written(ctx, arena, want, layout, k, source=None):
    """export specialisation k into a PAD-filled backing array laid out as `layout` -> (the array's bytes, what they must be)"""
    fmt, ch, tm, ex = X.SPECS[k]
    flat, off, sx, sy, sc = X.lay(want, layout)
    addr = arena.blank(flat)
    arena.ready()
    ctx.export_device(tex() if source is None else source, fmt, ch, tm, ex, image=X.image(addr, off, sx, sy, sc, flat.dtype.itemsize))
    ctx.sync()
    return arena.read(addr), flat.tobytes()


# ---------------------------------------------------------------- 1. forms x specialisations x sizes
@pytest.mark.parametrize("case", X.cases(), ids=X.case_id)
def test_forms_specialisations_sizes(case):
    """(1, 1): no group at all; (3, 2): only a tail; (4, 3): exactly one group per row; (5, 4), (66, 5), (97, 55): W mod 4 = 1, 2, 1 with odd
    rows and, at 97 x 55, more than one workgroup along the rows.  The whole backing array: the values and the padding."""
    layout, W, H, k = case
    ctx, want = reference(W, H, k)
    got, flat = written(ctx, X.ReadArena(), want, layout, k)
    assert got == flat, "%s: first differing byte %d of %d" % (X.case_id(case), next(i for i, (a, b) in enumerate(zip(got, flat)) if a != b), len(flat))


# ---------------------------------------------------------------- 2. row tiles
@pytest.mark.parametrize("layout", ["planar_top", "planar_pitch_top"])
def test_row_tiles_write_one_frame(layout):
    """H = 55 in three tiles with halo 4, contexts of one process: each writes its band into one frame-sized buffer, planar and top-down (the
    element form at this width; with padded rows the planar vector form).  The buffer equals the whole-frame context's export."""
    W, H = 97, 55
    frame = X.input_frame(W, H)
    for k in (3, 6, 0):
        fmt, ch, tm, ex = X.SPECS[k]
        _, want = reference(W, H, k)
        flat, off, sx, sy, sc = X.lay(want, layout)
        arena = X.ReadArena()
        addr = arena.blank(flat)
        arena.ready()
        tiles = []
        for y0, n in ((0, 19), (19, 18), (37, 18)):
            ctx = D.context(W, H, (y0, n, 4))
            h0, hn = ctx.held_rows(tex())
            ctx.upload(tex(), frame[h0:h0 + hn])
            ctx.export_device(tex(), fmt, ch, tm, ex, image=X.image(addr, off + y0 * sy, sx, sy, sc, flat.dtype.itemsize))
            tiles.append(ctx)
        for ctx in tiles:
            ctx.sync()
            ctx.close()
        assert arena.read(addr) == flat.tobytes(), (layout, k)


# ---------------------------------------------------------------- 3. mixed sequences
def test_mixed_sequence_keeps_tickets():
    """stage_export -> export_device -> stage_export -> export_wait x 2 on a fresh context: tickets 1 and 2, both host buffers right, the
    device image right"""
    W, H = 97, 55
    _, want_a = reference(W, H, 2)
    _, want_b = reference(W, H, 7)
    _, want_d = reference(W, H, 5)
    ctx = D.context(W, H)
    ctx.upload(tex(), X.input_frame(W, H))
    a, b = ctx.host_alloc(want_a.shape, want_a.dtype), ctx.host_alloc(want_b.shape, want_b.dtype)
    arena = X.ReadArena()
    ta = ctx.stage_export(tex(), *X.SPECS[2], out=a)
    flat, off, sx, sy, sc = X.lay(want_d, "pitch5")
    addr = arena.blank(flat)
    arena.ready()
    ctx.export_device(tex(), *X.SPECS[5], image=X.image(addr, off, sx, sy, sc, flat.dtype.itemsize))
    tb = ctx.stage_export(tex(), *X.SPECS[7], out=b)
    assert (ta, tb) == (1, 2)
    ctx.export_wait(ta)
    ctx.export_wait(tb)
    assert a.tobytes() == want_a.tobytes() and b.tobytes() == want_b.tobytes()
    ctx.sync()
    assert arena.read(addr) == flat.tobytes()
    ctx.close()


def test_drawn_source_both_ways():
    """three frames of SSGIEffect at 96 x 54 (test_chain_from_device_planes' set-up): RFX_TEX_COMPOSE exported both ways each frame"""
    from rfx_amd import abi
    from rfx_amd.effect import SSGIEffect
    from rfx_amd.scene import AnalyticScene
    W, H, N = 96, 54, 3
    gen = AnalyticScene(1234)
    ctx = D.context(W, H)
    arena = X.ReadArena()
    scene = types.SimpleNamespace(frame=None)
    cam = None
    fx = None
    for i in range(N):
        f = gen.render(W, H, i, aov=True)
        frame = types.SimpleNamespace(camera=f.camera, static="resident", depth=f.depth, direct=f.direct, gbuffer=None, velocity=None, aov=f.aov)
        if fx is None:
            cam = types.SimpleNamespace(**vars(f.camera))
            fx = SSGIEffect(None, scene, cam, dict(width=W, height=H, steps=10, refineSteps=2), seeds=dict(ssgi=3, denoise=4), half_store_rtz=True)
        ctx.stage_frame(frame)
        ctx.stage_flip()
        scene.frame = frame
        for k, v in vars(f.camera).items():
            setattr(cam, k, v)
        fx.update(ctx, None)
        for k, layout in ((3, "planar_pitch_top"), (4, "pitch4"), (1, "tight")):
            want = ctx.export(abi.TEX_COMPOSE, *X.SPECS[k])
            got, flat = written(ctx, arena, want, layout, k, source=abi.TEX_COMPOSE)
            assert got == flat, (i, k, layout)
    assert want.any() and ctx.halo_violations() == 0
    ctx.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals_leave_everything_as_it_was():
    """each refusal returns its code and names the entry point; a good call right after gives the right bytes"""
    from rfx_amd import abi
    from rfx_amd.context import Context
    W, H = 5, 4
    ctx = D.context(W, H)
    ctx.upload(tex(), X.input_frame(W, H))
    arena = X.ReadArena()
    lib, h = ctx.lib, ctx._h
    E, S = abi.RFX_EINVAL, abi.RFX_ESTATE

    def good(k, layout="planar_pitch"):
        fmt, ch, tm, ex = X.SPECS[k]
        want = ctx.export(tex(), fmt, ch, tm, ex)
        got, flat = written(ctx, arena, want, layout, k)
        assert got == flat, (k, layout)

    def refused(code, k=1, source=None, params=None, image=None, null_dst=False, **strides):
        """the call with one thing wrong: over a PAD-filled tight backing array that must stay PAD"""
        fmt, ch, tm, ex = X.SPECS[k]
        p = Context.export_params(tex() if source is None else source, fmt, ch, tm, ex)
        for name, v in (params or {}).items():
            setattr(p, name, v)
        elem = X.ELEM[fmt]
        blank = np.full(W * H * ch + 8, X.PAD, abi.EXPORT_DTYPE[X.FORMAT_ID[fmt]])
        addr = arena.put(blank)
        arena.ready()
        img = abi.DeviceImage(addr, ch, W * ch, 1) if image is None else image(addr, elem, ch)
        for name, v in strides.items():
            setattr(img, name, v)
        rc = lib.rfx_export_device(h, C.byref(p), None if null_dst else C.byref(img))
        msg = lib.rfx_last_error(h)
        assert rc == code and b"rfx_export_device" in msg, (rc, msg)
        ctx.sync()
        assert arena.read(addr) == blank.tobytes()
        good(k)

    good(1)
    # what rfx_export refuses
    refused(E, params=dict(source=abi.TEX_DEPTH))
    refused(E, params=dict(format=3))
    refused(E, params=dict(channels=2))
    refused(E, params=dict(channels=5))
    refused(E, params=dict(tonemap=1))                # (an operator with F32)
    refused(E, k=4, params=dict(tonemap=2))
    refused(E, k=4, params=dict(exposure=-1.0))
    refused(E, k=4, params=dict(exposure=float("nan")))
    refused(E, k=2, params=dict(exposure=0.5))        # (an exposure with F16)
    # dst or data NULL
    refused(E, null_dst=True)
    refused(E, image=lambda a, e, ch: abi.DeviceImage(None, ch, W * ch, 1))
    # the address against the element size: F32 at 2 and at 1 byte, F16 at 1 byte (U8 has none)
    refused(E, k=0, image=lambda a, e, ch: abi.DeviceImage(a + 2, ch, W * ch, 1))
    refused(E, k=1, image=lambda a, e, ch: abi.DeviceImage(a + 1, ch, W * ch, 1))
    refused(E, k=3, image=lambda a, e, ch: abi.DeviceImage(a + 1, ch, W * ch, 1))
    good(2, "offset1")                                # (a half one element in is fine)
    # strides that do not nest: a 0 stride on every axis, rows that overlap by one element, channels inside the pixel step, planes inside a row
    refused(E, stride_x=0)
    refused(E, stride_y=0)
    refused(E, stride_c=0)
    refused(E, k=0, stride_y=W * 3 - 1)
    refused(E, k=5, stride_y=-(W * 4 - 1))
    refused(E, k=3, stride_x=3)                       # (4 channels in a pixel step of 3)
    refused(E, k=7, image=lambda a, e, ch: abi.DeviceImage(a, 1, W, W - 1))          # planar, plane pitch inside a row ...
    refused(E, k=7, image=lambda a, e, ch: abi.DeviceImage(a, 1, W, H * W - 1))      # ... and one element short of a plane
    # extents beyond 62 bits of bytes, with products that overflow 64 bits
    refused(E, stride_y=2 ** 62)
    refused(E, stride_x=-2 ** 63)
    refused(E, stride_c=2 ** 61)
    refused(E, k=6, stride_x=2 ** 60, stride_y=-2 ** 62, stride_c=2 ** 57)
    refused(E, k=2, stride_x=2 ** 58, stride_y=-2 ** 61)
    # RFX_ESTATE: a source never filled (a slot a draw writes does not exist yet; a host-filled one was never uploaded)
    refused(S, params=dict(source=abi.TEX_FINAL))
    refused(S, params=dict(source=abi.TEX_DIRECT_LIGHT))
    # the ordering calls: NULL streams, unknown queues
    for fn in (lib.rfx_queue_wait_stream, lib.rfx_stream_wait_queue):
        name = b"rfx_queue_wait_stream" if fn is lib.rfx_queue_wait_stream else b"rfx_stream_wait_queue"
        for queue, stream in ((abi.QUEUE_DRAW, None), (abi.QUEUE_UPLOAD, None), (2, C.c_void_p(4096)), (-1, C.c_void_p(4096))):
            assert fn(h, queue, stream) == E and name in lib.rfx_last_error(h), (name, queue)
        good(6, "scanline")
    for bad in (0, None, 1.5, True):
        with pytest.raises((ValueError, TypeError)):
            ctx.queue_wait_stream(abi.QUEUE_DRAW, bad)
    ctx.close()


# ---------------------------------------------------------------- 5. a producer loop without a host wait
def test_producer_loop_without_a_host_wait():
    """two frames at 97 x 55 staged from ONE set of device planes that a producer stream refills: the upload queue waits for the producer's
    copies, the producer's next copies wait for the pack kernel, the host waits for neither"""
    import aov_cases as AC
    from rfx_amd import abi
    W, H = 97, 55
    frames = [AC.stage(D.frame(W, H, 0xb00 + i), D.TYPES["typed"], 4, 4, AC.NAMES) for i in range(2)]
    wants = [D.host_reference(W, H, f) for f in frames]
    ctx = D.context(W, H)
    arena, st = X.ReadArena(), X.Streams()
    p = st.stream()
    # per plane: one device backing array (planar, padded rows: the vector form) and per frame a pinned host array of the same bytes
    planes, pinned = {}, []
    for name, v in frames[0].items():
        flat, off, sx, sy, sc = D.lay(v, "planar_pitch")
        addr = arena.put(np.zeros_like(flat))
        ch = 1 if v.ndim == 2 else v.shape[2]
        planes[name] = (abi.DevicePlane(addr + off * v.dtype.itemsize, abi.PLANE_TYPES[v.dtype], ch, sx, sy, sc), addr, flat.nbytes)
    arena.ready()
    for f in frames:
        host = {}
        for name, v in f.items():
            flat = D.lay(v, "planar_pitch")[0]
            pin = ctx.host_alloc(flat.shape, flat.dtype)
            pin[...] = flat
            host[name] = pin
        pinned.append(host)
    for k in range(2):
        for name, (_, addr, n) in planes.items():
            st.copy_async(addr, pinned[k][name].ctypes.data, n, 1, p)
        ctx.queue_wait_stream(abi.QUEUE_UPLOAD, p)
        ctx.stage_aov_device({name: rec[0] for name, rec in planes.items()})
        ctx.stream_wait_queue(abi.QUEUE_UPLOAD, p)
        ctx.stage_flip()
        bad = D.same_bytes(D.slots_of(ctx), wants[k])
        assert not bad, "frame %d: %s" % (k, "\n".join(bad))
    # the keyword: the same ordering through stage_aov_device(producer=)
    for name, (_, addr, n) in planes.items():
        st.copy_async(addr, pinned[0][name].ctypes.data, n, 1, p)
    ctx.stage_aov_device({name: rec[0] for name, rec in planes.items()}, producer=p)
    ctx.stage_flip()
    bad = D.same_bytes(D.slots_of(ctx), wants[0])
    assert not bad, "\n".join(bad)
    st.sync(p)
    ctx.close()
    st.close()


# ---------------------------------------------------------------- 6. a consumer loop
def test_consumer_loop_reuses_one_image():
    """three frames, one device image rewritten every frame, a consumer stream that copies it away: export_device(stream=) orders the encode
    behind the consumer's last read and the consumer's copy behind the encode; one synchronise at the end"""
    W, H, N, k = 97, 55, 3, 3
    fmt, ch, tm, ex = X.SPECS[k]
    ctx = D.context(W, H)
    arena, st = X.ReadArena(), X.Streams()
    c = st.stream()
    wants = []
    for i in range(N):
        ctx.upload(tex(), X.input_frame(W, H, seed=i))
        wants.append(ctx.export(tex(), fmt, ch, tm, ex))
    flat0, off, sx, sy, sc = X.lay(wants[0], "planar_pitch_top")
    img_addr = arena.blank(flat0)
    kept = [arena.blank(flat0) for _ in range(N)]
    arena.ready()
    img = X.image(img_addr, off, sx, sy, sc, flat0.dtype.itemsize)
    for i in range(N):
        ctx.upload(tex(), X.input_frame(W, H, seed=i))
        ctx.export_device(tex(), fmt, ch, tm, ex, image=img, stream=c)
        st.copy_async(kept[i], img_addr, flat0.nbytes, 3, c)
    st.sync(c)
    for i in range(N):
        assert arena.read(kept[i]) == X.lay(wants[i], "planar_pitch_top")[0].tobytes(), i
    assert len({w.tobytes() for w in wants}) == N
    ctx.close()
    st.close()


# ---------------------------------------------------------------- 7. the dependency exists
@pytest.mark.skipif(X.HOSTSIM, reason="--hostsim: every stream is immediate, there is no order to observe")
def test_the_dependency_exists():
    """A gate — a host function that waits on a threading.Event, for 5 s at the most — holds the caller's stream.  What the ordering calls make
    wait for it is not ready while an unrelated stream still runs; once the gate opens it completes with the right bytes.  For
    RFX_QUEUE_UPLOAD (a producer) and for RFX_QUEUE_DRAW (export_device(stream=))."""
    import aov_cases as AC
    from rfx_amd import abi
    hip = D.hip()
    HOSTFN = C.CFUNCTYPE(None, C.c_void_p)
    hip.hipLaunchHostFunc.argtypes = [C.c_void_p, HOSTFN, C.c_void_p]
    NOT_READY = 600  # hipErrorNotReady
    W, H = 97, 55
    st, arena = X.Streams(), X.ReadArena()
    gate = threading.Event()
    held = HOSTFN(lambda _: gate.wait(5.0) and None)
    scratch = arena.put(np.zeros(64, np.uint8))
    arena.ready()

    def control_runs():
        """an unrelated stream with one small memset finishes: the runtime itself is not stalled.  (Streams share hardware queues, and a held
        stream holds its queue: of as many fresh streams as a process has queues by default, one that does not share the gate's must finish.)"""
        fresh = [st.stream() for _ in range(4)]
        for s in fresh:
            assert hip.hipMemsetAsync(scratch, 1, 64, s) == 0
        for _ in range(200000):
            if any(hip.hipStreamQuery(s) == 0 for s in fresh):
                return
        raise AssertionError("no control stream finished while the gate was held")

    # UPLOAD: the pack kernel waits for the gated producer; a second stream made to wait for the upload queue is not ready
    staged = AC.stage(D.frame(W, H, 0xc00), D.TYPES["typed"], 4, 4, AC.NAMES)
    want = D.host_reference(W, H, staged)
    ctx = D.context(W, H)
    planes = D.device_planes(arena, staged, "planar_pitch")
    p, t = st.stream(), st.stream()
    try:
        assert hip.hipLaunchHostFunc(p, held, None) == 0
        ctx.stage_aov_device(planes, producer=p)
        ctx.stream_wait_queue(abi.QUEUE_UPLOAD, t)
        assert hip.hipStreamQuery(t) == NOT_READY
        control_runs()
        assert hip.hipStreamQuery(t) == NOT_READY
    finally:
        gate.set()
    st.sync(t)
    ctx.stage_flip()
    bad = D.same_bytes(D.slots_of(ctx), want)
    assert not bad, "\n".join(bad)
    ctx.close()

    # DRAW: the encode waits for the gated consumer stream, and that stream for the encode
    gate.clear()
    k = 5
    ctx, ref = reference(W, H, k)
    flat, off, sx, sy, sc = X.lay(ref, "pitch4_top")
    addr = arena.blank(flat)
    arena.ready()
    c, t = st.stream(), st.stream()
    try:
        assert hip.hipLaunchHostFunc(c, held, None) == 0
        ctx.export_device(tex(), *X.SPECS[k], image=X.image(addr, off, sx, sy, sc, flat.dtype.itemsize), stream=c)
        ctx.stream_wait_queue(abi.QUEUE_DRAW, t)
        assert hip.hipStreamQuery(t) == NOT_READY and hip.hipStreamQuery(c) == NOT_READY
        control_runs()
        assert hip.hipStreamQuery(t) == NOT_READY
    finally:
        gate.set()
    st.sync(t)
    st.sync(c)
    assert arena.read(addr) == flat.tobytes()
    st.close()
