"""rfx.h "streamed EXR frames" (rfx_stage_exr_aov / rfx_exr_aov_stage_bytes / rfx_exr_aov_status; the kernels: k9_exr_import.hip).  The reference
everywhere is the host decode of the same pixels — imageio.exr_to_typed_planes + stage_aov on a second context — and the check is equality of
bytes of DEPTH, GBUFFER, VELOCITY and DIRECT_LIGHT: the device decode feeds the same pack kernel the same planes, so there is nothing to tolerate.
The deflate form inside a file is chosen by exr_import_cases.repack.  Runs on the device (-m gpu) and on the host simulator (--hostsim)."""
import ctypes as C

import numpy as np
import pytest

import exr_import_cases as X
import inflate_cases as IC

pytestmark = pytest.mark.gpu

HALF_LAYERS_MIXED = ("diffuse", "normal", "roughness", "metalness", "emissive", "direct")  # velocity and depth stay float: the 44 B/px frame


def _slots():
    from rfx_amd import abi
    return (abi.TEX_DEPTH, abi.TEX_GBUFFER, abi.TEX_VELOCITY, abi.TEX_DIRECT_LIGHT)


def host_planes(path):
    """stage_aov's planes from the host decode: exr_to_typed_planes, or — a file that lacks a whole plane, which that call refuses — its rules
    applied to the planes the file has"""
    from rfx_amd import imageio
    try:
        t = imageio.exr_to_typed_planes(path)
        return dict(t["aov"], depth=t["depth"], direct=t["direct"])
    except KeyError:
        ch, types_ = imageio.read_exr(path), imageio.exr_channel_types(path)
        out = {}
        for key, cn in imageio.AOV_LAYOUT.items():
            have = [c for c in cn if c in ch]
            if not have:
                continue
            assert have == list(cn) or (key in ("diffuse", "direct") and have == list(cn[:3]))
            a = np.stack([ch[c] for c in have], -1) if len(cn) > 1 else ch[have[0]]
            out[key] = np.ascontiguousarray(a.astype(np.float16 if all(types_[c] == "half" for c in have) else np.float32))
        return out


def write_base(tmp_path, W, H, types="half", multi=False, planes=None, drop=(), seed=3, noise=False, name="base.exr"):
    """a compression="none" file of seeded channels -> its path.  types: "half" | "float" | "mixed" (velocity, depth float) | "onefloat" (all half
    but diffuse.G)"""
    from rfx_amd import imageio
    ch = {k: v for k, v in X.channels(W, H, seed, planes, noise=noise).items() if k not in drop}
    path = str(tmp_path / name)
    if multi:
        assert types in ("half", "float")
        imageio.write_exr_multipart(path, X.as_parts(ch), "none", half=types == "half")
    else:
        half = {"half": True, "float": False, "mixed": {c for c in ch if c.split(".")[0] in HALF_LAYERS_MIXED}, "onefloat": set(ch) - {"diffuse.G"}}[types]
        imageio.write_exr(path, ch, "none", half=half)
    return path


def device_slots(W, H, path, ctx_args=(), pre=None):
    from rfx_amd import imageio
    from rfx_amd.context import Context
    c = Context(W, H, *ctx_args)
    if pre:
        pre(c)
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data)
    c.stage_exr_aov(data, lay)
    c.stage_flip()
    out = [c.download(t) for t in _slots()], c.exr_aov_status(), lay
    c.close()
    return out


def host_slots(W, H, path, ctx_args=(), pre=None):
    from rfx_amd.context import Context
    c = Context(W, H, *ctx_args)
    if pre:
        pre(c)
    c.stage_aov(host_planes(path))
    c.stage_flip()
    out = [c.download(t) for t in _slots()]
    c.close()
    return out


def assert_same(got, want, what=""):
    from rfx_amd import abi
    for t, a, b in zip(_slots(), got, want):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %s differs in %d texels" % (
            what, abi.TEX_NAMES[t], int((a.reshape(a.shape[0], a.shape[1], -1) != b.reshape(a.shape[0], a.shape[1], -1)).any(-1).sum()))


# (W, H, compression, channel types, multi-part, repack keywords)
FILES = [
    (97, 55, X.ZIPS, "half", False, {}), (97, 55, X.ZIP, "half", True, {}), (97, 55, X.ZIP, "float", False, {}), (97, 55, X.NONE, "mixed", False, {}),
    (97, 55, X.ZIP, "half", False, dict(line_order=1)), (97, 55, X.ZIPS, "float", True, dict(line_order=1)),
    (33, 17, X.ZIP, "mixed", False, {}), (33, 17, X.ZIPS, "onefloat", False, {}), (33, 17, X.ZIP, "float", True, {}), (33, 17, X.NONE, "half", True, {}),
    (1, 1, X.ZIPS, "half", False, {}), (1, 1, X.ZIP, "float", True, {}), (64, 1, X.ZIP, "half", False, {}), (64, 1, X.ZIPS, "float", True, {}),
    (1, 40, X.ZIP, "half", True, {}), (1, 40, X.ZIPS, "mixed", False, {}),
]


@pytest.mark.parametrize("W,H,comp,types,multi,kw", FILES, ids=lambda v: str(v).replace(" ", ""))
def test_device_decode_equals_host_decode(tmp_path, W, H, comp, types, multi, kw):
    """every size, compression, channel typing and file form: the four slots hold the bytes the host decode + stage_aov leaves.  H = 55 and 17
    give ZIP a short last chunk; 97 x 55 leaves the pack kernel a tail."""
    base = write_base(tmp_path, W, H, types, multi)
    path = str(tmp_path / "packed.exr")
    X.repack(base, path, comp, X.zlib_form(6), writer_rule=True, **kw)  # (a chunk whose stream is not smaller stays raw: a file any reader takes)
    got, status, lay = device_slots(W, H, path)
    want_types = {"half": "half", "float": "float"}.get(types)
    for key, (n, t) in lay.planes.items():
        assert t == (want_types or ("float" if (key in ("velocity", "depth") if types == "mixed" else key == "diffuse") else "half")), key
    assert status == (0, -1, 0)
    assert_same(got, host_slots(W, H, base), "%dx%d" % (W, H))
    if comp != X.NONE:  # ... the host reader among them
        assert_same(got, host_slots(W, H, path), "host decode of the packed file")


def test_file_written_by_the_library_writer(tmp_path):
    """imageio.write_exr / write_exr_multipart's own ZIP and ZIPS files (zlib level 4), no repacking"""
    from rfx_amd import imageio
    W, H = 97, 55
    ch = X.channels(W, H, 8)
    a, b = str(tmp_path / "a.exr"), str(tmp_path / "b.exr")
    imageio.write_exr(a, ch, "zip", half={c for c in ch if c.split(".")[0] in HALF_LAYERS_MIXED})
    imageio.write_exr_multipart(b, X.as_parts(ch), "zips", half=True)
    for path in (a, b):
        got, status, _ = device_slots(W, H, path)
        assert status == (0, -1, 0)
        assert_same(got, host_slots(W, H, path), path)


def test_three_channel_diffuse_and_direct(tmp_path):
    W, H = 33, 17
    base = write_base(tmp_path, W, H, "half", drop=("diffuse.A", "direct.A"))
    path = str(tmp_path / "packed.exr")
    X.repack(base, path, X.ZIP, X.zlib_form(6))
    got, status, lay = device_slots(W, H, path)
    assert lay.planes["diffuse"] == (3, "half") and lay.planes["direct"] == (3, "half") and status[0] == 0
    assert_same(got, host_slots(W, H, base))
    assert (got[3][..., 3].view(np.uint32) == 0x3f800000).all()  # alpha 1


@pytest.mark.parametrize("absent", ["velocity", "direct"])
def test_absent_plane_keeps_what_stage_upload_staged(tmp_path, absent):
    from rfx_amd import abi, imageio
    W, H = 33, 17
    planes = [k for k in imageio.AOV_LAYOUT if k != absent]
    base = write_base(tmp_path, W, H, "mixed", planes=planes)
    path = str(tmp_path / "packed.exr")
    X.repack(base, path, X.ZIPS, X.zlib_form(9))
    tex = abi.TEX_VELOCITY if absent == "velocity" else abi.TEX_DIRECT_LIGHT
    other = np.random.default_rng(5).random((H, W, 4), dtype=np.float32)
    pre = lambda c: c.stage_upload(tex, other)  # noqa: E731
    got, status, lay = device_slots(W, H, path, pre=pre)
    assert absent not in lay.planes and status[0] == 0
    assert_same(got, host_slots(W, H, base, pre=pre))
    assert got[_slots().index(tex)].tobytes() == other.tobytes()


FORM_CASES = [(name, dict(level=lv, strategy=st)) for name, (lv, st) in IC.FORMS.items()] + [("full_flush", dict(level=6, flush_every=97)),
                                                                                             ("full_flush_level0", dict(level=0, flush_every=97))]


@pytest.mark.parametrize("name,form", FORM_CASES, ids=[n for n, _ in FORM_CASES])
def test_deflate_forms(tmp_path, name, form):
    """the CPU corpus's deflate forms inside a ZIP file of 33 x 17 (two chunks, the second short): stored, fixed and dynamic blocks, long
    distance-1 matches (roughness is constant here), many blocks.  The pixels are the base file's whatever the stream looks like."""
    W, H = 33, 17
    ch = X.channels(W, H, 4)
    from rfx_amd import imageio
    ch["roughness.Y"] = np.full((H, W), 0.5, np.float32)
    base = str(tmp_path / "base.exr")
    imageio.write_exr(base, ch, "none", half=True)
    path = str(tmp_path / "packed.exr")
    X.repack(base, path, X.ZIP, X.zlib_form(**form))
    got, status, _ = device_slots(W, H, path)
    assert status == (0, -1, 0)
    assert_same(got, host_slots(W, H, base), name)


def one_big_zip_chunk(tmp_path, ch, deflate):
    """600 x 16, eight half channels in one part = ONE ZIP chunk of 153 600 raw bytes, packed by `deflate`; depth and — fed by the diffuse
    channels — direct are staged, roughness and velocity are decoded and dropped.  DEPTH and DIRECT_LIGHT must hold the channels' halves,
    widened.  -> the chunk's record"""
    from rfx_amd import abi, imageio
    from rfx_amd.context import Context
    W, H = 600, 16
    assert sorted(ch) == ["depth.Z", "diffuse.A", "diffuse.B", "diffuse.G", "diffuse.R", "roughness.Y", "velocity.X", "velocity.Y"]
    base, path = str(tmp_path / "base.exr"), str(tmp_path / "packed.exr")
    imageio.write_exr(base, ch, "none", half=True)
    recs = X.repack(base, path, X.ZIP, deflate)
    assert len(recs) == 1
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data, {"direct": ("diffuse.R", "diffuse.G", "diffuse.B", "diffuse.A"), "diffuse": ("-", "-", "-", "-"), "roughness": ("-",),
                                        "velocity": ("-", "-")})
    assert set(lay.planes) == {"depth", "direct"} and int(lay.chunks[0]["rows"]) * 8 * W * 2 == 153600
    a, b = Context(W, H), Context(W, H)
    a.stage_exr_aov(data, lay)
    a.stage_flip()
    b.stage_aov({"depth": ch["depth.Z"].astype(np.float16), "direct": np.stack([ch["diffuse." + c] for c in "RGBA"], -1).astype(np.float16)})
    b.stage_flip()
    assert a.exr_aov_status() == (0, -1, 0)
    for t in (abi.TEX_DEPTH, abi.TEX_DIRECT_LIGHT):
        assert a.download(t).tobytes() == b.download(t).tobytes()
    a.close(); b.close()
    return recs[0]


def test_zip_chunk_of_several_stored_blocks(tmp_path):
    """level 0: the chunk's 153 600 bytes lie in three stored blocks (65 535 bytes is the most one holds)"""
    ch = X.channels(600, 16, planes=("diffuse", "velocity", "depth", "roughness"))
    rec = one_big_zip_chunk(tmp_path, ch, X.zlib_form(0))
    assert rec[4] > 153600 + 3 * 5


def test_zip_chunk_with_matches_at_the_far_end_of_the_window(tmp_path):
    """The device twin of the CPU corpus's period-32768 class: the chunk's 76 800 halves are seeded finite noise that repeats every 32 500
    halves, so its predicted bytes — the low bytes, then the high bytes — repeat every 32 500 bytes and nothing nearer does: level 9 codes the
    repeats as matches of length up to 258 at distance 32 500 (zlib itself emits no distance above 32 768 - 262), each copied by the wave out
    of the far end of a window it wrote tens of kilobytes earlier; what does not repeat stays literals."""
    W, H, period = 600, 16, 32500
    rng = np.random.default_rng(17)
    bits = rng.integers(0, 1 << 16, period).astype(np.uint16)
    bits[(bits & 0x7c00) == 0x7c00] ^= 0x0400  # (no infinity, no NaN)
    flat = np.resize(bits, H * 8 * W).view(np.float16).astype(np.float32).reshape(H, 8, W)  # scanline (top first), channel in file order, x
    names = ["depth.Z", "diffuse.A", "diffuse.B", "diffuse.G", "diffuse.R", "roughness.Y", "velocity.X", "velocity.Y"]
    ch = {n: np.ascontiguousarray(flat[::-1, k]) for k, n in enumerate(names)}  # row 0 = bottom
    rec = one_big_zip_chunk(tmp_path, ch, X.zlib_form(9))
    # literals alone cannot shrink the noise: the stream is far below the raw size only through the distance-32 500 matches
    assert 2 * period < rec[4] < 2 * period + (153600 - 2 * period) // 8


def test_zip_chunk_left_raw_because_noise_does_not_shrink(tmp_path):
    """seeded halves with every bit random: zlib's stream is not smaller, so the writer's rule stores the raw block, which the device copies"""
    W, H = 33, 17
    base = write_base(tmp_path, W, H, "half", noise=True)
    path = str(tmp_path / "packed.exr")
    recs = X.repack(base, path, X.ZIP, X.zlib_form(6), writer_rule=True)
    assert any(size == rows * W * 19 * 2 for _, _, rows, _, size in recs), "the seeded noise shrank: no chunk was stored raw"  # (19 half channels)
    got, status, _ = device_slots(W, H, path)
    assert status == (0, -1, 0)
    assert_same(got, host_slots(W, H, base))
    assert_same(got, host_slots(W, H, path))


def test_two_frames_alternate_and_the_areas_grow(tmp_path):
    """six flips over two files on one context: the small one first (ZIP, half), then one that needs more of every area (NONE, float) — buffers
    are reused, the areas grow once"""
    from rfx_amd import imageio
    from rfx_amd.context import Context
    W, H = 33, 17
    small = str(tmp_path / "small.exr")
    X.repack(write_base(tmp_path, W, H, "half", seed=1, name="b1.exr"), small, X.ZIP, X.zlib_form(9))
    large = write_base(tmp_path, W, H, "float", multi=True, seed=2, name="b2.exr")
    want = [host_slots(W, H, small), host_slots(W, H, large)]
    files = [open(small, "rb").read(), open(large, "rb").read()]
    lays = [imageio.exr_aov_layout(f) for f in files]
    c = Context(W, H)
    assert c.exr_aov_stage_bytes(files[0], lays[0]) < c.exr_aov_stage_bytes(files[1], lays[1])
    for k in range(6):
        c.stage_exr_aov(files[k & 1], lays[k & 1])
        c.stage_flip()
        assert c.exr_aov_status()[0] == 0
        assert_same([c.download(t) for t in _slots()], want[k & 1], "flip %d" % k)
    c.close()


def test_band_of_a_row_tiled_context(tmp_path):
    """tile rows 16 .. 39 of 97 x 55 with a halo of 3: the band's scanlines 15 .. 38 cut ZIP chunks at both edges (chunks 0, 1 and 2 of four).
    Only those are copied; the rest of the frame is staged by a second call; the slots equal the host path's on the same tile."""
    from rfx_amd import abi, imageio
    from rfx_amd.context import Context
    W, H, args = 97, 55, (0, 16, 24, 3)
    base = write_base(tmp_path, W, H, "mixed")
    path = str(tmp_path / "packed.exr")
    X.repack(base, path, X.ZIP, X.zlib_form(6))
    data = open(path, "rb").read()
    lay = imageio.exr_aov_layout(data)
    a, b = Context(W, H, *args), Context(W, H, *args)
    r0, n = a.held_rows(abi.TEX_GBUFFER)
    assert (r0, n) == (13, 30)
    need = lay.band_chunks(16, 24)
    assert [int(y) for y in need["y"]] == [0, 16, 32] and a.exr_aov_stage_bytes(data, lay, 16, 24) == int(need["packed_bytes"].sum())
    assert a.exr_aov_stage_bytes(data, lay) == int(lay.chunks["packed_bytes"].sum())
    planes = host_planes(base)
    for row0, rows in ((16, 24), (0, 16), (40, 15)):  # the tile's rows, then the rest of DEPTH (and of the halo) in two more bands
        a.stage_exr_aov(data, lay, row0, rows)
        assert a.exr_aov_status()[0] == 0
        b.stage_aov({k: v[row0:row0 + rows] for k, v in planes.items()}, row0, rows)
    a.stage_flip(); b.stage_flip()
    assert_same([a.download(t) for t in _slots()], [b.download(t) for t in _slots()])
    a.close(); b.close()


def test_status_reports_the_chunk_whose_trailer_is_flipped(tmp_path):
    """the one corrupt input sent to a device: a chunk whose Adler-32 trailer has a bit flipped.  It is the chunk reported, its rows read as not
    covered, every other row is the clean frame's."""
    from rfx_amd import abi
    W, H = 97, 55
    base = write_base(tmp_path, W, H, "half", multi=True)
    path = str(tmp_path / "packed.exr")
    recs = X.repack(base, path, X.ZIP, X.zlib_form(6))
    clean, status, lay = device_slots(W, H, path)
    assert status == (0, -1, 0)
    layers = list(X.as_parts(X.channels(W, H)))  # part order
    victim = next(i for i, r in enumerate(recs) if r[0] == layers.index("emissive") and r[1] == 16)  # scanlines 16 .. 31 of the emissive part
    X.flip_adler_byte(path, recs[victim])
    got, status, lay = device_slots(W, H, path)
    assert status == (1, victim, 10)  # K9_E_ADLER
    rows = slice(H - 32, H - 16)  # frame rows of scanlines 16 .. 31
    depth, gbuffer, velocity, direct = got
    assert (depth[rows] == 1.0).all()
    assert (gbuffer[rows].reshape(-1, 4).view(np.uint32) == np.array([0, 0, 0, 0x3f800000], np.uint32)).all()
    assert (velocity[rows].reshape(-1, 4).view(np.uint32) == np.array([0, 0, 0, 0x3f800000], np.uint32)).all()
    keep = np.ones(H, bool)
    keep[rows] = False
    for g, w in zip(got, clean):
        assert g[keep].tobytes() == w[keep].tobytes()
    assert direct[rows].tobytes() == clean[3][rows].tobytes()  # (the direct part decoded: its samples are staged as they are)


def test_refusals(tmp_path):
    from rfx_amd import abi, imageio
    from rfx_amd.context import Context
    W, H = 33, 17
    path = str(tmp_path / "packed.exr")
    X.repack(write_base(tmp_path, W, H, "half", multi=True), path, X.ZIP, X.zlib_form(6))
    data = open(path, "rb").read()
    c = Context(W, H)

    def rc(mutate, row0=0, rows=H):
        lay = imageio.exr_aov_layout(data)
        lay.chunks = lay.chunks.copy()
        mutate(lay)
        f, keep = c._exr_frame(data, lay)
        assert c.lib.rfx_exr_aov_stage_bytes(c._h, C.byref(f), row0, rows) == 0
        r = c.lib.rfx_stage_exr_aov(c._h, C.byref(f), row0, rows)
        assert r != 0 and b"rfx_stage_exr_aov" in c.lib.rfx_last_error(c._h)
        return r

    def part(lay, k, comp=None, chan=None):
        comp0, chans = lay.parts[k]
        lay.parts[k] = (comp0 if comp is None else comp, chans if chan is None else chan(list(chans)))
    depth_part = [i for i, (_, ch) in enumerate(imageio.exr_aov_layout(data).parts) if any(pl == 6 for _, pl, _ in ch)][0]
    layers = list(imageio.AOV_LAYOUT)
    E = abi.RFX_EINVAL
    assert c.exr_aov_stage_bytes(data, imageio.exr_aov_layout(data)) > 0
    assert rc(lambda l: part(l, 0, chan=lambda ch: [(0,) + ch[0][1:]] + ch[1:])) == E                    # a UINT channel
    assert rc(lambda l: part(l, 0, comp=4)) == E                                                        # PIZ
    assert rc(lambda l: part(l, 0, comp=1)) == E                                                        # RLE
    assert rc(lambda l: l.chunks["offset"].__setitem__(3, len(data) - 2)) == E                          # a chunk outside the file bytes
    assert rc(lambda l: l.chunks["rows"].__setitem__(0, 15)) == E                                       # rows that do not fit the header
    assert rc(lambda l: l.chunks["y"].__setitem__(1, 8)) == E                                           # a scanline that is no multiple of 16
    assert rc(lambda l: l.chunks["part"].__setitem__(0, 99)) == E                                       # a part that does not exist
    assert rc(lambda l: l.chunks["y"].__setitem__(1, 0)) == E                                           # two chunks on one scanline (and one missing)
    assert rc(lambda l: part(l, depth_part, chan=lambda ch: [(ch[0][0], -1, 0)])) == E                  # no depth
    assert rc(lambda l: part(l, layers.index("emissive"), chan=lambda ch: [(p, -1, 0) for p, _, _ in ch])) == E  # a partial G-buffer set
    assert rc(lambda l: part(l, layers.index("normal"), chan=lambda ch: [ch[0], ch[0], ch[2]])) == E   # a component fed twice
    assert rc(lambda l: None, 0, H + 1) == E                                                            # a band outside DEPTH's rows
    c.close()


def test_sequence_and_whole_file_entry_points(tmp_path):
    """frames.ExrSequence over a directory (two pinned file buffers, readinto) and Context.stage_exr_frame: every frame's slots are the host
    decode's; a PIZ file in the sequence goes the host's way by itself"""
    from rfx_amd import frames, imageio
    from rfx_amd.context import Context
    W, H = 33, 17
    d = tmp_path / "seq"
    d.mkdir()
    kinds = ("zip", "zips", "piz", "zip")
    for i, comp in enumerate(kinds):
        imageio.write_exr(str(d / ("f%02d.exr" % i)), X.channels(W, H, 20 + i), comp, half={c for c in X.channels(1, 1) if c.split(".")[0] in HALF_LAYERS_MIXED})
    c = Context(W, H)
    seq = frames.ExrSequence(c, str(d))
    assert len(seq) == 4
    for i in range(len(seq)):
        assert seq.stage(i) == ("host" if kinds[i] == "piz" else "device")
        c.stage_flip()
        assert_same([c.download(t) for t in _slots()], host_slots(W, H, seq.paths[i]), "frame %d" % i)
    assert c.stage_exr_frame(seq.paths[0]) == "host" and c.stage_exr_frame(seq.paths[1], decode="device") == "device"  # (the later call's frame wins)
    c.stage_flip()
    assert_same([c.download(t) for t in _slots()], host_slots(W, H, seq.paths[1]))
    assert c.stage_exr_frame(seq.paths[2], decode="device") == "host"
    c.stage_flip()
    assert_same([c.download(t) for t in _slots()], host_slots(W, H, seq.paths[2]))
    with pytest.raises(ValueError):
        c.stage_exr_frame(seq.paths[0], decode="gpu")
    c.close()
