"""EER rendering (render_eer_raw, read_eer, EerMovie, eer_frames_per_fraction), without a GPU: the names, parameter
lists and defaults, the header and the ctypes table on mc_eer_render, the codec rule's restatement
(tests/eer_reference.py) on hand-made streams, read_eer on TIFF and BigTIFF files written here, every refusal before
any device is touched, the entry point's host checks with fake pointers, and the three passes' per-lane bodies run
lane by lane on the CPU under the address and undefined-behaviour sanitizers (tests/host_eer.cpp, a stand-alone
program started as a child process)."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import eer_reference as er
from kernel_harness import assert_entry_point, run_host_program
import torch_motion_correction_amd as mc
from torch_motion_correction_amd import _lib, eer


def test_names_parameter_lists_and_defaults():
    for name in ("render_eer_raw", "read_eer", "EerMovie", "eer_frames_per_fraction"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(eer, name)
    sig = inspect.signature(mc.render_eer_raw)
    assert list(sig.parameters) == ["data", "offsets", "nbytes", "shape", "group", "upsampling", "rle_bits",
                                    "return_event_counts", "device"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(upsampling=1, rle_bits=7, return_event_counts=False, device=None)
    assert list(inspect.signature(mc.read_eer).parameters) == ["path"]
    sig = inspect.signature(mc.EerMovie.render)
    assert list(sig.parameters) == ["self", "group", "upsampling", "device"]
    assert sig.parameters["upsampling"].default == 1 and sig.parameters["device"].default is None
    assert [f for f in mc.EerMovie.__dataclass_fields__] == ["data", "offsets", "nbytes", "shape", "rle_bits"]
    assert list(inspect.signature(mc.eer_frames_per_fraction).parameters) == [
        "n_frames", "total_fluence", "dose_per_output_frame"]


def test_header_signatures_and_build_agree():
    from torch_motion_correction_amd import _build

    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert_entry_point("mc_eer_render", [vp, i64, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp],
                       source=("eer_render.hip", "eer_render", []))
    # the segment size the wrapper asks for is one the header's records hold and the entry point takes
    text = open(os.path.join(_build.CSRC, "eer.h")).read()
    assert int(re.search(r"SEG_MAX = (\d+)", text).group(1)) == 256 and eer.SEGMENT_BYTES in (64, 128, 256)


# ------------------------------------------------------------------ the rule on hand-made streams


def _as_int(strip):
    return int.from_bytes(strip, "little")


def test_rule_on_hand_made_streams():
    N = 200
    # an empty frame: one skip and a run of 73, 14 bits
    s = er.encode_frame([], [], N)
    assert len(s) == 2 and _as_int(s) == 127 | 73 << 7
    assert er.decode_frame(s, N) == ([], [], N)
    # an event after exactly 126, 127 and 128 empty pixels
    s = er.encode_frame([126], [5], N)
    assert len(s) == 3 and _as_int(s) == 126 | 5 << 7 | 73 << 11
    assert er.decode_frame(s, N) == ([126], [5], N)
    s = er.encode_frame([127], [9], N)  # a skip, then a run of 0 with its code
    assert len(s) == 4 and _as_int(s) == 127 | 0 << 7 | 9 << 14 | 72 << 18
    assert er.decode_frame(s, N) == ([127], [9], N)
    s = er.encode_frame([128], [15], N)
    assert len(s) == 4 and _as_int(s) == 127 | 1 << 7 | 15 << 14 | 71 << 18
    assert er.decode_frame(s, N) == ([128], [15], N)
    # an event on the last pixel: a trailing run of 0
    s = er.encode_frame([3, N - 1], [1, 2], N)
    assert _as_int(s) == 3 | 1 << 7 | 127 << 11 | (N - 1 - 4 - 127) << 18 | 2 << 25 | 0 << 29 and len(s) == 5
    assert er.decode_frame(s, N) == ([3, N - 1], [1, 2], N)
    # a trailing run that is a multiple of 127: skips only, the decoder stops at n == N
    s = er.encode_frame([145], [7], 400)  # 145 = 127 + 18, then 254 pixels remain
    assert len(s) == 4 and _as_int(s) == 127 | 18 << 7 | 7 << 14 | 127 << 18 | 127 << 25
    assert er.decode_frame(s, 400) == ([145], [7], 400)
    s = er.encode_frame([], [], 381)  # a frame of three skips
    assert len(s) == 3 and _as_int(s) == 0x1fffff and er.decode_frame(s, 381) == ([], [], 381)
    # a full frame: N runs of 0 with codes, then a run of 0
    codes = [k % 16 for k in range(N)]
    s = er.encode_frame(list(range(N)), codes, N)
    assert len(s) == (11 * N + 7 + 7) // 8
    assert er.decode_frame(s, N) == (list(range(N)), codes, N)
    # malformed: cut short (n never reaches N), a last run that overshoots
    assert er.decode_frame(s[:40], N)[2] < N
    over = (127 | 100 << 7).to_bytes(2, "little")
    assert er.decode_frame(over, N) == ([], [], 227)
    assert er.decode_frame(b"", N) == ([], [], 0)


def test_round_trip_and_renderer_on_random_frames():
    rng = np.random.default_rng(3)
    h, w = 12, 20
    strips, want1, want2 = [], np.zeros((2, h, w), np.uint8), np.zeros((2, 2 * h, 2 * w), np.uint8)
    for f, d in enumerate((0.0, 1.0, 0.3, 0.01, 0.6)):
        pos, sub = er.random_frame(rng, h * w, d)
        strips.append(er.encode_frame(pos, sub, h * w))
        got = er.decode_frame(strips[-1], h * w)
        assert got == (pos.tolist(), sub.tolist(), h * w)
        if f < 4:
            for p, s in zip(pos.tolist(), sub.tolist()):
                want1[f // 2, p // w, p % w] += 1
                want2[f // 2, 2 * (p // w) + ((s >> 3) & 1), 2 * (p % w) + ((s >> 1) & 1)] += 1
    movie, final_n, counts = er.render(strips, (h, w), 2)
    assert movie.shape == (2, h, w) and np.array_equal(movie, want1) and list(final_n) == [h * w] * 5
    assert counts[0] == 0 and counts[1] == h * w
    assert np.array_equal(er.render(strips, (h, w), 2, upsampling=2)[0], want2)


# ------------------------------------------------------------------ containers


def _strips(rng, shape, n):
    return [er.encode_frame(*er.random_frame(rng, shape[0] * shape[1], 0.2), shape[0] * shape[1]) for _ in range(n)]


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("byte_order", ["<", ">"])
def test_read_eer_on_both_containers(tmp_path, big, byte_order):
    rng = np.random.default_rng(11)
    shape = (9, 12)
    strips = _strips(rng, shape, 5)
    path = tmp_path / "movie.eer"
    # strips out of order, each at an odd offset, each followed by its IFD
    offsets, nbytes = er.write_tiff(path, strips, shape, big=big, order=[3, 0, 4, 1, 2], byte_order=byte_order)
    assert all(o % 2 == 1 for o in offsets) and offsets != sorted(offsets)
    movie = mc.read_eer(path)
    assert isinstance(movie, mc.EerMovie) and movie.shape == shape and movie.rle_bits == 7
    assert movie.offsets == offsets and movie.nbytes == nbytes
    assert movie.data.dtype == torch.uint8 and movie.data.dim() == 1 and movie.data.numel() == os.path.getsize(path)
    for o, n, s in zip(movie.offsets, movie.nbytes, strips):
        assert bytes(movie.data[o:o + n].tolist()) == s
    # compression 65002 with the default layout, stated or not
    er.write_tiff(path, strips, shape, big=big, compression=65002, byte_order=byte_order)
    assert mc.read_eer(path).shape == shape
    er.write_tiff(path, strips, shape, big=big, compression=65002, byte_order=byte_order,
                  overrides={i: {65007: (3, 1, 7), 65008: (3, 1, 2), 65009: (3, 1, 2)} for i in range(5)})
    assert mc.read_eer(str(path)).nbytes == nbytes


@pytest.mark.parametrize("big", [False, True])
def test_read_eer_refusals_name_the_tag(tmp_path, big):
    rng = np.random.default_rng(12)
    shape = (9, 12)
    strips = _strips(rng, shape, 3)
    path = tmp_path / "bad.eer"

    def refuse(match, **kw):
        er.write_tiff(path, strips, shape, big=big, **kw)
        with pytest.raises(ValueError, match=match):
            mc.read_eer(path)

    refuse("Compression 65000", compression=65000)
    refuse("Compression 1 ", compression=1)
    refuse(r"65002 with .*\(8, 2, 2\)", compression=65002, overrides={0: {65007: (3, 1, 8)}})
    refuse("frame 2: Compression 65002 differs", overrides={2: {259: (3, 1, 65002)}})
    refuse("frame 1: ImageLength x ImageWidth", overrides={1: {256: (4, 1, 13)}})
    for tag, name in ((256, "ImageWidth"), (257, "ImageLength"), (259, "Compression"), (273, "StripOffsets"),
                      (279, "StripByteCounts")):
        refuse(f"frame 1: {name} is missing", overrides={1: {tag: None}})
    refuse("frame 0: StripOffsets has 2 values", overrides={0: {273: (4, 2, 64)}})
    refuse("frame 0: StripByteCounts has 2 values", overrides={0: {279: (4, 2, 64)}})
    refuse("ImageWidth has TIFF type 5", overrides={0: {256: (5, 1, 64)}})
    refuse("frame 2: StripOffsets \\+ StripByteCounts", overrides={2: {279: (4, 1, 10**6)}})
    path.write_bytes(b"II" + (44).to_bytes(2, "little") + bytes(12))
    with pytest.raises(ValueError, match="magic 44"):
        mc.read_eer(path)
    path.write_bytes(b"PK\x03\x04" + bytes(12))
    with pytest.raises(ValueError, match="not a TIFF"):
        mc.read_eer(path)
    path.write_bytes((b"II+\x00\x08\x00\x00\x00" + bytes(8)) if big else (b"II*\x00" + bytes(4)))
    with pytest.raises(ValueError, match="no frame"):
        mc.read_eer(path)


# ------------------------------------------------------------------ argument rules, devices refused


def _refuse_devices(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(eer, "require_gpu", refuse)
    monkeypatch.setattr(eer, "device_scope", refuse)


def test_argument_rules_hold_before_any_device_is_touched(monkeypatch, tmp_path):
    _refuse_devices(monkeypatch)
    data = torch.zeros(100, dtype=torch.uint8)
    ok = dict(data=data, offsets=[0, 10, 20], nbytes=[10, 10, 10], shape=(8, 8), group=1)

    def refuse(match, **kw):
        with pytest.raises(ValueError, match=match):
            mc.render_eer_raw(**{**ok, **kw})

    for bad in (np.zeros(100, np.uint8), torch.zeros(100, dtype=torch.int16), torch.zeros(10, 10, dtype=torch.uint8),
                b"abc"):
        refuse("1-D uint8 tensor", data=bad)
    for bad in ((8,), (8, 8, 8), (0, 8), (8, -1), 8, (8.0, 8)):
        refuse(r"\(h, w\)", shape=bad)
    refuse("2\\^31 pixels", shape=(1 << 16, 1 << 15))
    refuse("65000", rle_bits=8)
    refuse("rle_bits", rle_bits=6)
    for bad in (4, 3, 0, True, 2.5, None):
        refuse("upsampling must be 1 or 2", upsampling=bad)
    refuse("multiple of 4", shape=(8, 6))
    refuse("multiple of 4", shape=(8, 9), upsampling=2)
    for bad in (0, -1, 2.0, None, True, "3"):
        refuse("group must be an int >= 1", group=bad)
    refuse("at most 255 frames", group=256, offsets=[0] * 300, nbytes=[1] * 300)
    refuse("needs at least that many frames", group=4)
    refuse("same frames", offsets=[0, 10])
    refuse("same frames", offsets=[], nbytes=[])
    refuse("sequences of ints", offsets=5)
    refuse("an offset must be an int >= 0", offsets=[0, -1, 20])
    refuse("a byte count must be an int >= 0", nbytes=[10, 1.5, 10])
    refuse("frame 2: its strip .* leaves the 100 bytes", offsets=[0, 10, 95])
    refuse("frame 1: its strip", nbytes=[10, 91, 10])
    refuse("frame 0: strips of 2\\^28 bytes", data=torch.zeros(1, dtype=torch.uint8).expand(2**28 + 1),
           offsets=[0], nbytes=[2**28])
    # EerMovie.render goes through the same rules
    movie = mc.EerMovie(data=data, offsets=[0], nbytes=[10], shape=(8, 8), rle_bits=7)
    with pytest.raises(ValueError, match="upsampling must be 1 or 2"):
        movie.render(1, upsampling=4)
    with pytest.raises(ValueError, match="65000"):
        mc.EerMovie(data=data, offsets=[0], nbytes=[10], shape=(8, 8), rle_bits=8).render(1)


def test_frames_per_fraction():
    f = mc.eer_frames_per_fraction
    assert f(1000, 50.0, 1.0) == 20 and f(1000, 50.0, 0.5) == 10 and f(3000, 40, 1) == 75
    assert f(10, 50.0, 1.0) == 1 and f(7, 1.0, 1.0) == 7  # never below 1
    assert f(1000, 40.0, 0.9) == round(0.9 * 1000 / 40.0) == 22
    for bad in (dict(n_frames=0), dict(n_frames=2.5), dict(total_fluence=0.0), dict(total_fluence=float("nan")),
                dict(dose_per_output_frame=-1.0), dict(dose_per_output_frame=float("inf"))):
        with pytest.raises(ValueError):
            f(**{**dict(n_frames=100, total_fluence=50.0, dose_per_output_frame=1.0), **bad})


def test_entry_point_validates_on_the_host():
    """Fake device pointers and a null stream: every call below must answer before it touches or launches anything."""
    lib = _lib.load()
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(5)]
    ARG, UNSUPPORTED = -1, -2
    i64x = lambda v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731

    def call(data=p[0], data_bytes=1000, offsets=(0, 100, 200), nbytes=(100, 100, 100), n=3, h=8, w=8, rle=7, up=1,
             g=1, seg=128, out=p[1], final_n=p[2], events=p[3], scratch=p[4], scratch_bytes=1 << 20):
        off = None if offsets is None else i64x(offsets)
        nb = None if nbytes is None else i64x(nbytes)
        return lib.mc_eer_render(data, data_bytes, off, nb, n, h, w, rle, up, g, seg, out, final_n, events, scratch,
                                 scratch_bytes, None)

    for name in ("data", "offsets", "nbytes", "out", "final_n", "events", "scratch"):
        assert call(**{name: None}) == ARG, name
    assert call(n=0) == ARG and call(h=0) == ARG and call(w=-1) == ARG and call(g=0) == ARG and call(g=-3) == ARG
    assert call(data_bytes=-1) == ARG
    assert call(rle=8) == UNSUPPORTED and call(rle=6) == ARG  # compression 65000
    assert call(up=4) == UNSUPPORTED and call(up=3) == ARG and call(up=0) == ARG
    assert call(g=256, n=3) == UNSUPPORTED  # a uint8 count
    assert call(g=4) == ARG  # n_frames < g
    for seg in (16, 32, 100, 512, 0):
        assert call(seg=seg) == UNSUPPORTED, seg
    assert call(h=1 << 16, w=1 << 15) == UNSUPPORTED  # N = 2^31
    assert call(w=6) == UNSUPPORTED and call(w=9, up=2) == UNSUPPORTED
    assert call(w=6, up=2, scratch_bytes=0) == ARG  # 2 w = 12 is whole words: only the scratch is refused
    assert call(out=ctypes.c_void_p(0x200002)) == ARG and call(final_n=ctypes.c_void_p(0x300001)) == ARG
    assert call(events=ctypes.c_void_p(0x400002)) == ARG and call(scratch=ctypes.c_void_p(0x500004)) == ARG
    assert call(offsets=(0, -1, 200)) == ARG and call(nbytes=(100, -5, 100)) == ARG
    assert call(offsets=(0, 100, 901)) == ARG and call(offsets=(0, 100, 2000)) == ARG  # a strip leaves the buffer
    assert call(data_bytes=1 << 40, nbytes=(100, 1 << 28, 100)) == UNSUPPORTED
    # the scratch: 24 n + 52 segments bytes (three strips of 100 bytes are three segments of 128)
    assert call(scratch_bytes=24 * 3 + 52 * 3 - 1) == ARG and call(seg=64, scratch_bytes=24 * 3 + 52 * 6 - 1) == ARG


# ------------------------------------------------------------------ the passes' bodies on the CPU, sanitized


def test_pass_bodies_on_the_host_under_sanitizers(tmp_path):
    """csrc/eer.h -- the per-lane bodies eer_render.hip compiles for the device -- is built for the host with
    -fsanitize=address,undefined into a program of its own and run as a child process: the three passes lane by lane
    on exactly-sized heap buffers, segment sizes 16 .. 256, the mixed densities of tests/test_eer_render.py, 255 full
    frames, streams cut short, overshooting, empty and of one byte, every frame also alone in an allocation of its own
    bytes, against a bit-by-bit sequential decode in the same program.  Nothing sanitized is loaded into this
    process."""
    res = run_host_program("host_eer.cpp", tmp_path)
    assert res.stdout.count(": ok") == 98
