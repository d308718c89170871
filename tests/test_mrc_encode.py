"""MRC encode on the GPU (encode_mrc_raw, write_mrc_raw: mc_mrc_encode, csrc/mrc_encode.hip over csrc/mrc_encode.h)
against the numpy restatement of tests/mrc_encode_reference.py.  The encoder moves bytes and sums integers: equality
throughout.  Every payload the kernel writes here lies inside a NaN-guarded allocation (kernel_harness.byte_buffer) at
an odd address, and the guards are looked at after every launch."""

import struct

import numpy as np
import pytest
import torch

import mrc_encode_reference as er
from kernel_harness import assert_byte_guards, byte_buffer

pytestmark = pytest.mark.gpu

# one-sample rows; an odd width above one 16-byte unit; several units a row and rows at every alignment; a row longer
# than a workgroup; more rows than resident workgroups; more row-threads a frame than 1024 workgroups hold (the
# grid-stride loop: 1040 rows of 258 (uint8) or 514 (int16) row-threads)
SHAPES = [(3, 5, 1), (2, 7, 33), (2, 37, 129), (1, 3, 4099), (2, 3000, 17), (1, 1040, 4099)]


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def run(dev, px, mode, flip=False, past=1, on_gpu=True):
    """mrc._encode of `px` into a guarded payload `past` bytes beyond a 16-byte boundary -> (payload bytes, table),
    the guards checked."""
    from torch_motion_correction_amd import mrc

    t, h, w = px.shape
    movie = torch.from_numpy(px)
    out, whole = byte_buffer(t * h * er.row_bytes(mode, w), dev, past=past)
    assert out.data_ptr() % 2 == 1
    got, table = mrc._encode(movie.to(dev) if on_gpu else movie, t, h, w, mode, flip, dev, out=out)
    torch.cuda.synchronize()
    what = f"{px.dtype} -> mode {mode} {px.shape} flip {flip}"
    assert got.data_ptr() == out.data_ptr() and table.device.type == "cpu" and table.dtype == torch.int64
    assert_byte_guards(out, whole, what)
    return bytes(got.cpu().numpy()), table.numpy(), what


@pytest.mark.parametrize("dtype,mode", er.KINDS)
def test_payload_and_statistics_equal_the_restatement(dev, dtype, mode):
    for n, shape in enumerate(SHAPES):
        px = er.pixels(dtype, mode, shape, seed=n)
        want_table = er.statistics(px, mode)
        assert not want_table[:, 4].any()
        for flip in (False, True):
            got, table, what = run(dev, px, mode, flip, past=(1, 3, 7, 13)[n % 4])
            assert got == er.encode(px, mode, flip), what
            assert np.array_equal(table, want_table), what


def test_extreme_frames(dev):
    px = np.full((1, 64, 64), -32768, dtype=np.int16)  # the largest sum of squares a sample gives
    got, table, what = run(dev, px, 1)
    assert got == er.encode(px, 1) and table.tolist() == [[-32768, -32768, -32768 * 4096, 2**30 * 4096, 0]]
    for dtype in ("u1", "i2"):
        px = np.full((2, 7, 33), 15, dtype=dtype)
        got, table, what = run(dev, px, 101, past=5)
        assert got == er.encode(px, 101) and got == (b"\xff" * 16 + b"\x0f") * 14, what  # the padding nibble is 0
        assert table.tolist() == [[15, 15, 15 * 231, 225 * 231, 0]] * 2


@pytest.mark.parametrize("dtype,mode", er.KINDS)
def test_cpu_and_gpu_input_give_the_same_bytes(mc, dev, dtype, mode):
    px = er.pixels(dtype, mode, (2, 37, 129), seed=11)
    a, ta, _ = run(dev, px, mode, on_gpu=True)
    b, tb, _ = run(dev, px, mode, on_gpu=False)
    assert a == b == er.encode(px, mode) and np.array_equal(ta, tb)
    # the public route: an MrcMovie on the device whose decode is the movie
    for movie in (torch.from_numpy(px), torch.from_numpy(px).to(dev)):
        enc, table = mc.encode_mrc_raw(movie, mode=mode, return_statistics=True, device=dev)
        assert isinstance(enc, mc.MrcMovie) and enc.data.device == dev and enc.data.dtype == torch.uint8
        assert enc.data.dim() == 1 and bytes(enc.data.cpu().numpy()) == a and np.array_equal(table.numpy(), ta)
        assert (enc.offset, enc.shape, enc.mode, enc.swap, enc.pixel_spacing) == (0, (2, 37, 129), mode, False, None)
        assert enc.unsigned_bytes is ((dtype, mode) == ("u1", 0))
        back = enc.decode(device=dev)
        assert back.dtype == (torch.uint8 if mode == 101 or dtype == "u1" else torch.int16)
        assert torch.equal(back.cpu().long(), torch.from_numpy(px).long())
    # the default mode, and one image
    enc = mc.encode_mrc_raw(torch.from_numpy(px[0]), device=dev)
    assert enc.mode == (0 if dtype == "u1" else 1) and enc.shape == (1, 37, 129)
    if mode == enc.mode:
        assert bytes(enc.data.cpu().numpy()) == er.encode(px[:1], mode)
    flipped = mc.encode_mrc_raw(torch.from_numpy(px), mode=mode, flip_rows=True, device=dev)
    assert bytes(flipped.data.cpu().numpy()) == er.encode(px, mode, True)
    assert torch.equal(flipped.decode(device=dev, flip_rows=True).cpu().long(), torch.from_numpy(px).long())


@pytest.mark.parametrize("dtype,mode,value,lo,hi", [("u1", 101, 16, 0, 15), ("i2", 101, 16, 0, 15), ("i2", 6, -1, 0, 32767),
                                                    ("i2", 0, 128, -128, 127)])
def test_one_sample_out_of_range_is_refused(mc, dev, tmp_path, dtype, mode, value, lo, hi):
    px = er.pixels(dtype, mode, (2, 37, 129), seed=13)
    px[1, 20, 77] = value
    want = er.statistics(px, mode)
    assert want[:, 4].tolist() == [0, 1]
    got, table, what = run(dev, px, mode)
    assert got == er.encode(px, mode) and np.array_equal(table, want), what  # masked to the field, and counted
    message = (f"mode {mode} holds values {lo} .. {hi}: 1 samples of the movie lie outside \\(its minimum is "
               f"{int(px.min())}, its maximum {int(px.max())}\\)")
    with pytest.raises(ValueError, match=message):
        mc.encode_mrc_raw(torch.from_numpy(px), mode=mode, device=dev)
    path = tmp_path / "refused.mrc"
    with pytest.raises(ValueError, match=message):
        mc.write_mrc_raw(path, torch.from_numpy(px).to(dev), 1.0, mode=mode)
    assert not path.exists()
    px[1, 20, 77] = hi if value > hi else lo
    assert mc.encode_mrc_raw(torch.from_numpy(px), mode=mode, device=dev).mode == mode


@pytest.mark.parametrize("dtype,mode", er.KINDS)
def test_file_round_trip(mc, dev, tmp_path, monkeypatch, dtype, mode):
    from torch_motion_correction_amd import mrc

    monkeypatch.setattr(mrc, "_CHUNK_BYTES", 3 * 37 * er.row_bytes(mode, 129) + 5)  # three frames a chunk, then two
    shape = (5, 37, 129)
    px = er.pixels(dtype, mode, shape, seed=17)
    movie = torch.from_numpy(px)
    path = tmp_path / "movie.mrc"
    for flip in (False, True):
        assert mc.write_mrc_raw(path, movie.to(dev) if flip else movie, 0.83, mode=mode, flip_rows=flip, device=dev) == path
        raw = path.read_bytes()
        assert len(raw) == 1024 + 5 * 37 * er.row_bytes(mode, 129) and raw[1024:] == er.encode(px, mode, flip)
        back = mc.read_mrc(path)
        assert (back.mode, back.shape, back.offset, back.swap) == (mode, shape, 1024, False)
        assert back.unsigned_bytes is ((dtype, mode) == ("u1", 0)) and back.pixel_spacing == pytest.approx(0.83, rel=1e-6)
        got = back.decode(device=dev, flip_rows=flip)
        assert got.dtype == (torch.uint8 if mode == 101 or dtype == "u1" else torch.int16)
        assert torch.equal(got.cpu().long(), movie.long())
        # the header: write_mrc's fields, and the four statistics of the movie
        nx, ny, nz, m = struct.unpack_from("<4i", raw, 0)
        assert (nz, ny, nx, m) == (*shape, mode) and struct.unpack_from("<3i", raw, 28) == (nx, ny, nz)
        assert struct.unpack_from("<3i", raw, 64) == (1, 2, 3) and struct.unpack_from("<2i", raw, 88) == (0, 0)
        assert struct.unpack_from("<3f", raw, 40) == pytest.approx((nx * 0.83, ny * 0.83, nz * 0.83), rel=1e-6)
        assert struct.unpack_from("<3f", raw, 52) == (90.0, 90.0, 90.0) and raw[104:108] == bytes(4)
        assert struct.unpack_from("<i", raw, 108)[0] == 20140 and raw[208:216] == b"MAP \x44\x44\x00\x00"
        assert struct.unpack_from("<2i", raw, 152) == ((1146047817, 0) if (dtype, mode) == ("u1", 0) else (0, 0))
        assert struct.unpack_from("<i", raw, 220)[0] == 1 and b"torch_motion_correction_amd" in raw[224:304]
        dmin, dmax, dmean, rms = er.header_statistics(px)
        assert struct.unpack_from("<2f", raw, 76) == (dmin, dmax)
        # float32 fields (2^-24) of exactly rounded values against float64 numpy
        assert struct.unpack_from("<f", raw, 84)[0] == pytest.approx(dmean, rel=1e-6, abs=1e-6)
        assert struct.unpack_from("<f", raw, 216)[0] == pytest.approx(rms, rel=1e-6)


def test_counts_to_4_bit_file_to_statistics(mc, dev, tmp_path):
    """uint8 event counts as render_eer_raw gives them -> a mode-101 file -> read_mrc(...).decode() ->
    RawStatistics.add: the sums of the original movie."""
    shape = (4, 37, 129)
    counts = torch.from_numpy(np.minimum(np.random.default_rng(5).poisson(1.5, shape), 15).astype(np.uint8)).to(dev)
    path = mc.write_mrc_raw(tmp_path / "counts.mrc", counts, 0.5, mode=101)
    assert path.stat().st_size == 1024 + 4 * 37 * 65
    movie = mc.read_mrc(path).decode(device=dev)
    assert movie.dtype == torch.uint8 and torch.equal(movie, counts)
    a = mc.RawStatistics(shape[1:], device=dev).add(movie)
    b = mc.RawStatistics(shape[1:], device=dev).add(counts)
    assert a.frames == b.frames == 4 and torch.equal(a.sum, b.sum) and torch.equal(a.sumsq, b.sumsq)
