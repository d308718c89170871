"""TIFF LZW decode on the GPU (decode_tiff_raw: mc_tiff_decode, csrc/tiff_decode.hip over csrc/tiff_lzw.h) against the
committed libtiff-written files and the sequential decoder of tests/tiff_reference.py.  The decoder moves bytes:
torch.equal throughout.  Every output buffer lies inside a guarded allocation (kernel_harness.byte_buffer), so a write
outside the movie shows."""

import os

import numpy as np
import pytest
import torch

import tiff_reference as tr
from kernel_harness import assert_byte_guards, byte_buffer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_lzw_libtiff.npz")
NAMES = ("u8_strips", "u8_long_strip", "u16", "f32", "u8_stored")


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def decode(dev, data, offsets, nbytes, shape, rps, compression=5, dtype=torch.uint8):
    """decode_tiff_raw's own steps with the output in a guarded buffer -> (movie bytes on the CPU, produced)."""
    from torch_motion_correction_amd import tiff

    flat_o, flat_n, t, spf, h, w, rps = tiff._check_decode_args(data, offsets, nbytes, shape, rps, compression, dtype)
    row_bytes = w * tiff._DTYPES[dtype][0]
    out, whole = byte_buffer(t * h * row_bytes, dev, past=3)  # an odd address, one byte before a word
    got, produced = tiff._decode_strips(data, flat_o, flat_n, t, spf, h, row_bytes, rps, compression, dev, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert_byte_guards(out, whole, "mc_tiff_decode")
    return got.cpu(), produced.cpu().tolist()


def check_movie(mc, dev, movie, strips, rps, order=None, fill=None, dtype=torch.uint8, **lay):
    """The strips through decode_tiff_raw (data on the CPU and on the GPU) and through the guarded decode, against
    the sequential reference and the movie they were made from."""
    t, h, w = movie.shape
    row_bytes = w * movie.dtype.itemsize
    want, produced = tr.decode_movie(strips, (h, w), rps, row_bytes)
    assert want == movie.tobytes()
    buf, offsets, nbytes = tr.lay_out(strips, order=order, fill=fill, **lay)
    data = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
    want_t = torch.from_numpy(movie.copy())
    for d in (data, data.to(dev)):
        got = mc.decode_tiff_raw(d, offsets, nbytes, (h, w), rps, dtype=dtype, device=dev)
        assert got.dtype == want_t.dtype and got.device == dev and got.is_contiguous() and got.shape == movie.shape
        assert torch.equal(got.cpu(), want_t)
    raw, got_produced = decode(dev, data, offsets, nbytes, (h, w), rps, dtype=dtype)
    assert got_produced == produced and bytes(raw.numpy()) == want


# ------------------------------------------------------------------ files libtiff wrote


@pytest.mark.parametrize("name", NAMES)
def test_committed_files(mc, dev, golden, tmp_path, name):
    path = tmp_path / (name + ".tif")
    path.write_bytes(golden["file_" + name].tobytes())
    pixels = golden["pixels_" + name]
    movie = mc.read_tiff(path)
    got = movie.decode(device=dev)
    assert got.device == dev and got.is_contiguous() and got.shape == pixels.shape
    if name == "u16":
        assert got.dtype == torch.int16
        assert torch.equal(got.cpu(), torch.from_numpy(pixels.astype(np.int16)))
    else:
        assert got.dtype == {np.dtype("uint8"): torch.uint8, np.dtype("float32"): torch.float32}[pixels.dtype]
        assert torch.equal(got.cpu(), torch.from_numpy(pixels.copy()))
    raw, produced = decode(dev, movie.data, movie.offsets, movie.nbytes, movie.shape, movie.rows_per_strip,
                           movie.compression, movie.dtype)
    assert bytes(raw.numpy()) == pixels.tobytes()


# ------------------------------------------------------------------ encoder-made movies against the reference


def poisson(seed, shape, mean=1.0):
    return np.random.default_rng(seed).poisson(mean, shape).astype(np.uint8)


def test_one_strip_per_frame(mc, dev):
    movie = poisson(1, (3, 70, 100))  # 7000 bytes per strip: no multiple of the wavefront's 64
    check_movie(mc, dev, movie, tr.encode_movie(movie, 70), 70)


def test_short_last_strip_and_odd_row_bytes(mc, dev):
    movie = poisson(2, (2, 37, 129))
    strips = tr.encode_movie(movie, 5)
    assert len(strips[0]) == 8 and 37 % 5 == 2
    check_movie(mc, dev, movie, strips, 5)


def test_clear_and_twelve_bit_codes_inside_a_strip(mc, dev):
    movie = np.random.default_rng(3).integers(0, 256, (1, 40, 512), dtype=np.uint8)
    strips = tr.encode_movie(movie, 40)
    trace = []
    tr.decode_strip(strips[0][0], 40 * 512, trace)
    assert len(trace) > 4100 and {w for _, w, _ in trace} == {9, 10, 11, 12}
    assert sum(c == tr.CLEAR for c, _, _ in trace) >= 3
    check_movie(mc, dev, movie, strips, 40)


def test_all_zero_every_code_kwkwk(mc, dev):
    movie = np.zeros((2, 64, 4096), dtype=np.uint8)
    one = tr.encode_strip(bytes(8 * 4096))
    trace = []
    tr.decode_strip(one, 8 * 4096, trace)
    data = [(c, n) for c, _, n in trace if c != tr.CLEAR]
    assert all(c == n for c, n in data[1:-1]) and len(data) > 250  # code k is a string of k bytes: up to 255
    check_movie(mc, dev, movie, [[one] * 8] * 2, 8)
    # 16-row strips: strings of more than 256 bytes (1 + 2 + .. + 361 > 65536), the copy loops six times
    two = tr.encode_strip(bytes(16 * 4096))
    trace = []
    tr.decode_strip(two, 16 * 4096, trace)
    assert sum(c != tr.CLEAR for c, _, _ in trace) > 360
    check_movie(mc, dev, movie[:1, :32], [[two] * 2], 16)


def test_long_strings_that_do_not_overlap(mc, dev):
    row = np.tile(np.array([3, 3, 3, 7, 7], dtype=np.uint8), 600)  # a two-valued pattern of period 5
    movie = np.stack([row.reshape(4, 750), np.roll(row, 2).reshape(4, 750)])
    strips = tr.encode_movie(movie, 4)
    trace = []
    tr.decode_strip(strips[0][0], 3000, trace)
    assert len(trace) < 200  # 3000 bytes in fewer than 200 codes: strings far longer than a wavefront
    check_movie(mc, dev, movie, strips, 4)


def test_int16(mc, dev):
    movie = (np.random.default_rng(4).poisson(40.0, (2, 33, 50)) - 45).astype(np.int16)
    assert movie.min() < 0
    check_movie(mc, dev, movie, tr.encode_movie(movie, 7), 7, dtype=torch.int16)


def test_strips_anywhere_in_data(mc, dev):
    movie = poisson(5, (3, 37, 129))
    strips = tr.encode_movie(movie, 5)
    rng = np.random.default_rng(6)
    order = rng.permutation(3 * 8).tolist()
    buf, offsets, _ = tr.lay_out(strips, order=order, fill=np.random.default_rng(7), gap=5)
    assert all(o % 2 == 1 for f in offsets for o in f) and sorted(sum(offsets, [])) != sum(offsets, [])
    check_movie(mc, dev, movie, strips, 5, order=order, fill=np.random.default_rng(7), gap=5)


@pytest.mark.parametrize("kw", [dict(leading_clear=False), dict(eoi=False), dict(leading_clear=False, eoi=False),
                                dict(defer_clear=300), dict(clear_at=37)], ids=str)
def test_encoder_options(mc, dev, kw):
    """streams without a leading Clear, without EOI, with a Clear deferred past a full table (nothing is added, codes
    stay at 12 bits) and with frequent Clears"""
    movie = np.random.default_rng(8).integers(0, 256, (1, 30, 400), dtype=np.uint8) if "defer_clear" in kw \
        else poisson(9, (2, 30, 100))
    strips = tr.encode_movie(movie, 30 if "defer_clear" in kw else 8, **kw)
    if "defer_clear" in kw:
        trace = []
        tr.decode_strip(strips[0][0], 12000, trace)
        assert sum(n == tr.TABLE for _, _, n in trace) > 300
    check_movie(mc, dev, movie, strips, 30 if "defer_clear" in kw else 8, gap=0, odd=False, lead=0)


def test_more_strips_than_resident_waves(mc, dev):
    """4000 one-row strips: a chip of 256 CUs holds at most 6 one-wave workgroups of 24 KB LDS per CU, 1536 in all, so
    the strips run in several scheduling rounds."""
    movie = poisson(10, (2, 2000, 64))
    check_movie(mc, dev, movie, tr.encode_movie(movie, 1), 1, gap=0, odd=False, lead=0)


def test_stored_strips(mc, dev):
    movie = poisson(11, (2, 37, 129), mean=3.0)
    strips = [[bytes(s) for s in tr.strips_of(f.tobytes(), 129, 5)] for f in movie]
    buf, offsets, nbytes = tr.lay_out(strips, order=list(reversed(range(16))))
    data = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
    got = mc.decode_tiff_raw(data, offsets, nbytes, (37, 129), 5, compression=1, device=dev)
    assert torch.equal(got.cpu(), torch.from_numpy(movie))
    raw, produced = decode(dev, data, offsets, nbytes, (37, 129), 5, compression=1)
    assert bytes(raw.numpy()) == movie.tobytes() and produced == [645] * 7 + [258] + [645] * 7 + [258]
    nbytes[1][3] -= 1  # a stored strip one byte short
    with pytest.raises(ValueError, match="frame 1, strip 3: .* 644 of the 645 bytes"):
        mc.decode_tiff_raw(data, offsets, nbytes, (37, 129), 5, compression=1, device=dev)


# ------------------------------------------------------------------ malformed input is refused, not run away with


@pytest.mark.parametrize("what", ["cut in half", "first code 300"])
def test_malformed_strips(mc, dev, what):
    """Both strips are among the cases of the sanitized host program (tests/test_tiff_host.py): the kernel's bounds
    make them ordinary inputs."""
    movie = poisson(12, (2, 37, 129))
    strips = tr.encode_movie(movie, 5)
    good = strips[1][2]
    if what == "cut in half":
        bad = good[:len(good) // 2]
    else:  # Clear, then code 300 with no previous code, then the rest of a good stream
        bits = tr._Bits()
        bits.put(256, 9)
        bits.put(300, 9)
        bad = bits.bytes() + good[2:]
    strips[1][2] = bad
    want, produced = tr.decode_movie(strips, (37, 129), 5, 129)
    assert produced[8 + 2] < 645 and sum(p != w for p, w in zip(produced, [645] * 7 + [258] + [645] * 7 + [258])) == 1
    # the bad strip last in the buffer: nothing readable follows it
    order = [i for i in range(16) if i != 10] + [10]
    buf, offsets, nbytes = tr.lay_out(strips, order=order, gap=0, odd=False)
    data = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
    assert offsets[1][2] + nbytes[1][2] == data.numel()
    for d in (data, data.to(dev)):
        with pytest.raises(ValueError, match="frame 1, strip 2: "):
            mc.decode_tiff_raw(d, offsets, nbytes, (37, 129), 5, device=dev)
    raw, got_produced = decode(dev, data, offsets, nbytes, (37, 129), 5)  # asserts the guards
    assert got_produced == produced
    got = raw.numpy().reshape(2, 37, 129)
    ok = np.ones((2, 37), dtype=bool)
    ok[1, 10:15] = False
    assert np.array_equal(got[ok], movie[ok])  # every other strip's rows
    n = produced[10]
    assert bytes(got[1, 10:15].reshape(-1)[:n]) == want[(37 + 10) * 129:(37 + 10) * 129 + n]  # and what it did give


def test_unsigned_16_bit_samples(mc, dev):
    movie = np.random.default_rng(13).poisson(300.0, (2, 9, 20)).astype(np.uint16)
    strips = tr.encode_movie(movie, 4)
    buf, offsets, nbytes = tr.lay_out(strips)
    data = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
    got = mc.decode_tiff_raw(data, offsets, nbytes, (9, 20), 4, dtype=torch.uint16, device=dev)
    assert got.dtype == torch.int16 and torch.equal(got.cpu(), torch.from_numpy(movie.astype(np.int16)))
    movie[1, 3, 7] = 32768
    buf, offsets, nbytes = tr.lay_out(tr.encode_movie(movie, 4))
    data = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
    with pytest.raises(ValueError, match="32768 or more"):
        mc.decode_tiff_raw(data, offsets, nbytes, (9, 20), 4, dtype=torch.uint16, device=dev)
    # the same bytes as a signed file are a movie
    got = mc.decode_tiff_raw(data, offsets, nbytes, (9, 20), 4, dtype=torch.int16, device=dev)
    assert int(got[1, 3, 7]) == -32768


# ------------------------------------------------------------------ a raw movie for every raw route


def test_downstream_use(mc, dev, golden, tmp_path):
    path = tmp_path / "movie.tif"
    path.write_bytes(golden["file_u8_strips"].tobytes())
    pixels = torch.from_numpy(golden["pixels_u8_strips"].copy())
    movie = mc.read_tiff(path).decode(device=dev)
    stats = mc.RawStatistics(tuple(movie.shape[1:]), device=dev).add(movie)
    assert stats.frames == 3
    assert torch.equal(stats.sum.cpu(), pixels.long().sum(0))
    assert torch.equal(stats.sumsq.cpu(), (pixels.long() ** 2).sum(0))
    gain = torch.ones(movie.shape[1:], dtype=torch.float32, device=dev)
    got = mc.motion_correct_raw(movie, gain, pixel_spacing=1.0)
    want = mc.motion_correct_raw(pixels.to(dev), gain, pixel_spacing=1.0)
    for a, b in zip(got if isinstance(got, (tuple, list)) else [got], want if isinstance(want, (tuple, list)) else [want]):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b)
