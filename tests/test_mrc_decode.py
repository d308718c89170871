"""MRC decode on the GPU (decode_mrc_raw: mc_mrc_decode, csrc/mrc_decode.hip over csrc/mrc.h) against the numpy decoder
of tests/mrc_reference.py.  The decoder moves bytes: torch.equal throughout.  Every output lies inside a NaN-guarded
allocation (kernel_harness.byte_buffer) at an address that is aligned for its element and for nothing more, and
`data` ends at the payload's last byte, so a write outside the movie shows and a read outside the payload has nothing
behind it."""

import numpy as np
import pytest
import torch

import mrc_reference as mr
from kernel_harness import assert_byte_guards, byte_buffer

pytestmark = pytest.mark.gpu

# (mode, swap, unsigned_bytes): every kernel instantiation
KINDS = [(0, False, True), (0, False, False), (1, False, False), (1, True, False), (6, False, False),
         (6, True, False), (12, False, False), (12, True, False), (2, False, False), (2, True, False),
         (101, False, False)]
WIDTHS = (1, 15, 16, 17, 31, 33, 63, 64 + 1, 2 * 64 * 16 + 3)  # around one unit, one wavefront's and a workgroup's units
TORCH_OF = {np.dtype("u1"): torch.uint8, np.dtype("i2"): torch.int16, np.dtype("f2"): torch.float16,
            np.dtype("f4"): torch.float32}


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def pixels_for(mode, shape, seed, unsigned_bytes=False):
    rng = np.random.default_rng([seed, mode, *shape])
    if mode == 101:
        return rng.integers(0, 16, shape, dtype=np.uint8)
    if mode == 0:
        return rng.integers(0, 256, shape, dtype=np.uint8) if unsigned_bytes else \
            rng.integers(-128, 128, shape).astype(np.int8)
    if mode == 1:
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    if mode == 6:
        return rng.integers(0, 32768, shape).astype(np.uint16)
    if mode == 2:  # every bit pattern, NaNs included: the comparisons are of bits
        return rng.integers(0, 2**32, shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return rng.integers(0, 2**16, shape).astype(np.uint16).view(np.float16)


def guarded(shape, dtype, dev):
    """An output of `shape` and `dtype` inside a NaN-filled allocation, starting three elements past a 16-byte boundary
    -> (the view, the whole allocation as bytes)"""
    view, whole = byte_buffer(int(np.prod(shape)) * dtype.itemsize, dev, past=3 * dtype.itemsize)
    view = view.view(dtype).view(*shape)
    assert view.data_ptr() % dtype.itemsize == 0 and view.data_ptr() % 16 != 0
    return view, whole


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def case(mode, swap, ub, shape, offset, seed):
    """-> (data: `offset` bytes of 0xEE and the payload, nothing after it; the payload)"""
    px = pixels_for(mode, shape, seed, ub)
    payload = mr.pack_rows(px, mode, ">" if swap else "<", pad_nibble=15)
    return torch.frombuffer(bytearray(b"\xee" * offset + payload), dtype=torch.uint8), payload


@pytest.mark.parametrize("mode,swap,ub", KINDS)
def test_every_branch_of_a_row(mc, dev, mode, swap, ub):
    from torch_motion_correction_amd import mrc

    seed = 0
    for w in WIDTHS:
        for h in (1, 5):
            for t in (1, 3):
                for offset in (1024, 1024 + 1, 1024 + 7):
                    seed += 1
                    data, payload = case(mode, swap, ub, (t, h, w), offset, seed)
                    assert data.numel() == offset + t * h * mr.row_bytes(mode, w)
                    on_dev = data.to(dev)
                    for flip in (False, True):
                        want = torch.from_numpy(mr.decode(payload, (t, h, w), mode, swap, ub, flip))
                        out, whole = guarded((t, h, w), want.dtype, dev)
                        got = mrc._decode(on_dev, offset, t, h, w, mode, swap, ub, flip, dev, out=out)
                        torch.cuda.synchronize()
                        what = f"mode {mode} swap {swap} unsigned {ub} {(t, h, w)} offset {offset} flip {flip}"
                        assert got.data_ptr() == out.data_ptr()
                        assert_byte_guards(out, whole, what)
                        assert same_bits(got.cpu(), want), what


@pytest.mark.parametrize("mode,swap,ub", KINDS)
def test_public_route(mc, dev, tmp_path, mode, swap, ub):
    """decode_mrc_raw with the data on the CPU and on the GPU, a `data` that is a view at an odd address, and
    read_mrc(...).decode() of a file with an extended header of 7 bytes."""
    shape = (3, 5, 2 * 64 * 16 + 3)
    data, payload = case(mode, swap, ub, shape, 1031, 77)
    for flip in (False, True):
        want = torch.from_numpy(mr.decode(payload, shape, mode, swap, ub, flip))
        for d in (data, data.to(dev), data.to(dev)[1:]):
            got = mc.decode_mrc_raw(d, 1031 - (d.numel() != data.numel()), shape, mode, swap=swap, unsigned_bytes=ub,
                                    flip_rows=flip, device=dev)
            assert got.device == dev and got.is_contiguous() and same_bits(got.cpu(), want)
    px = pixels_for(mode, shape, 77, ub)
    path = tmp_path / "m.mrc"
    mr.write_mrc(path, px, mode, byte_order=">" if swap else "<", nsymbt=7, imod=0 if ub else None, pad_nibble=15)
    movie = mc.read_mrc(path)
    assert (movie.mode, movie.swap, movie.unsigned_bytes, movie.offset) == (mode, swap, ub, 1031)
    for flip in (False, True):
        want = torch.from_numpy(mr.decode(payload, shape, mode, swap, ub, flip))
        assert same_bits(movie.decode(device=dev, flip_rows=flip).cpu(), want)


@pytest.mark.parametrize("swap", [False, True])
def test_mode_6_refuses_32768(mc, dev, swap):
    px = np.random.default_rng(3).integers(0, 32768, (2, 9, 20)).astype(np.uint16)
    px[1, 3, 7] = 32767
    payload = mr.pack_rows(px, 6, ">" if swap else "<")
    data = torch.frombuffer(bytearray(payload), dtype=torch.uint8)
    got = mc.decode_mrc_raw(data, 0, (2, 9, 20), 6, swap=swap, device=dev)
    assert got.dtype == torch.int16 and torch.equal(got.cpu(), torch.from_numpy(px.astype(np.int16)))
    px[1, 3, 7] = 32768
    data = torch.frombuffer(bytearray(mr.pack_rows(px, 6, ">" if swap else "<")), dtype=torch.uint8)
    with pytest.raises(ValueError, match="32768 or more"):
        mc.decode_mrc_raw(data, 0, (2, 9, 20), 6, swap=swap, device=dev)
    # the same bytes as a signed file are a movie
    assert int(mc.decode_mrc_raw(data, 0, (2, 9, 20), 1, swap=swap, device=dev)[1, 3, 7]) == -32768


def test_gain_decodes_bit_exactly(mc, dev, tmp_path):
    gain = (4.0 ** (2 * np.random.default_rng(4).random((1, 67, 130)) - 1)).astype(np.float32)
    gain[0, 5, 5], gain[0, 6, 6], gain[0, 7, 7] = np.float32("inf"), -0.0, np.float32(1e-42)  # a denormal too
    path = tmp_path / "gain.mrc"
    for bo in "<>":
        mr.write_mrc(path, gain, 2, byte_order=bo, pixel_spacing=0.83)
        movie = mc.read_mrc(path)
        got = movie.decode(device=dev)
        assert got.dtype == torch.float32 and same_bits(got.cpu(), torch.from_numpy(gain))
        assert movie.pixel_spacing == pytest.approx(0.83, rel=1e-6)


@pytest.mark.parametrize("mode", [101, 0, 1])
def test_the_result_is_a_raw_movie(mc, dev, tmp_path, mode):
    shape = (4, 37, 129)
    rng = np.random.default_rng(5)
    if mode == 1:
        original = (rng.poisson(40.0, shape) - 45).astype(np.int16)
    else:
        original = np.minimum(rng.poisson(2.0, shape), 15).astype(np.uint8)
    path = tmp_path / "movie.mrc"
    mr.write_mrc(path, original, mode, imod=0 if mode == 0 else None)
    movie = mc.read_mrc(path).decode(device=dev)
    assert movie.dtype == torch.from_numpy(original).dtype and torch.equal(movie.cpu(), torch.from_numpy(original))
    a = mc.RawStatistics(shape[1:], device=dev).add(movie)
    b = mc.RawStatistics(shape[1:], device=dev).add(torch.from_numpy(original).to(dev))
    assert a.frames == b.frames == 4 and torch.equal(a.sum, b.sum) and torch.equal(a.sumsq, b.sumsq)
