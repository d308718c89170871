"""TIFF LZW encode on the GPU (encode_tiff_raw: mc_tiff_encode and mc_tiff_pack, csrc/tiff_encode.hip over
csrc/tiff_lzw_encode.h) against the reference encoder of tests/tiff_reference.py, byte for byte, and write_tiff's files
read back by read_tiff.  The input, the slots and the payload lie inside guarded, NaN-filled allocations
(kernel_harness.byte_buffer): a write outside a buffer, or into a slot beyond the bytes a strip produced, shows."""

import numpy as np
import pytest
import torch

import tiff_reference as tr
from kernel_harness import assert_byte_guards, byte_buffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def pattern(nbytes):
    """what an untouched stretch of a NaN-filled allocation holds, from a 4-byte boundary on"""
    return torch.full(((nbytes + 3) // 4,), float("nan"), dtype=torch.float32).view(torch.uint8)[:nbytes]


def encode(dev, movie, rps):
    """encode_tiff_raw's own steps with the input, the slots and the payload in guarded buffers -> (the payload's
    bytes, the per-strip sizes)."""
    from torch_motion_correction_amd import tiff

    t, h, w, rps, spf, row_bytes = tiff._check_encode_args(movie, rps, 5)
    raw = movie.contiguous().view(torch.uint8).reshape(-1)
    src, src_whole = byte_buffer(raw.numel(), dev, past=1)
    src.copy_(raw)
    slot = tiff._slot_bytes(rps * row_bytes)
    slots, slots_whole = byte_buffer(t * spf * slot, dev)
    assert slots.data_ptr() % 16 == 0
    got_slots, got_slot, produced = tiff._encode_strips(src, t, spf, h, row_bytes, rps, dev, slots=slots)
    torch.cuda.synchronize()
    assert got_slots.data_ptr() == slots.data_ptr() and got_slot == slot
    sizes = produced.cpu().tolist()
    assert_byte_guards(slots, slots_whole, "mc_tiff_encode")
    assert bytes(src.cpu().numpy()) == bytes(raw.numpy())
    assert_byte_guards(src, src_whole, "mc_tiff_encode (input)")
    # every slot byte past what its strip produced is untouched (slots start on 16-byte boundaries of the pattern)
    image, fresh = slots.cpu().view(t * spf, slot), pattern(slot)
    assert all(0 < n <= slot for n in sizes)
    keep = torch.arange(slot)[None, :] >= torch.tensor(sizes)[:, None]
    assert torch.equal(image[keep], fresh.expand(t * spf, slot)[keep]), "a strip wrote beyond the bytes it produced"
    total = sum(sizes)
    payload, pay_whole = byte_buffer(total, dev, past=1)
    got = tiff._pack_strips(slots, slot, produced, total, dev, payload=payload)
    torch.cuda.synchronize()
    assert got.data_ptr() == payload.data_ptr()
    assert_byte_guards(payload, pay_whole, "mc_tiff_pack")
    return bytes(payload.cpu().numpy()), sizes


def check_movie(mc, dev, movie, rps=None):
    """`movie` (a CPU tensor) through the guarded encode and through encode_tiff_raw: every strip's bytes equal the
    reference encoder's, and the decoders -- the device's and the reference's -- give the movie back."""
    from torch_motion_correction_amd import tiff

    t, h, w, want_rps, spf, row_bytes = tiff._check_encode_args(movie, rps, 5)
    frames = movie.contiguous().numpy().reshape(t, h, w)
    want = [s for f in tr.encode_movie(frames, want_rps) for s in f]
    assert len(want) == t * spf
    payload, sizes = encode(dev, movie, rps)
    assert sizes == [len(s) for s in want]
    assert payload == b"".join(want)
    for m in (movie, movie.to(dev)):
        got = mc.encode_tiff_raw(m, rows_per_strip=rps, device=dev)
        assert isinstance(got, mc.TiffMovie) and got.data.device == dev and got.data.dtype == torch.uint8
        assert got.shape == (h, w) and got.rows_per_strip == want_rps and got.compression == 5
        assert got.dtype == movie.dtype and bytes(got.data.cpu().numpy()) == payload
        assert [n for f in got.nbytes for n in f] == sizes and len(got.nbytes) == t
        flat = [o for f in got.offsets for o in f]
        assert flat == [sum(sizes[:k]) for k in range(len(sizes))]
        back = got.decode()
        assert back.dtype == movie.dtype and torch.equal(back.cpu(), movie.reshape(t, h, w))
    rows = [s for f in frames for s in tr.strips_of(f.tobytes(), row_bytes, want_rps)]
    for k in sorted({0, min(1, len(want) - 1), len(want) // 2, len(want) - 1}):
        at = sum(sizes[:k])
        assert tr.decode_strip(payload[at:at + sizes[k]], len(rows[k])) == (rows[k], "full")
    return want


def poisson(seed, shape, mean=1.0):
    return torch.from_numpy(np.random.default_rng(seed).poisson(mean, shape).astype(np.uint8))


# ------------------------------------------------------------------ every strip equals the reference encoder's


def test_short_last_strip_and_odd_row_bytes(mc, dev):
    check_movie(mc, dev, poisson(1, (3, 12, 10)), rps=5)


def test_one_byte(mc, dev):
    want = check_movie(mc, dev, torch.tensor([[[200]]], dtype=torch.uint8))
    assert want == [tr.encode_strip(bytes([200]))] and len(want[0]) == 4


def test_one_strip_per_frame(mc, dev):
    movie = poisson(2, (3, 70, 100))  # 7000 bytes per strip: no multiple of the wavefront's 64
    assert len(check_movie(mc, dev, movie)) == 3


def test_int16(mc, dev):
    movie = torch.from_numpy((np.random.default_rng(3).poisson(40.0, (2, 7, 33)) - 45).astype(np.int16))
    assert int(movie.min()) < 0
    check_movie(mc, dev, movie, rps=3)


def test_float32_gain(mc, dev):
    gain = torch.from_numpy(np.random.default_rng(4).normal(1.0, 0.05, (11, 9)).astype(np.float32))
    check_movie(mc, dev, gain, rps=4)
    got = mc.encode_tiff_raw(gain, device=dev)
    assert len(got.offsets) == 1 and got.rows_per_strip == 11 and torch.equal(got.decode()[0].cpu(), gain)


def test_all_zero_longest_strings(mc, dev):
    want = check_movie(mc, dev, torch.zeros(2, 64, 512, dtype=torch.uint8))
    trace = []
    tr.decode_strip(want[0], 64 * 512, trace)
    assert len(want) == 2 and len(trace) < 300  # 32 KB in one strip: strings of up to 255 bytes


def test_poisson_counts(mc, dev):
    check_movie(mc, dev, poisson(5, (2, 48, 256)))


@pytest.mark.parametrize("h,clears", [(32, 3), (64, 5)])
def test_clear_and_all_widths_inside_a_strip(mc, dev, h, clears):
    """random bytes in one strip: Clear at 4093 reached, widths 9 - 12, the table refilled once (8 KB) and three
    times (16 KB)"""
    movie = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (1, h, 256), dtype=np.uint8))
    want = check_movie(mc, dev, movie, rps=h)
    trace = []
    tr.decode_strip(want[0], h * 256, trace)
    assert {w for _, w, _ in trace} == {9, 10, 11, 12}
    assert sum(c == tr.CLEAR for c, _, _ in trace) >= clears - 1 >= 2


def test_more_strips_than_resident_waves(mc, dev):
    """8192 one-row strips: a chip of 256 CUs holds 5 one-wave workgroups of 32 KB LDS per CU, 1280 in all, so the
    strips run in several scheduling rounds"""
    assert len(check_movie(mc, dev, poisson(7, (8, 1024, 16)), rps=1)) == 8192


def test_non_contiguous_view(mc, dev):
    base = poisson(8, (2, 30, 44))
    view = base.transpose(1, 2)[:, ::2]
    assert not view.is_contiguous()
    check_movie(mc, dev, view, rps=4)
    got = mc.encode_tiff_raw(view.to(dev), rows_per_strip=4)
    assert torch.equal(got.decode().cpu(), view)


def test_stored_strips_round_trip(mc, dev):
    movie = poisson(9, (2, 37, 129), mean=3.0)
    got = mc.encode_tiff_raw(movie.to(dev), rows_per_strip=5, compression=1)
    assert got.compression == 1 and got.data.device == dev and bytes(got.data.cpu().numpy()) == movie.numpy().tobytes()
    assert got.nbytes == [[645] * 7 + [258]] * 2 and got.offsets[1][0] == 37 * 129
    assert torch.equal(got.decode().cpu(), movie)
    assert torch.equal(mc.encode_tiff_raw(movie, compression=1).decode(device=dev).cpu(), movie)


# ------------------------------------------------------------------ files


@pytest.mark.parametrize("bigtiff", [None, True])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.float32])
def test_files_round_trip(mc, dev, tmp_path, bigtiff, dtype):
    movie = (poisson(10, (3, 37, 129), mean=2.0).to(torch.float32) - 1).to(dtype) if dtype != torch.uint8 \
        else poisson(10, (3, 37, 129))
    path, again = tmp_path / "movie.tif", tmp_path / "again.tif"
    mc.write_tiff(path, movie.to(dev), rows_per_strip=5, bigtiff=bigtiff)
    raw = path.read_bytes()
    assert raw[:4] == (b"II+\x00" if bigtiff else b"II*\x00")
    got = mc.read_tiff(path)
    assert got.shape == (37, 129) and got.rows_per_strip == 5 and got.compression == 5 and got.dtype == dtype
    assert len(got.offsets) == 3 and len(got.offsets[0]) == 8
    assert torch.equal(got.decode(device=dev).cpu(), movie)
    # the strips in the file are the reference encoder's, in frame order, from the header on
    want = b"".join(s for f in tr.encode_movie(movie.numpy(), 5) for s in f)
    first = 16 if bigtiff else 8
    assert got.offsets[0][0] == first and raw[first:first + len(want)] == want
    # a TiffMovie gives the same file
    mc.write_tiff(again, mc.encode_tiff_raw(movie, rows_per_strip=5, device=dev), bigtiff=bigtiff)
    assert again.read_bytes() == raw


# ------------------------------------------------------------------ a raw movie for every raw route, after the file


def test_downstream_use(mc, dev, tmp_path):
    movie = poisson(11, (6, 64, 96)).to(dev)
    grouped = mc.group_frames_raw(movie, 3)
    path = tmp_path / "grouped.tif"
    mc.write_tiff(path, grouped)
    back = mc.read_tiff(path).decode(device=dev)
    assert back.dtype == torch.int16 and torch.equal(back, grouped)
    a = mc.RawStatistics((64, 96), device=dev).add(back)
    b = mc.RawStatistics((64, 96), device=dev).add(grouped)
    assert a.frames == b.frames == 6 and torch.equal(a.sum, b.sum) and torch.equal(a.sumsq, b.sumsq)
    gain = torch.ones((64, 96), dtype=torch.float32, device=dev)
    got = mc.motion_correct_raw(back, gain, pixel_spacing=1.0)
    want = mc.motion_correct_raw(grouped, gain, pixel_spacing=1.0)
    for x, y in zip(got if isinstance(got, (tuple, list)) else [got], want if isinstance(want, (tuple, list)) else [want]):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y)
