"""EER rendering on the GPU (render_eer_raw: mc_eer_render, csrc/eer_render.hip over csrc/eer.h) against the
sequential decoder and the np.add.at renderer of tests/eer_reference.py.  Event counts are integers: torch.equal
throughout."""

import numpy as np
import pytest
import torch

import eer_reference as er

pytestmark = pytest.mark.gpu

SHAPE = (48, 64)
DENSITIES = (0.0, 1.0, 0.5, 0.1, 0.02, 0.004, 0.3)


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


@pytest.fixture(scope="module")
def mixed():
    """The seven frames of mixed densities, laid into one buffer at odd offsets, out of order and with gaps."""
    rng = np.random.default_rng(7)
    n = SHAPE[0] * SHAPE[1]
    strips = [er.encode_frame(*er.random_frame(rng, n, d), n) for d in DENSITIES]
    buf, offsets, nbytes = er.lay_out(strips, order=[4, 1, 6, 0, 3, 5, 2])
    return strips, torch.frombuffer(bytearray(buf), dtype=torch.uint8), offsets, nbytes


def test_mixed_streams_meet_every_entry_offset(mc, mixed):
    """On the CPU: for these streams and the library's segment size, a segment begins at every offset 0 .. 10 of its
    first symbol, and the streams run from less than one segment to dozens."""
    from torch_motion_correction_amd import eer

    strips, _, offsets, nbytes = mixed
    seen = set()
    for s in strips:
        seen |= er.entry_offsets(s, SHAPE[0] * SHAPE[1], eer.SEGMENT_BYTES)
    assert seen == set(range(11))
    assert min(nbytes) == 22 and max(nbytes) == 4225
    assert all(o % 2 == 1 for o in offsets) and offsets != sorted(offsets)


@pytest.mark.parametrize("upsampling", [1, 2])
@pytest.mark.parametrize("group", [1, 2, 3, 7])
def test_mixed_densities(mc, dev, mixed, group, upsampling):
    strips, data, offsets, nbytes = mixed
    want, final_n, counts = er.render(strips, SHAPE, group, upsampling)
    assert list(final_n) == [SHAPE[0] * SHAPE[1]] * 7
    for d in (data, data.to(dev)):  # a CPU buffer and one that is already on the device
        got, ev = mc.render_eer_raw(d, offsets, nbytes, SHAPE, group, upsampling=upsampling,
                                    return_event_counts=True, device=dev)
        assert got.dtype == torch.uint8 and got.device == dev and got.is_contiguous()
        assert got.shape == (7 // group, upsampling * SHAPE[0], upsampling * SHAPE[1])
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (group, upsampling)
        assert ev.dtype == torch.int32 and torch.equal(ev.cpu(), torch.from_numpy(counts))


def test_no_byte_carry(mc, dev):
    n = 64
    strip = er.encode_frame(np.arange(n), np.arange(n) % 16, n)
    data = torch.frombuffer(bytearray(strip * 255), dtype=torch.uint8)
    offsets, nbytes = [i * len(strip) for i in range(255)], [len(strip)] * 255
    got = mc.render_eer_raw(data, offsets, nbytes, (8, 8), 255, device=dev)
    assert got.shape == (1, 8, 8) and torch.equal(got.cpu(), torch.full((1, 8, 8), 255, dtype=torch.uint8))
    # with half of the pixels hit, every neighbour of a 255 stays 0
    strip = er.encode_frame(np.arange(0, n, 2), np.zeros(n // 2, dtype=np.int64), n)
    data = torch.frombuffer(bytearray(strip * 255), dtype=torch.uint8)
    got = mc.render_eer_raw(data, [i * len(strip) for i in range(255)], [len(strip)] * 255, (8, 8), 255, device=dev)
    want = torch.zeros(64, dtype=torch.uint8)
    want[::2] = 255
    assert torch.equal(got.cpu().reshape(-1), want)


def test_remainder_and_counts(mc, dev):
    rng = np.random.default_rng(21)
    shape = (20, 36)
    n = shape[0] * shape[1]
    strips = [er.encode_frame(*er.random_frame(rng, n, 0.05 + 0.05 * f), n) for f in range(10)]
    buf, offsets, nbytes = er.lay_out(strips, order=range(10), gap=0, odd=False)
    data = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
    want, _, counts = er.render(strips, shape, 4)
    got, ev = mc.render_eer_raw(data, offsets, nbytes, shape, 4, return_event_counts=True, device=dev)
    assert got.shape == (2, 20, 36) and torch.equal(got.cpu(), torch.from_numpy(want))
    assert ev.shape == (10,) and torch.equal(ev.cpu(), torch.from_numpy(counts))  # the dropped frames' counts too
    assert mc.EerMovie(data, offsets, nbytes, shape, 7).render(4, upsampling=2, device=dev).shape == (2, 40, 72)


def test_malformed_streams(mc, dev, mixed):
    strips, _, _, _ = mixed
    n = SHAPE[0] * SHAPE[1]
    # a stream cut in half, and one written for a frame of 50 more pixels: its last run (69) ends at n + 50
    over = er.encode_frame([10, n - 20], [3, 12], n + 50)
    assert er.decode_frame(over, n) == ([10, n - 20], [3, 12], n + 50)
    cases = {"cut short": (strips[2][:len(strips[2]) // 2], 3), "overshoots": (over, 1)}
    for what, (bad, at) in cases.items():
        frames = list(strips[:4])
        frames[at] = bad
        assert er.decode_frame(bad, n)[2] != n
        # the bad strip last in the buffer: nothing readable follows it
        buf, offsets, nbytes = er.lay_out(frames, order=[0, 2, 3, 1] if at == 1 else [0, 1, 2, 3], gap=0, odd=False)
        data = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
        assert offsets[at] + nbytes[at] == data.numel()
        with pytest.raises(ValueError, match=f"frame {at}: .*{what}"):
            mc.render_eer_raw(data, offsets, nbytes, SHAPE, 1, device=dev)
        with pytest.raises(ValueError, match=f"frame {at}: "):
            mc.render_eer_raw(data.to(dev), offsets, nbytes, SHAPE, 2, upsampling=2, device=dev)


def test_downstream_use(mc, dev, mixed):
    strips, data, offsets, nbytes = mixed
    movie = mc.render_eer_raw(data, offsets, nbytes, SHAPE, 1, device=dev)
    want = torch.from_numpy(er.render(strips, SHAPE, 1)[0])
    stats = mc.RawStatistics(SHAPE, device=dev).add(movie)
    assert stats.frames == 7
    assert torch.equal(stats.sum.cpu(), want.long().sum(0)) and torch.equal(stats.sumsq.cpu(), (want.long() ** 2).sum(0))
    grouped = mc.group_frames_raw(movie, 3)
    assert grouped.dtype == torch.int16 and grouped.shape == movie.shape
    assert torch.equal(grouped.cpu(), mc.group_frames_raw(want, 3, device=dev).cpu())
    assert torch.equal(grouped[1].cpu().long(), want[:3].long().sum(0))
