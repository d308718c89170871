"""Gain-reference and defect-map estimation from raw u8 / i16 movies on the GPU: the per-pixel sums of
mc_raw_pixel_sums (through RawStatistics.add) and the finalisation against tests/calibration_reference.py.  Every
comparison with the restatement is torch.equal: the sums are integers, and the gain is one correctly rounded float64
division cast to fp32 on both sides."""

import numpy as np
import pytest
import torch

import calibration_reference as cr

pytestmark = pytest.mark.gpu

FRAME_BLOCK = 32768  # frames per launch of mc_raw_pixel_sums (csrc/raw_accumulate.hip)


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def random_movie(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        return torch.from_numpy(rng.integers(0, 256, size=shape, dtype=np.uint8))
    return torch.from_numpy(rng.integers(-32768, 32768, size=shape, dtype=np.int16))


def assert_sums(stats, movies, frames):
    s = sum(cr.pixel_sums(m.numpy())[0] for m in movies)
    q = sum(cr.pixel_sums(m.numpy())[1] for m in movies)
    assert stats.frames == frames
    assert stats.sum.dtype == torch.int64 and stats.sumsq.dtype == torch.int64 and stats.sum.is_cuda
    assert tuple(stats.sum.shape) == tuple(stats.sumsq.shape) == stats.shape
    assert torch.equal(stats.sum.cpu(), torch.from_numpy(s)), "sum"
    assert torch.equal(stats.sumsq.cpu(), torch.from_numpy(q)), "sumsq"


# ------------------------------------------------------------------ 1. the sums, at the shapes where they can go wrong

SHAPES = [(3, 5, 16),      # one u8 piece per row (two i16 pieces)
          (7, 33, 927),    # odd width: unaligned row starts and a tail; more than one workgroup
          (2, 64, 4096),   # whole aligned pieces, many workgroups
          (5, 3, 8),       # one i16 piece per row (half a u8 piece)
          (1, 1, 1),
          (9, 6, 48),      # one full batch of 8 loads in flight and one frame more
          (3, 7, 959)]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
@pytest.mark.parametrize("shape", SHAPES)
def test_pixel_sums_equal_the_integer_reference(mc, dev, shape, dtype):
    movie = random_movie(shape, dtype, seed=sum(shape))
    stats = mc.RawStatistics(shape[1:], device=dev)
    assert stats.add(movie) is stats  # from the CPU: staged
    assert_sums(stats, [movie], shape[0])
    assert stats.dtype == dtype and stats.device == dev
    again = mc.RawStatistics(shape[1:]).add(movie.to(dev))  # on the device already
    assert torch.equal(again.sum, stats.sum) and torch.equal(again.sumsq, stats.sumsq)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_a_single_frame_and_a_misaligned_movie(mc, dev, dtype):
    """(h, w) input is one frame; a contiguous movie that starts one element past a 16-byte address takes the
    element path at a width of whole pieces."""
    frame = random_movie((12, 64), dtype, seed=3)
    assert_sums(mc.RawStatistics((12, 64)).add(frame.to(dev)), [frame[None]], 1)
    flat = random_movie((3 * 4 * 64 + 1,), dtype, seed=4).to(dev)
    movie = flat[1:].view(3, 4, 64)
    assert movie.is_contiguous() and movie.data_ptr() % 16 != 0
    assert_sums(mc.RawStatistics((4, 64)).add(movie), [movie.cpu()], 3)


# ------------------------------------------------------------------ 2. overflow edges


@pytest.mark.parametrize("shape,dtype,value", [
    ((512, 4, 64), torch.uint8, 255),
    ((512, 4, 64), torch.int16, -32768),
    ((512, 4, 64), torch.int16, 32767),
    # a whole FRAME_BLOCK at the extreme value and a second launch: the u32 sum of squares reaches 255^2 * 2^15 >
    # 2^31, the i32 sum -2^30, the u64 sum of squares 2^45
    ((2 * FRAME_BLOCK + 7, 1, 16), torch.uint8, 255),
    ((2 * FRAME_BLOCK + 7, 1, 8), torch.int16, -32768)])
def test_extreme_values_do_not_overflow(mc, dev, shape, dtype, value):
    t, h, w = shape
    movie = torch.full(shape, value, dtype=dtype, device=dev)
    stats = mc.RawStatistics((h, w)).add(movie)
    assert stats.frames == t
    assert torch.equal(stats.sum.cpu(), torch.full((h, w), t * value, dtype=torch.int64))
    assert torch.equal(stats.sumsq.cpu(), torch.full((h, w), t * value * value, dtype=torch.int64))


def test_random_frames_over_several_frame_blocks(mc, dev):
    movie = random_movie((1100, 2, 48), torch.uint8, seed=9)
    assert_sums(mc.RawStatistics((2, 48)).add(movie.to(dev)), [movie], 1100)
    long_movie = random_movie((2 * FRAME_BLOCK + 7, 1, 16), torch.uint8, seed=10)
    assert_sums(mc.RawStatistics((1, 16)).add(long_movie.to(dev)), [long_movie], 2 * FRAME_BLOCK + 7)


# ------------------------------------------------------------------ 3. accumulation


@pytest.mark.parametrize("shape,dtype", [((7, 33, 927), torch.uint8), ((7, 16, 64), torch.int16)])
def test_add_twice_and_merge_equal_the_concatenation(mc, dev, shape, dtype):
    movie = random_movie(shape, dtype, seed=21).to(dev)
    whole = mc.RawStatistics(shape[1:]).add(movie)
    twice = mc.RawStatistics(shape[1:]).add(movie[:3]).add(movie[3:])
    assert twice.frames == 7 and torch.equal(twice.sum, whole.sum) and torch.equal(twice.sumsq, whole.sumsq)
    a, b = mc.RawStatistics(shape[1:]).add(movie[:3]), mc.RawStatistics(shape[1:]).add(movie[3:])
    merged = a.merge(b)
    assert merged is a and a.frames == 7 and b.frames == 4
    assert torch.equal(a.sum, whole.sum) and torch.equal(a.sumsq, whole.sumsq)
    assert_sums(whole, [movie.cpu()], 7)
    with pytest.raises(ValueError, match="cannot be mixed"):
        whole.add(movie.to(torch.int16 if dtype == torch.uint8 else torch.uint8))
    assert whole.frames == 7


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_a_non_contiguous_view_equals_its_copy(mc, dev, dtype):
    movie = random_movie((4, 20, 96), dtype, seed=2).to(dev)
    view = movie[:, ::2, :]
    assert not view.is_contiguous()
    a, b = mc.RawStatistics((10, 96)).add(view), mc.RawStatistics((10, 96)).add(view.contiguous())
    assert torch.equal(a.sum, b.sum) and torch.equal(a.sumsq, b.sumsq)
    assert_sums(a, [view.cpu().contiguous()], 4)


# ------------------------------------------------------------------ 4. the defect map and the gain

DEAD, HOT, STUCK = [(0, 0), (40, 17), (95, 159)], [(3, 150), (50, 80), (77, 1)], [(10, 10), (60, 120)]


def planted_session():
    """(64, 96, 160) u8 counts: Poisson(20 g_true) with g_true in [0.8, 1.2], clipped to 255; three dead pixels, three
    at 8 x the mean and two stuck at 37.

    Margins of this data in the restatement, computed on the CPU before this test was committed (n M = 1282.7): the
    unplanted pixel sums lie in [927, 1657], that is 0.723 .. 1.292 of n M -- the nearest one to a threshold is 3.6 x
    the dead threshold (0.2) and a factor 3.9 below the hot one (5.0), so none is within 10 % of either; the hot
    pixels' sums are 7.97 .. 8.09 x n M, 59 % above the threshold; the stuck pixels (37 n = 1.85 x n M) are flagged by
    the stuck rule alone, and no unplanted pixel is near zero variance (the smallest n sumsq - sum^2 is 34 415)."""
    rng = np.random.default_rng(0)
    g_true = rng.uniform(0.8, 1.2, size=(96, 160))
    movie = np.minimum(rng.poisson(20.0 * g_true, size=(64, 96, 160)), 255).astype(np.uint8)
    for y, x in DEAD:
        movie[:, y, x] = 0
    for y, x in HOT:
        movie[:, y, x] = np.minimum(rng.poisson(160.0, size=64), 255)
    for y, x in STUCK:
        movie[:, y, x] = 37
    planted = np.zeros((96, 160), dtype=bool)
    for y, x in DEAD + HOT + STUCK:
        planted[y, x] = True
    return torch.from_numpy(movie), planted


def test_defect_map_and_gain_equal_the_restatement(mc, dev):
    movie, planted = planted_session()
    n = movie.shape[0]
    stats = mc.RawStatistics((96, 160)).add(movie[:40].to(dev)).add(movie[40:].to(dev))
    s, q = cr.pixel_sums(movie.numpy())
    assert_sums(stats, [movie], n)
    want_map = cr.defect_map(s, q, n)
    want_gain = cr.gain_reference(s, want_map)
    assert np.array_equal(want_map, planted)  # the restatement finds exactly the planted set
    dmap = mc.estimate_defect_map(stats)
    assert dmap.dtype == torch.bool and dmap.is_cuda and torch.equal(dmap.cpu(), torch.from_numpy(planted))
    gain, dmap2 = mc.estimate_gain_reference(stats, return_defect_map=True)
    assert gain.dtype == torch.float32 and gain.is_cuda and torch.equal(dmap2, dmap)
    assert torch.equal(gain.cpu(), torch.from_numpy(want_gain))
    assert not gain[dmap].any() and bool((gain[~dmap] > 0).all())
    # straight from the movies, and with the caller's own map
    assert torch.equal(mc.estimate_gain_reference([movie[:40].to(dev), movie[40:]]), gain)
    own = torch.zeros(96, 160, dtype=torch.bool)
    own[5, 5] = own[0, 0] = own[40, 17] = own[95, 159] = True  # every never-counting pixel has to be in it
    assert torch.equal(mc.estimate_gain_reference(stats, defect_map=own).cpu(),
                       torch.from_numpy(cr.gain_reference(s, own.numpy())))
    # the corrected mean image is flat over the good pixels: fp32 roundings of the gain and of one product, <= 0.5 ulp
    # each, give <= 1.2e-7 relative (sum_p < 2^24 is exact in fp32, the division by n = 64 too)
    good = ~dmap
    flat = (gain * stats.sum.float() / n)[good]
    level = float(int(s[~planted].sum())) / (int((~planted).sum()) * n)
    assert torch.allclose(flat, torch.full_like(flat, level), rtol=1e-6, atol=0.0)


# ------------------------------------------------------------------ 5. the estimated gain feeds the raw flow


def drift_movie(seed, dy, dx, sens, h=512, w=512, pad=64):
    """u8 counts of one texture at integer drift offsets + noise (the raw tests' drift stacks), seen through a
    detector of per-pixel sensitivity `sens`: the planted multiplicative fixed pattern, gain_true = 1 / sens."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(h + 2 * pad, w + 2 * pad, generator=g) * 40 + 60
    frames = [base[pad - y: pad - y + h, pad - x: pad - x + w] + 6 * torch.randn(h, w, generator=g)
              for y, x in zip(dy, dx)]
    return (torch.stack(frames) * sens).round().clamp(0, 255).to(torch.uint8)


def drift_session():
    t = 8
    g = torch.Generator().manual_seed(77)
    sens = 1.0 + 0.2 * (2 * torch.rand(512, 512, generator=g) - 1)
    movies, drifts = [], []
    for i, amp in enumerate((5, 3, 7, 4)):
        dy = torch.round(torch.linspace(-amp, amp + 2, t)).long().tolist()
        dx = torch.round(torch.linspace(amp - 1, -amp, t)).long().tolist()
        movies.append(drift_movie(100 + i, dy, dx, sens))
        drifts.append((dy, dx))
    return movies, drifts, (1.0 / sens)


def test_estimated_gain_gives_the_shifts_of_the_true_gain(mc, dev):
    movies, drifts, gain_true = drift_session()
    stats = mc.RawStatistics((512, 512))
    for m in movies:
        stats.add(m.to(dev))
    est = mc.estimate_gain_reference(stats)
    assert stats.frames == 32 and bool((est > 0).all())
    (dy, dx), t = drifts[0], 8
    field_est = mc.motion_correct_raw(movies[0].to(dev), est, 1.0)[0]
    field_true = mc.motion_correct_raw(movies[0].to(dev), gain_true.to(dev), 1.0)[0]
    expect = torch.tensor([[dy[f] - dy[t // 2], dx[f] - dx[t // 2]] for f in range(t)], dtype=torch.float32)
    assert torch.equal(field_true[:, :, 0, 0].T.cpu(), expect)
    assert torch.equal(field_est, field_true)


# ------------------------------------------------------------------ 6. nothing frame-sized beyond the accumulators


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_add_allocates_the_accumulators_and_nothing_else(mc, dev, dtype):
    t, h, w = 16, 1024, 1024
    movie = random_movie((t, h, w), dtype, seed=1).to(dev)
    stats = mc.RawStatistics((h, w))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    stats.add(movie)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"{dtype}: peak {peak / 2**20:.2f} MiB above the inputs; the accumulators are {16 * h * w / 2**20:.0f} MiB")
    assert peak < 16 * h * w + 2**20, peak  # sum + sumsq, 16 B per pixel: no fp32 or int64 copy of a frame
    stats.add(movie)  # and a second add stays below that peak: the accumulators are there already
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base == peak
    assert stats.frames == 2 * t
