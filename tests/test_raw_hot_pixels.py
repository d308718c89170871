"""The fused raw path (motion_correct_raw, RawMoviePipeline) with the example's hot-pixel step
(examples/ttMotion.py:127-172): results equal condition_movie(..., hot_pixel_threshold) followed by the fp32
path, without a conditioned fp32 movie."""

import numpy as np
import pytest
import torch

from torch_motion_correction_amd import engine
from torch_motion_correction_amd._lib import McorrUnsupported

pytestmark = pytest.mark.gpu

THR = 10.0


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _raw_drift_movie(t, h, w, dtype, seed, amp, pad=64):
    """raw detector-like counts of one texture at integer drift offsets + noise, and a gain reference"""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(h + 2 * pad, w + 2 * pad, generator=g) * 40 + 10
    dy = torch.round(torch.linspace(-amp, amp + 2, t)).long().tolist()
    dx = torch.round(torch.linspace(amp - 1, -amp, t)).long().tolist()
    raw = torch.empty((t, h, w), dtype=dtype)
    for f in range(t):
        v = base[pad - dy[f]: pad - dy[f] + h, pad - dx[f]: pad - dx[f] + w] + 6 * torch.randn(h, w, generator=g)
        if dtype == torch.int16:
            raw[f] = (v * 8 - 100).round().clamp(-32768, 32767).to(dtype)
        else:
            raw[f] = v.round().clamp(0, 255).to(dtype)
    gain = (1.0 + 0.1 * torch.randn(h, w, generator=g)).clamp(0.5, 1.5)
    return raw, gain, dy, dx


def _hot_pixel_reference(x, thr):
    """numpy restatement of the example's detection (examples/ttMotion.py:145-153) and of this package's
    deterministic replacement; x (t,h,w) float64 = raw * gain.  Returns the replaced frames and the counts."""
    out = x.copy()
    counts = []
    t, h, w = x.shape
    for f in range(t):
        fr = x[f]
        m, sd = fr.mean(), fr.std()
        hot = (fr > m + thr * sd) | (fr < m - thr * sd)
        counts.append(int(hot.sum()))
        for y, xx in zip(*np.where(hot)):
            vals = [fr[yy, xc] for yy in range(max(0, y - 1), min(h - 1, y + 1) + 1)
                    for xc in range(max(0, xx - 1), min(w - 1, xx + 1) + 1)
                    if (yy != y or xc != xx) and not hot[yy, xc]]
            out[f, y, xx] = np.mean(vals) if vals else m
    return out, counts


def _add_hot_pixels(raw, gain, seed, per_frame=6):
    """hot pixels at the four corners, on the first / last rows and columns, inside, as adjacent pairs (in the
    centre, where the estimator's mask is 1) and, for int16, low outliers; plus a few random ones per frame"""
    t, h, w = raw.shape
    g = torch.Generator().manual_seed(seed)
    hi = 255 if raw.dtype == torch.uint8 else 30000
    fixed = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 3), (h - 1, w // 2 + 5), (h // 3, 0),
             (h // 2 + 3, w - 1), (h // 2, w // 2), (h // 2, w // 2 + 1), (h // 2 + 17, w // 2 - 40),
             (h // 2 + 18, w // 2 - 40), (1, 1), (h - 2, w - 2)]
    for y, x in fixed:
        raw[:, y, x] = hi
        gain[y, x] = 1.0
    if raw.dtype == torch.int16:
        for y, x in [(h // 2 - 9, w // 2 + 21), (0, w // 2), (h - 1, 7), (h // 2 - 9, w // 2 + 22)]:
            raw[:, y, x] = -30000
            gain[y, x] = 1.0
    for f in range(t):
        ys = torch.randint(0, h, (per_frame,), generator=g)
        xs = torch.randint(0, w, (per_frame,), generator=g)
        raw[f, ys, xs] = hi
        gain[ys, xs] = 1.0
    return raw, gain


def _conditioned_route(mc, rd, gd, mean_zero=True, thr=THR):
    img, counts = mc.condition_movie(rd, gd, mean_zero, hot_pixel_threshold=thr, return_hot_counts=True)
    field = mc.estimate_global_motion(img, 1.0)
    total, frames = mc.motion_correct_sum(img, field, 1.0, return_frames=True)
    return field, total, frames, counts


@pytest.mark.parametrize("shape,dtype", [((6, 512, 4096), torch.uint8), ((6, 512, 4096), torch.int16),
                                         ((5, 512, 1024), torch.uint8), ((3, 4092, 5760), torch.uint8),
                                         ((3, 4092, 5760), torch.int16)])
def test_fused_hot_pixels_equal_conditioning_then_the_fp32_path(mc, dev, shape, dtype):
    """every fused engine (wave-per-row K1 at 4096 columns, the workgroup engine, the mixed-radix rows of the
    K3 format): shifts exactly, frames and sum to 1e-5, counts as the numpy restatement; with and without
    mean-zero and gain"""
    t, h, w = shape
    raw, gain, dy, dx = _raw_drift_movie(t, h, w, dtype, 41, 4)
    raw, gain = _add_hot_pixels(raw, gain, 7)
    rd = raw.to(dev)
    x = raw.numpy().astype(np.float64) * gain.numpy().astype(np.float64)
    _, ref_counts = _hot_pixel_reference(x, THR)
    assert min(ref_counts) >= 14
    for gd, mean_zero in ((gain.to(dev), True), (gain.to(dev), False), (None, True)):
        field, total, frames, counts = mc.motion_correct_raw(rd, gd, 1.0, mean_zero=mean_zero, return_frames=True,
                                                             hot_pixel_threshold=THR, return_hot_counts=True)
        fa, sa, fra, ca = _conditioned_route(mc, rd, gd, mean_zero)
        assert torch.equal(field, fa), (gd is None, mean_zero)
        assert rel_err(frames, fra) <= 1e-5 and rel_err(total, sa) <= 1e-5, (rel_err(frames, fra), rel_err(total, sa))
        assert torch.equal(counts, ca)
        if gd is not None:
            assert counts.cpu().tolist() == ref_counts
        # the fused route really was taken: the engine calls raise instead of falling back
        rm = engine.RawMovie(rd, gd, mean_zero=mean_zero, hot_pixel_threshold=THR)
        assert rm.n_hot == int(counts.sum())
        sh = engine.global_shifts_raw(rm, t // 2, 1.0, 500.0, (300, 10))
        assert torch.equal(field[:, :, 0, 0].T, sh)
    expect = torch.tensor([[dy[f] - dy[t // 2], dx[f] - dx[t // 2]] for f in range(t)], dtype=torch.float32)
    assert torch.equal(field[:, :, 0, 0].T.cpu(), expect)


def test_fixed_pattern_hot_pixels_bias_the_plain_path_and_removing_them_fixes_it(mc, dev):
    t, h, w = 6, 512, 4096
    raw, gain, dy, dx = _raw_drift_movie(t, h, w, torch.int16, 5, 5)
    g = torch.Generator().manual_seed(3)
    ys = torch.randint(h // 2 - 80, h // 2 + 80, (48,), generator=g)
    xs = torch.randint(w // 2 - 80, w // 2 + 80, (48,), generator=g)
    raw[:, ys, xs] = 32000  # the same detector positions in every frame
    rd, gd = raw.to(dev), gain.to(dev)
    x = raw.numpy().astype(np.float64) * gain.numpy().astype(np.float64)
    _, counts = _hot_pixel_reference(x, THR)
    assert min(counts) == len(set(zip(ys.tolist(), xs.tolist())))  # every one of them is above 10 sigma
    expect = torch.tensor([[dy[f] - dy[t // 2], dx[f] - dx[t // 2]] for f in range(t)], dtype=torch.float32)
    plain, _ = mc.motion_correct_raw(rd, gd, 1.0)
    assert not torch.equal(plain[:, :, 0, 0].T.cpu(), expect)  # the zero-lag peak of the fixed pattern wins
    fixed, _ = mc.motion_correct_raw(rd, gd, 1.0, hot_pixel_threshold=THR)
    assert torch.equal(fixed[:, :, 0, 0].T.cpu(), expect)


def test_headline_size_without_an_fp32_movie(mc, dev):
    """40 x 4096^2 u8 with a few hundred hot pixels per frame: the known drift, and no fp32 movie (2.7 GB) --
    the peak memory stays within 256 MB of the call without the threshold"""
    t, h, w = 40, 4096, 4096
    raw, gain, dy, dx = _raw_drift_movie(t, h, w, torch.uint8, 17, 6)
    g = torch.Generator().manual_seed(9)
    for f in range(t):
        ys = torch.randint(0, h, (300,), generator=g)
        xs = torch.randint(0, w, (300,), generator=g)
        raw[f, ys, xs] = 255
        gain[ys, xs] = 1.0
    rd, gd = raw.to(dev), gain.to(dev)
    del raw
    expect = torch.tensor([[dy[f] - dy[t // 2], dx[f] - dx[t // 2]] for f in range(t)], dtype=torch.float32)
    peaks = []
    for thr in (None, THR):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        field, total, counts = mc.motion_correct_raw(rd, gd, 1.0, hot_pixel_threshold=thr, return_hot_counts=True)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(dev))
        assert torch.equal(field[:, :, 0, 0].T.cpu(), expect), thr
        del field, total
    assert int(counts.min()) >= 200
    assert peaks[1] - peaks[0] <= 256 << 20, peaks


def test_list_overflow_takes_the_conditioned_route(mc, dev):
    t, h, w = 3, 512, 1024
    raw, gain, _, _ = _raw_drift_movie(t, h, w, torch.uint8, 23, 3)
    rd, gd = raw.to(dev), gain.to(dev)
    with pytest.raises(McorrUnsupported, match="0.5"):
        rm = engine.RawMovie(rd, gd, hot_pixel_threshold=0.5)
        engine.global_shifts_raw(rm, t // 2, 1.0, 500.0, (300, 10))
    got = mc.motion_correct_raw(rd, gd, 1.0, return_frames=True, hot_pixel_threshold=0.5, return_hot_counts=True)
    fa, sa, fra, ca = _conditioned_route(mc, rd, gd, thr=0.5)
    for a, b in zip(got, (fa, sa, fra, ca)):
        assert torch.equal(a, b)
    with pytest.raises(McorrUnsupported, match="hot_pixel_threshold=0.5"):
        mc.RawMoviePipeline(gd, dev, 1.0, hot_pixel_threshold=0.5).run([rd])


@pytest.mark.parametrize("with_gain", [True, False])
def test_pipeline_equals_one_call_per_movie(mc, dev, with_gain):
    movies, g = [], None
    for i in range(3):
        raw, gain, _, _ = _raw_drift_movie(4, 256, 4096, torch.uint8, 60 + i, 4)
        raw, gain = _add_hot_pixels(raw, gain, 80 + i)
        movies.append(raw.to(dev))
        g = gain if g is None else g
    gd = g.to(dev) if with_gain else None
    pipe = mc.RawMoviePipeline(gd, dev, 1.0, return_frames=True, overlap=True, hot_pixel_threshold=THR)
    res = pipe.run(movies)
    torch.cuda.synchronize()
    for m, r in zip(movies, res):
        f, s, fr = mc.motion_correct_raw(m, gd, 1.0, return_frames=True, hot_pixel_threshold=THR)
        assert torch.equal(r.field, f) and torch.equal(r.total, s) and torch.equal(r.frames, fr)


def test_default_is_unchanged(mc, dev):
    raw, gain, _, _ = _raw_drift_movie(6, 512, 4096, torch.uint8, 11, 5)
    raw, gain = _add_hot_pixels(raw, gain, 5)
    rd, gd = raw.to(dev), gain.to(dev)
    a = mc.motion_correct_raw(rd, gd, 1.0, return_frames=True)
    b = mc.motion_correct_raw(rd, gd, 1.0, return_frames=True, hot_pixel_threshold=None)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    f0, s0, c0 = mc.motion_correct_raw(rd, gd, 1.0, hot_pixel_threshold=None, return_hot_counts=True)
    assert int(c0.abs().sum()) == 0 and c0.dtype == torch.int32 and c0.shape == (6,)
    c = mc.motion_correct_raw(rd, gd, 1.0, return_frames=True, hot_pixel_threshold=1e6, return_hot_counts=True)
    assert torch.equal(c[0], a[0]) and int(c[3].sum()) == 0
    assert rel_err(c[1], a[1]) <= 1e-6 and rel_err(c[2], a[2]) <= 1e-6
