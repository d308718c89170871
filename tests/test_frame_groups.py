"""Rolling frame-group sums on the GPU (group_frames_raw: mc_raw_group_frames, csrc/raw_group.hip) against the numpy
int64 restatement of the window rule (tests/group_reference.py), and motion_correct_raw_grouped against the two
compositions its docstring names.  Integers and compositions: torch.equal throughout."""

import numpy as np
import pytest
import torch

import group_reference as gr
import oracle

pytestmark = pytest.mark.gpu

DTYPES = {"u8": torch.uint8, "i16": torch.int16}
# the smallest shapes at which piece ownership (16 u8 / 8 i16 pixels), the element path (927, 959: no whole
# pieces), more than one workgroup (4096 columns x 64 rows) and the window ends can each go wrong
SHAPES = [(1, 1, 1), (5, 3, 8), (7, 5, 48), (9, 33, 927), (3, 7, 959), (2, 64, 4096)]


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def random_movie(shape, dtype, seed):
    """numpy movie whose window sums stay inside int16 for every group: u8 full range (at most 9 frames: 9 * 255),
    i16 within +- 3000 (9 * 3000 = 27000)."""
    rs = np.random.RandomState(seed)
    if dtype == torch.uint8:
        return rs.randint(0, 256, size=shape).astype(np.uint8)
    return rs.randint(-3000, 3001, size=shape).astype(np.int16)


def want_groups(movie_np, group):
    want = gr.group_frames(movie_np, group)
    assert want.min() >= -32768 and want.max() <= 32767
    return torch.from_numpy(want.astype(np.int16))


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_restatement(mc, dev, shape, kind):
    t = shape[0]
    m = random_movie(shape, DTYPES[kind], seed=sum(shape))
    movie = torch.from_numpy(m).to(dev)
    for group in (1, 2, 3, 4, 8, t, 2 * t + 3):
        got = mc.group_frames_raw(movie, group)
        assert got.dtype == torch.int16 and got.shape == movie.shape and got.device == movie.device
        assert torch.equal(got.cpu(), want_groups(m, group)), (shape, kind, group)
    assert torch.equal(mc.group_frames_raw(movie, 1), movie.to(torch.int16))


@pytest.mark.parametrize("kind", list(DTYPES))
def test_storage_variants(mc, dev, kind):
    shape = (7, 5, 48)
    m = random_movie(shape, DTYPES[kind], seed=5)
    n = m.size
    # a contiguous view that starts one element off a 16-byte boundary: the element path for the whole call
    flat = torch.zeros(n + 1, dtype=DTYPES[kind], device=dev)
    flat[1:] = torch.from_numpy(m).to(dev).reshape(-1)
    view = flat[1:].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == view.element_size()
    assert torch.equal(mc.group_frames_raw(view, 3).cpu(), want_groups(m, 3))
    # a non-contiguous view is staged as the other raw routes stage it
    wide = random_movie((7, 10, 48), DTYPES[kind], seed=6)
    rows = torch.from_numpy(wide).to(dev)[:, ::2]
    assert not rows.is_contiguous()
    assert torch.equal(mc.group_frames_raw(rows, 4).cpu(), want_groups(np.ascontiguousarray(wide[:, ::2]), 4))
    # a CPU movie comes back on the CPU
    got = mc.group_frames_raw(torch.from_numpy(m), 2)
    assert got.device.type == "cpu" and torch.equal(got, want_groups(m, 2))


def test_extremes(mc, dev):
    full = torch.full((130, 2, 32), 255, dtype=torch.uint8, device=dev)
    got = mc.group_frames_raw(full, 128).cpu()
    assert torch.equal(got, want_groups(full.cpu().numpy(), 128))
    assert int(got.max()) == 32640 and torch.all(got[63:66] == 32640)  # lo = 63, hi = 64: frames 63 .. 65 see 128 frames
    top = torch.full((3, 2, 16), 32767, dtype=torch.int16, device=dev)
    with pytest.raises(ValueError, match="group=2"):
        mc.group_frames_raw(top, 2)
    with pytest.raises(ValueError, match="group=2"):  # the element path raises the flag as well
        mc.group_frames_raw(top[:, :, :13].contiguous(), 2)
    assert torch.equal(mc.group_frames_raw(top, 1), top)
    bottom = torch.full((3, 2, 16), -32768, dtype=torch.int16, device=dev)
    assert torch.equal(mc.group_frames_raw(bottom, 1), bottom)
    with pytest.raises(ValueError, match="group=3"):
        mc.group_frames_raw(bottom, 3)
    # one pixel of one window beyond the edge is enough, exactly on it is not
    edge = torch.zeros((4, 3, 24), dtype=torch.int16, device=dev)
    edge[1:3, 2, 23] = 16384
    with pytest.raises(ValueError, match="group=2"):
        mc.group_frames_raw(edge, 2)
    edge[2, 2, 23] = 16383
    assert int(mc.group_frames_raw(edge, 2).max()) == 32767
    edge[1:3, 2, 23] = -16384
    assert int(mc.group_frames_raw(edge, 2).min()) == -32768


def test_nothing_frame_sized_besides_the_output(mc, dev):
    t, h, w = 16, 1024, 1024
    movie = torch.from_numpy(random_movie((t, h, w), torch.uint8, seed=1)).to(dev)
    mc.group_frames_raw(movie[:2], 2)  # the library is loaded outside the measured call
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = mc.group_frames_raw(movie, 3)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak <= 2 * t * h * w + (1 << 20), peak
    assert out.dtype == torch.int16


# ------------------------------------------------------------------ motion_correct_raw_grouped


def poisson_drift_movie(dev, dtype, t=8, h=1024, w=1024, seed=77):
    """Poisson counts of a smooth texture cropped at a whole-pixel drift, divided by a gain of 1 +- 0.1."""
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.rand(h + 32, w + 32, generator=g, device=dev)
    base = (base + torch.roll(base, 1, 0) + torch.roll(base, 1, 1) + torch.roll(base, (1, 1), (0, 1))) / 4
    gain = 1.0 + 0.1 * (2 * torch.rand(h, w, generator=g, device=dev) - 1)
    raw = torch.empty((t, h, w), dtype=dtype, device=dev)
    for f in range(t):
        oy, ox = 16 + f - t // 2, 16 - (f - t // 2)
        counts = torch.poisson(4.0 + 12.0 * base[oy:oy + h, ox:ox + w], generator=g)
        if dtype == torch.uint8:
            raw[f] = (counts / gain).round().clamp(0, 255).to(dtype)
        else:
            raw[f] = (40 * counts / gain - 300).round().clamp(-32768, 32767).to(dtype)
    return raw, gain


@pytest.fixture(scope="module")
def drift_movies(dev):
    return {kind: poisson_drift_movie(dev, dtype) for kind, dtype in DTYPES.items()}


@pytest.mark.parametrize("kind", list(DTYPES))
def test_grouped_whole_image_route_is_the_composition(mc, dev, drift_movies, kind):
    raw, gain = drift_movies[kind]
    ps, dose = 1.1, 1.0
    grouped = mc.group_frames_raw(raw, 3)
    field = mc.motion_correct_raw_fast(grouped, gain, ps)[0]
    want = mc.motion_correct_sum_fast_raw(raw, gain, field, ps, dose_per_frame=dose, return_plain_sum=True)
    got = mc.motion_correct_raw_grouped(raw, gain, ps, 3, dose_per_frame=dose, return_plain_sum=True)
    assert len(got) == 3 and torch.equal(got[0], field)
    assert torch.equal(got[1], want[0]) and torch.equal(got[2], want[1])
    assert float(field.abs().max()) > 0
    plain = mc.motion_correct_raw_grouped(raw, gain, ps, 3)
    assert len(plain) == 2 and torch.equal(plain[0], field) and torch.equal(plain[1], want[1])
    # group = 1 estimates on the movie itself
    f1 = mc.motion_correct_raw_grouped(raw, gain, ps, 1)[0]
    assert torch.equal(f1, mc.motion_correct_raw_fast(raw, gain, ps)[0])


@pytest.mark.parametrize("kind", list(DTYPES))
def test_grouped_patch_route_is_the_composition(mc, dev, drift_movies, kind):
    raw, gain = drift_movies[kind]
    ps = 1.0
    grouped = mc.group_frames_raw(raw, 3)
    field, centres, _ = mc.motion_correct_raw_patches(grouped, gain, ps, 1024)
    want = mc.motion_correct_sum_raw(raw, gain, field, ps, dose_per_frame=1.0)
    got = mc.motion_correct_raw_grouped(raw, gain, ps, 3, patch_sidelength=1024, dose_per_frame=1.0)
    assert len(got) == 3 and torch.equal(got[0], field) and torch.equal(got[1], centres)
    assert torch.equal(got[2], want)


# ------------------------------------------------------------------ a low-dose movie

LOW_DOSE = 0.5


def test_low_dose_field_is_the_oracles_on_the_grouped_movie(mc, dev):
    """The seeded low-dose u8 Poisson movie of group_reference.low_dose_movie, (16, 512, 512), +1 / -1 px of drift
    per frame, group = 5, no gain: the field motion_correct_raw_grouped returns equals
    oracle.estimate_global_motion on the float64-conditioned restated groups (torch.equal, the rule of
    tests/test_gpu_parity.py for global shifts).

    The second half that was asked of this test -- a dose at which the oracle misses the planted shift by more than
    1 px on at least a quarter of the single frames and is within 0.5 px of it on every interior frame of the
    grouped movie -- is NOT asserted: no dose of 8, 4, 2, 1, 0.5, 0.3, 0.2, 0.1, 0.05, 0.03, 0.02, 0.01 counts per
    pixel and frame satisfies both under the oracle alone, and the bounds were not loosened.  Rolling windows that
    overlap the reference frame's window share raw frames with it; their shot noise correlates at zero shift, and on
    this grid that peak (4 shared frames of 5) beats the texture's wherever single frames fail.  The oracle's errors
    in pixels, max(|dy|, |dx|) per frame, reference frame 8:

      dose 0.5  single frames  13 69 107 75 3 2 57 38 0 45 49 30 20 77 1 45     (> 1 px on 14 of 16)
                groups of 5     0  1   1  1 3 3  2  1 0  1  2  2  3  0 1  1     (interior 2..13: up to 3 px)
      dose 1.0  single frames   1  1   1  0 1 53 1  1 0  1  2 17  1 24 26 1     (> 1 px on 5 of 16)
                groups of 5     1  0   0  0 2  2 1  1 0  1  2  2  2  0 1  1     (interior: up to 2 px)
      dose 2.0  single frames: none beyond 1 px; groups of 5: 1 px on 9 interior frames.

    At dose 0.5 the groups bring 14 lost frames back to within 3 px; they do not reach 0.5 px."""
    m, dy, dx = gr.low_dose_movie(LOW_DOSE)
    t = m.shape[0]
    grouped = gr.group_frames(m, 5)
    want = oracle.estimate_global_motion(torch.from_numpy(gr.conditioned(grouped)), 1.0)
    single = oracle.estimate_global_motion(torch.from_numpy(gr.conditioned(m)), 1.0)
    planted = torch.from_numpy(np.stack([dy - dy[t // 2], dx - dx[t // 2]])).float()[:, :, None, None]
    err_single = (single - planted).abs().amax(0).flatten()
    err_grouped = (want - planted).abs().amax(0).flatten()
    print("oracle error, single frames:", err_single.tolist())
    print("oracle error, groups of 5:  ", err_grouped.tolist())
    field, total = mc.motion_correct_raw_grouped(torch.from_numpy(m).to(dev), None, 1.0, 5)
    print("device field error:         ", (field.cpu() - planted).abs().amax(0).flatten().tolist())
    assert field.shape == (2, t, 1, 1) and total.shape == m.shape[1:]
    assert torch.equal(field.cpu(), want)
    assert int((err_single > 1.0).sum()) >= t // 4  # the single frames are lost at this dose
    assert float(err_grouped.max()) < float(err_single.max())
