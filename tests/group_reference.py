"""The rolling frame-group rule of group_frames_raw, restated in numpy int64, and the low-dose movie the tests of
motion_correct_raw_grouped estimate on.  Nothing here imports the package."""

import numpy as np


def group_window(i, t, group):
    """First and last frame (inclusive) of output frame i's window."""
    return max(0, i - (group - 1) // 2), min(t - 1, i + group // 2)


def group_frames(movie, group):
    """(t, h, w) integer movie -> int64 sums over each frame's centred window of `group` frames, clipped at the ends
    of the movie.  One slice sum per output frame: no running sum, nothing shared with the kernel's form."""
    m = np.asarray(movie).astype(np.int64)
    t = m.shape[0]
    out = np.empty_like(m)
    for i in range(t):
        a, b = group_window(i, t, group)
        out[i] = m[a:b + 1].sum(axis=0)
    return out


def interior_frames(t, group):
    """Frames whose window is not clipped."""
    return [i for i in range(t) if i - (group - 1) // 2 >= 0 and i + group // 2 <= t - 1]


def low_dose_movie(dose, t=16, h=512, w=512, seed=2024, pad=32):
    """A u8 Poisson movie of `dose` counts per pixel and frame on average: a fixed white texture of rates in
    dose * [0.5, 1.5], cropped at a linear whole-pixel drift of +1 / -1 px per frame (y / x), as conftest.drift_stack
    crops its texture.  Returns (movie (t, h, w) uint8, dy (t,), dx (t,)); the shifts an estimator should find are
    dy - dy[t // 2] and dx - dx[t // 2] pixels.  numpy's legacy RandomState: the same bytes everywhere."""
    rs = np.random.RandomState(seed)
    rate = dose * (0.5 + rs.random_sample((h + 2 * pad, w + 2 * pad)))
    dy = np.arange(t) - t // 2
    dx = t // 2 - np.arange(t)
    frames = [rs.poisson(rate[pad - dy[f]:pad - dy[f] + h, pad - dx[f]:pad - dx[f] + w]) for f in range(t)]
    return np.clip(np.stack(frames), 0, 255).astype(np.uint8), dy, dx


def conditioned(movie):
    """float64 conditioning of an integer movie without a gain: each frame minus its own mean, as fp32."""
    m = np.asarray(movie).astype(np.float64)
    return (m - m.mean(axis=(1, 2), keepdims=True)).astype(np.float32)
