"""Test-side restatement of the EER codec rule (csrc/eer.h) in numpy and Python integers: an encoder, the sequential
decoder, a renderer, and the EER flavour of the container writer (tests/tiff_files.py).  Nothing here is imported by
the package; scripts/eer_render_time.py reuses the encoder.

The rule.  A frame of a detector with N = h * w pixels is a little-endian bit stream (bit k of the stream is bit
k & 7 of byte k >> 3).  With bit = 0, n = 0:

    loop:  p = 7 bits at `bit`;  bit += 7;  n += p
           if n >= N: stop
           if p == 127: continue
           s = 4 bits at `bit`;  bit += 4;  event at linear position n with sub-pixel code s;  n += 1

and decoding also stops when the next symbol would begin at or after bit 8 * nbytes; bits beyond the strip read as
zero.  A well-formed stream stops with n == N."""

import numpy as np

import tiff_files

RUN_MAX = 127


def encode_frame(positions, subs, n_pixels):
    """The stream of one frame: `positions` strictly increasing linear positions < n_pixels, `subs` their 4-bit codes
    -> bytes.  Before each event, gap // 127 skips and a run of gap % 127; after the last one, the runs that bring n
    to n_pixels (skips, then the rest if any), which is one run of 0 when the last event sits on the last pixel.
    Vectorised: symbol lengths -> cumsum -> bit scatter."""
    pos = np.asarray(positions, dtype=np.int64)
    sub = np.asarray(subs, dtype=np.int64)
    assert pos.shape == sub.shape and pos.ndim == 1
    assert pos.size == 0 or (pos[0] >= 0 and pos[-1] < n_pixels and np.all(np.diff(pos) > 0))
    prev_end = np.concatenate(([0], pos[:-1] + 1)) if pos.size else pos
    gap = pos - prev_end
    skips = gap // RUN_MAX
    count = skips + 1  # symbols per event: its skips and its run + code
    last = np.cumsum(count) - 1
    vals = np.full(int(count.sum()), RUN_MAX, dtype=np.int64)
    lens = np.full(vals.size, 7, dtype=np.int64)
    vals[last] = (gap % RUN_MAX) | (sub << 7)
    lens[last] = 11
    rest = n_pixels - (int(pos[-1]) + 1 if pos.size else 0)
    tail = [RUN_MAX] * (rest // RUN_MAX) + ([rest % RUN_MAX] if rest % RUN_MAX or rest == 0 else [])
    vals = np.concatenate((vals, np.asarray(tail, dtype=np.int64)))
    lens = np.concatenate((lens, np.full(len(tail), 7, dtype=np.int64)))
    starts = np.cumsum(lens) - lens
    bits = np.zeros(int(lens.sum()), dtype=np.uint8)
    for b in range(11):
        m = lens > b
        bits[starts[m] + b] = (vals[m] >> b) & 1
    return np.packbits(bits, bitorder="little").tobytes()


def decode_frame(strip, n_pixels):
    """The sequential decoder of the rule -> (positions, subs, final n): an int.from_bytes walk.  Positions at and
    beyond n_pixels never occur: decoding stops first."""
    v = int.from_bytes(bytes(strip), "little")
    end = 8 * len(strip)
    bit = n = 0
    positions, subs = [], []
    while bit < end:
        p = (v >> bit) & 127
        bit += 7
        n += p
        if n >= n_pixels:
            break
        if p == RUN_MAX:
            continue
        subs.append((v >> bit) & 15)
        bit += 4
        positions.append(n)
        n += 1
    return positions, subs, n


def entry_offsets(strip, n_pixels, segment_bytes):
    """The offsets, within their segments, of the first symbol of every segment after the first (unstopped parse)."""
    v = int.from_bytes(bytes(strip), "little")
    end = 8 * len(strip)
    bit, seen, seg = 0, set(), 0
    while bit < end:
        if bit // (8 * segment_bytes) != seg:
            seg = bit // (8 * segment_bytes)
            seen.add(bit - seg * 8 * segment_bytes)
        p = (v >> bit) & 127
        bit += 7 if p == RUN_MAX else 11
    return seen


def render(strips, shape, group, upsampling=1):
    """(t_out, up h, up w) uint8 from the frames' strips (np.add.at), the (n_frames,) final n and event counts."""
    h, w = shape
    up = upsampling
    t_out = len(strips) // group
    out = np.zeros((t_out, up * h, up * w), dtype=np.int64)
    final_n, counts = [], []
    for f, strip in enumerate(strips):
        positions, subs, n = decode_frame(strip, h * w)
        final_n.append(n)
        counts.append(len(positions))
        if f // group >= t_out:
            continue
        pos, s = np.asarray(positions, dtype=np.int64), np.asarray(subs, dtype=np.int64)
        y, x = pos // w, pos % w
        if up == 2:
            y, x = 2 * y + ((s >> 3) & 1), 2 * x + ((s >> 1) & 1)
        np.add.at(out[f // group], (y, x), 1)
    assert out.max(initial=0) <= 255
    return out.astype(np.uint8), np.asarray(final_n, dtype=np.int32), np.asarray(counts, dtype=np.int32)


def random_frame(rng, n_pixels, density):
    """One `random(N) < d` mask, then `integers(0, 16)` codes -> (positions, subs)."""
    positions = np.nonzero(rng.random(n_pixels) < density)[0]
    return positions, rng.integers(0, 16, size=positions.size)


def lay_out(strips, order, lead=1, gap=3, odd=True):
    """tiff_files.lay_out for frames of one strip -> (bytes, offsets, nbytes) with offsets / nbytes in frame order."""
    buf, offsets, nbytes = tiff_files.lay_out([[s] for s in strips], order, lead, gap, odd)
    return buf, [o[0] for o in offsets], [n[0] for n in nbytes]


def write_tiff(path, strips, shape, big=False, compression=65001, order=None, overrides=None, byte_order="<"):
    """tiff_files.write_tiff with an EER file's tags: one strip per frame, no BitsPerSample, RowsPerStrip or
    SampleFormat.  Returns (offsets, nbytes) in frame order."""
    tags = {256: (4, 1, shape[1]), 257: (4, 1, shape[0]), 259: (3, 1, compression)}
    offsets, nbytes = tiff_files.write_tiff(path, [[s] for s in strips], tags, big=big, byte_order=byte_order,
                                            order=order, array_types=(16 if big else 4, 4), overrides=overrides)
    return [o[0] for o in offsets], [n[0] for n in nbytes]
