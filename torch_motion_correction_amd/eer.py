"""EER event movies (Falcon 4 / 4i) rendered into raw u8 movies on the device.

The reference's example flow starts with ``movie = eerfile.render(eer_file, dose_per_output_frame=...,
total_fluence=...)`` (examples/ttMotion.py, ``main()``): an ``.eer`` file is a TIFF or BigTIFF whose frames are
run-length-coded electron events, 1 000 - 3 000 detector frames in 0.5 - 1 GB.  This module is that first step:

  read_eer                 a pure-Python walk of the file's IFD chain -> ``EerMovie`` (the bytes and each frame's strip)
  render_eer_raw           the strips decoded on the GPU: output frame k = the per-pixel event count of the input
                           frames k g .. k g + g - 1, a (t_out, up h, up w) uint8 movie (mc_eer_render)
  eer_frames_per_fraction  the example's two dose parameters turned into ``group``

The result is a raw movie for every ``*_raw*`` function, ``RawStatistics`` and the pipelines, as the outputs of
``group_frames_raw`` and ``fill_defects_raw`` are.  The codec rule is stated once, in csrc/eer.h; it covers the
7-bit-run / 4-bit-sub-pixel layout (TIFF compression 65001, and 65002 when its tags give 7, 2, 2) and was written
from the public description of the format: no vendor-written file has been decoded with it.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from ._files import _check_data, _int, _positive_ints, read_file, require_tags, walk_ifds
from ._lib import check, device_scope, load, ptr, require_gpu, stream_ptr

SEGMENT_BYTES = 64   # the segment size of the parallel parse, chosen by measurement among 64, 128, 256
MAX_GROUP = 255      # a uint8 count holds one event per pixel of at most 255 frames
MAX_STRIP_BYTES = 2**28

_TAG_NAMES = {256: "ImageWidth", 257: "ImageLength", 259: "Compression", 273: "StripOffsets",
              279: "StripByteCounts", 65007: "EER rle bits", 65008: "EER horizontal sub-pixel bits",
              65009: "EER vertical sub-pixel bits"}


def _check_render_args(data, offsets, nbytes, shape, group, upsampling, rle_bits):
    """Every argument rule of render_eer_raw -> (offsets, nbytes, h, w, group) as Python ints; ValueError otherwise."""
    _check_data(data)
    h, w = _positive_ints(shape, 2, f"shape must be the detector's (h, w), got {shape!r}")
    if h * w >= 2**31:
        raise ValueError(f"shape {(h, w)}: detectors of 2^31 pixels and more are not supported")
    if rle_bits != 7:
        raise ValueError(f"rle_bits={rle_bits!r}: only the 7-bit-run / 4-bit-sub-pixel layout (compression 65001) is "
                         "decoded; 8-bit runs (compression 65000) are not supported")
    if upsampling not in (1, 2) or isinstance(upsampling, bool):
        raise ValueError(f"upsampling must be 1 or 2, got {upsampling!r} (4 is not supported)")
    if (upsampling * w) % 4:
        raise ValueError(f"upsampling * w = {upsampling * w} must be a multiple of 4")
    group = _int(group, "group", 1)
    if group > MAX_GROUP:
        raise ValueError(f"group={group}: a uint8 count holds at most {MAX_GROUP} frames")
    try:
        offsets = [_int(o, "an offset", 0) for o in offsets]
        nbytes = [_int(n, "a byte count", 0) for n in nbytes]
    except TypeError:
        raise ValueError("offsets and nbytes must be sequences of ints, one per frame") from None
    if len(offsets) != len(nbytes) or not offsets:
        raise ValueError(f"offsets and nbytes must name the same frames, at least one: got {len(offsets)} and "
                         f"{len(nbytes)}")
    if len(offsets) < group:
        raise ValueError(f"group={group} needs at least that many frames, got {len(offsets)}")
    total = int(data.numel())
    for i, (o, n) in enumerate(zip(offsets, nbytes)):
        if o + n > total:
            raise ValueError(f"frame {i}: its strip (offset {o}, {n} bytes) leaves the {total} bytes of data")
        if n >= MAX_STRIP_BYTES:
            raise ValueError(f"frame {i}: strips of 2^28 bytes and more are not supported, got {n}")
    return offsets, nbytes, h, w, group


def _render(data, offsets, nbytes, h, w, group, upsampling, device, segment_bytes=None):
    """The checked arguments rendered -> (movie, final n, event counts), all on the device."""
    seg = SEGMENT_BYTES if segment_bytes is None else segment_bytes
    n = len(offsets)
    dev = require_gpu(device if device is not None else data.device)
    with device_scope(dev):
        buf = data.detach().to(dev).contiguous()
        if buf.numel() == 0:  # frames without bytes: a pointer the library can take
            buf = torch.zeros(8, dtype=torch.uint8, device=dev)
        segments = sum((b + seg - 1) // seg for b in nbytes)
        scratch = torch.empty(3 * n + (13 * segments + 1) // 2, dtype=torch.int64, device=dev)
        out = torch.empty((n // group, upsampling * h, upsampling * w), dtype=torch.uint8, device=dev)
        final_n = torch.empty(n, dtype=torch.int32, device=dev)
        events = torch.empty(n, dtype=torch.int32, device=dev)
        off_c, nb_c = (C.c_int64 * n)(*offsets), (C.c_int64 * n)(*nbytes)
        check(load().mc_eer_render(ptr(buf), int(data.numel()), off_c, nb_c, n, h, w, 7, upsampling, group, seg,
                                   ptr(out), ptr(final_n), ptr(events), ptr(scratch), 8 * scratch.numel(),
                                   stream_ptr(dev)), "mc_eer_render")
    return out, final_n, events


def render_eer_raw(data, offsets, nbytes, shape, group, upsampling=1, rle_bits=7, return_event_counts=False,
                   device=None):
    """EER frames rendered into a raw movie: the (t_out, up h, up w) uint8 tensor, contiguous and on the GPU, whose
    frame ``k`` is the per-pixel event count of the input frames ``k group .. k group + group - 1``; ``t_out =
    n_frames // group``, the trailing ``n_frames - t_out * group`` frames are dropped (RELION ``--eer_grouping``).

    ``data``: a 1-D uint8 tensor (CPU or GPU) that holds the frames' strips anywhere in it -- it may be the whole
    file.  ``offsets`` / ``nbytes``: one int per frame, the strip's first byte and length in ``data``.  ``shape``:
    the detector's physical pixels ``(h, w)``.  ``upsampling`` 1 puts an event at its pixel, 2 at the half pixel its
    sub-pixel code names (csrc/eer.h states the rule); ``upsampling * w`` must be a multiple of 4.  ``rle_bits``
    must be 7 (TIFF compression 65001): 8-bit runs (65000) and ``upsampling=4`` are refused.

    Exact integers.  Within one input frame positions strictly increase, so a pixel gets at most one event per
    frame and a count is at most ``group <= 255``: nothing saturates.  A frame whose stream does not end exactly at
    ``h * w`` pixels (cut short, or its last run overshoots) raises ValueError naming the first such frame -- from
    the one device-to-host read of the per-frame final pixel counts.  Every other argument rule, a strip outside
    ``data`` included, is a ValueError raised before any device is touched.  The kernels read no byte outside a
    frame's own strip, whatever its bits say.

    With ``return_event_counts`` the result is ``(movie, counts)``, counts = the (n_frames,) int32 events per input
    frame.  ``device``: the GPU to render on (None: the device of ``data``, the current GPU for a CPU tensor)."""
    offsets, nbytes, h, w, group = _check_render_args(data, offsets, nbytes, shape, group, upsampling, rle_bits)
    out, final_n, events = _render(data, offsets, nbytes, h, w, group, upsampling, device)
    ends = final_n.cpu()
    bad = torch.nonzero(ends != h * w)
    if bad.numel():
        i = int(bad[0])
        raise ValueError(f"frame {i}: its stream ends at pixel {int(ends[i])} of {h * w} "
                         f"({'cut short' if int(ends[i]) < h * w else 'its last run overshoots'}): not a "
                         "well-formed EER frame")
    return (out, events) if return_event_counts else out


def eer_frames_per_fraction(n_frames, total_fluence, dose_per_output_frame):
    """``group`` for ``render_eer_raw`` from the example's two parameters: ``max(1, round(dose_per_output_frame *
    n_frames / total_fluence))`` input frames per output frame (Python's round).  The rule is this package's; it is
    not checked against ``eerfile``."""
    n = _int(n_frames, "n_frames", 1)
    total, dose = float(total_fluence), float(dose_per_output_frame)
    if not (0.0 < total < float("inf")) or not (0.0 < dose < float("inf")):
        raise ValueError(f"total_fluence and dose_per_output_frame must be positive numbers, got {total_fluence!r}, "
                         f"{dose_per_output_frame!r}")
    return max(1, round(dose * n / total))


@dataclass
class EerMovie:
    """An ``.eer`` file as ``read_eer`` found it: ``data`` (1-D uint8, the whole file), ``offsets`` / ``nbytes`` (one
    int per frame, file order), ``shape`` (h, w) and ``rle_bits``."""

    data: torch.Tensor
    offsets: list
    nbytes: list
    shape: tuple
    rle_bits: int

    def render(self, group, upsampling=1, device=None):
        """``render_eer_raw`` of this movie."""
        return render_eer_raw(self.data, self.offsets, self.nbytes, self.shape, group, upsampling=upsampling,
                              rle_bits=self.rle_bits, device=device)


def read_eer(path):
    """An ``.eer`` file -> ``EerMovie``: a walk of the TIFF (magic 42) or BigTIFF (magic 43) IFD chain in plain
    Python, no decoder involved.  Every IFD is one frame and must give ImageWidth, ImageLength, Compression,
    StripOffsets and StripByteCounts, with ONE strip; the shape and the compression must be the same throughout.
    Compression 65001 is the 7-bit-run layout, 65002 is accepted when its tags 65007 - 65009 give 7, 2, 2 (absent
    tags mean those defaults); 65000 (8-bit runs) and anything else raise ValueError, as does every other deviation,
    with the tag named."""
    raw, size, data = read_file(path)

    def fail(msg):
        raise ValueError(f"{path}: {msg}")

    offsets, nbytes, shape, compression = [], [], None, None
    for i, found in enumerate(walk_ifds(raw, size, _TAG_NAMES, fail)):
        require_tags(found, _TAG_NAMES, i, fail)
        for tag, (_, values) in found.items():
            if len(values) != 1:
                fail(f"frame {i}: {_TAG_NAMES[tag]} has {len(values)} values; one strip and one value per frame are "
                     "required")
        tags = {tag: values[0] for tag, (_, values) in found.items()}
        comp = tags[259]
        if comp == 65002:
            layout = (tags.get(65007, 7), tags.get(65008, 2), tags.get(65009, 2))
            if layout != (7, 2, 2):
                fail(f"frame {i}: Compression 65002 with (rle, horizontal, vertical) bits {layout}; only (7, 2, 2) is "
                     "decoded")
        elif comp != 65001:
            fail(f"frame {i}: Compression {comp} is not supported (65001, or 65002 with 7, 2, 2 bits"
                 + ("; 65000 has 8-bit runs)" if comp == 65000 else ")"))
        if compression is None:
            compression, shape = comp, (tags[257], tags[256])
        elif comp != compression:
            fail(f"frame {i}: Compression {comp} differs from the first frame's {compression}")
        elif (tags[257], tags[256]) != shape:
            fail(f"frame {i}: ImageLength x ImageWidth {(tags[257], tags[256])} differs from the first frame's "
                 f"{shape}")
        if tags[273] + tags[279] > size:
            fail(f"frame {i}: StripOffsets + StripByteCounts = {tags[273] + tags[279]} leaves the file of {size} "
                 "bytes")
        offsets.append(tags[273])
        nbytes.append(tags[279])
    if shape[0] < 1 or shape[1] < 1:
        fail(f"ImageLength x ImageWidth {shape} is empty")
    return EerMovie(data=data, offsets=offsets, nbytes=nbytes, shape=shape, rle_bits=7)
