"""What a caller may hand to a route, over the table of tests/route_cases.py: an input that starts off a 16-byte
boundary, an input it wants back unmodified, and the same call again after anything else.

1.  Off-boundary inputs.  api._stage is `.to(device).contiguous()`: a contiguous tensor viewed out of a larger buffer
    (`flat[1:].view(t, h, w)`) reaches the kernels where it lies, and many of them read float4 / float2.  A vector
    load at the next lower boundary reads the neighbouring sample, silently.  Each case's result on aligned inputs
    is compared with its result on kernel_harness.relocated() twins (one element past a boundary, all-ones padding
    around them): each input in turn, then all together.  Integer and bool results are equal bit for bit.
    Floating-point results are equal bit for bit where the same sequence of entry points ran and the case has no
    `rel`; otherwise (another engine answered, or double atomics) within `case.rel or ALIGN_REL` of the result's
    largest value, 1e-4 as route_cases.ATOMIC_REL for its reason: two correct engines differ in their last bits, and
    a load displaced by one sample of these inputs (noise of rms 2 on a level of 5, gains over a factor of 16,
    full-range integers) is wrong by tenths of the output's largest value.  A route that enters through the engine
    or the package answers; only a case that calls `lib` itself on buffers it staged may refuse, from its first
    entry point, and only if REFUSES quotes the header line that states the requirement.

2.  Inputs are left alone: every tensor of a case's inputs, those held by a RawMovie, a DefectFill or a
    LocalMotionProblem included, holds the same bits after the route, unless WRITES_IN_PLACE quotes the product's
    own text that says it is written.

3.  A result does not depend on what ran before: results pass through plan._PLANS, plan._LINES, plan._TWIDDLES,
    engine._CONST and the lazily built pl.mhat.  Every case runs in table order, then again in reverse order with
    every other configuration through the caches in between, then (first and last three) after the caches were
    cleared and the plans rebuilt.

Figures (MI355X), printed as ALIGN lines (per variant the worst relative difference, per case the worst over the
bound): the largest is 0 -- every variant of every case gave the aligned result bit for bit, the `rel` cases and the
ones whose C entry switches engine on a misaligned pointer (the K1 route rule, condition.hip's `vec`) included, each
with the aligned run's sequence of entry points; the one listed direct case refused all three of its variants.
Before the staging fixes this file came with, the routes of seven cases refused instead: fourier_shift on the
row-major kernels (mc_full_rows_forward) and every RawMovie route but the patch row pass (global_shifts_raw on both
row engines, fast_shift_sums with and without hot pixels, warp_rigid_raw, warp_field_raw).  The three tests take 4 s
together, the slowest case 0.6 s (the first, which loads the library)."""

import pytest
import torch

import kernel_harness as kh
from route_cases import CASES

ALIGN_REL = 1e-4  # = route_cases.ATOMIC_REL, for the reason given there and above; not tuned to the figures

# case name -> (input name, the docstring or header line that says the route writes it).  Closed: a route that writes
# to a caller's tensor without saying so is a bug of the route.  An excused input must in fact change.
WRITES_IN_PLACE = {}

# case name -> the header line that states the alignment requirement.  Only for cases that call `lib` themselves on
# buffers they staged (DIRECT); a listed case must in fact refuse.
REFUSES = {
    "raw hot-pixel list": "required (pass ones for none); w % 8 == 0 and 8-byte (u8) / 16-byte aligned raw, 16-byte "
                          "aligned gain,",
}

# The cases whose route calls the library itself, on buffers and device tables staged in make(): the "(direct)"
# cases, and the hot-pixel list, whose two entry points stand between read-backs in RawMovie.__init__.
DIRECT = tuple(c.name for c in CASES if c.name.endswith("(direct)")) + ("raw hot-pixel list",)

IDS = [c.name for c in CASES]

align = kh.ratios_fixture("ALIGN")


@pytest.fixture
def rec(monkeypatch):
    """A Recorder over every module that binds `load` (the modules of test_stream_order's `rec`)."""
    from torch_motion_correction_amd import _lib, calibration, eer, mrc, tiff

    r = kh.Recorder(_lib.load())
    for mod in (_lib, calibration, eer, mrc, tiff):
        monkeypatch.setattr(mod, "load", lambda: r)
    return r


# ------------------------------------------------------------------ the closed dicts (no GPU)


def test_excuses_and_refusals_are_closed():
    names = {c.name for c in CASES}
    assert len(CASES) >= 39 and len(names) == len(CASES) and len(DIRECT) == 5 and set(DIRECT) <= names
    import inspect

    import route_cases

    for c in CASES:  # a direct case never enters through an engine or package-level route function
        if c.name in DIRECT:
            src = inspect.getsource(c.route)
            assert "lib.mc_" in src and "E()." not in src.replace("E().hot_list_capacity", ""), c.name
    assert set(REFUSES) <= set(DIRECT), sorted(set(REFUSES) - set(DIRECT))
    assert len(REFUSES) <= len(DIRECT)
    header = " ".join(kh_header().split())
    for name, line in REFUSES.items():
        assert len(line) > 20 and " ".join(line.split()) in header, f"{name}: not a line of include/mcorr.h"
    assert set(WRITES_IN_PLACE) <= names
    for name, (arg, line) in WRITES_IN_PLACE.items():
        assert len(line) > 20 and any(" ".join(line.split()) in text for text in product_texts()), \
            f"{name}: {line!r} is not the product's own text"
    assert route_cases.CASES is CASES


def kh_header():
    import os

    with open(os.path.join(kh.ROOT, "include", "mcorr.h")) as fh:
        return fh.read()


def product_texts():
    """The header and every Python source of the package, blanks folded: where an excuse's quotation must stand."""
    import glob
    import os

    yield " ".join(kh_header().split())
    for path in sorted(glob.glob(os.path.join(kh.ROOT, "torch_motion_correction_amd", "**", "*.py"), recursive=True)):
        with open(path) as fh:
            yield " ".join(fh.read().split())


def test_a_displaced_sample_is_far_beyond_the_bound():
    """What ALIGN_REL is set against: the inputs of the table read one sample off, and two correct engines' last
    bits."""
    x = kh.float_stack(2, 61, 67)
    for base in (x, kh.raw_movie(2, 64, 96, torch.int16, 4).float(), kh.gain(64, 96)):
        shifted = torch.roll(base.flatten(), 1).view_as(base)
        assert kh.rel_err(shifted, base) > 0.1 > 100 * ALIGN_REL
        with pytest.raises(AssertionError, match="relative error"):
            kh.assert_close_rel(shifted, base, ALIGN_REL, "one sample off")
    assert kh.rel_err(x * (1 + 2.0 ** -22), x) < ALIGN_REL / 100  # a few last bits of fp32


# ------------------------------------------------------------------ inputs are left alone


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_inputs_are_left_unchanged(dev, rec, c):
    with torch.cuda.device(dev):
        inputs = c.make(dev)
        torch.cuda.synchronize()
        snap = kh.snapshot(inputs)
        assert snap or c.name == "plan tables", "a case without a tensor input"
        c.route(**inputs)
        torch.cuda.synchronize()
    excused = WRITES_IN_PLACE.get(c.name, (None,))[0]
    assert excused is None or excused in inputs, excused
    kh.assert_inputs_unchanged({k: v for k, v in inputs.items() if k != excused}, snap, c.name)
    if excused is not None:  # a stale excuse fails
        with pytest.raises(AssertionError, match="was written to"):
            kh.assert_inputs_unchanged({excused: inputs[excused]}, snap, c.name)


# ------------------------------------------------------------------ off-boundary inputs


def _compare(got, want, same_calls, c, what):
    """-> the worst relative difference of the floating-point results (0.0 where they are held to the same bits)."""
    if same_calls and c.rel is None:
        kh.assert_same_bits(got, want, what)
        return 0.0
    kh.assert_close_rel(got, want, c.rel or ALIGN_REL, what)  # integer and bool results: bit for bit
    return max([kh.rel_err(a, b) for a, b in zip(kh.leaves(got), kh.leaves(want)) if a.is_floating_point()] or [0.0])


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_off_boundary_inputs_give_the_aligned_result(dev, rec, align, c):
    from torch_motion_correction_amd._lib import McorrUnsupported

    with torch.cuda.device(dev):
        inputs = c.make(dev)
        torch.cuda.synchronize()
        rec.clear()
        want = c.route(**inputs)
        torch.cuda.synchronize()
        aligned_calls = list(rec.names)
        movable = [k for k, v in inputs.items() if kh._has_tensors(v) and kh.snapshot({k: v})]
        variants = [(k, (k,)) for k in movable] + [("all inputs", tuple(movable))]
        refused = []
        for label, names in variants:
            moved, pairs = kh.twins({k: inputs[k] for k in names}, kh.relocated)
            assert all(a.numel() == 0 or a.data_ptr() % 16 == a.element_size() for a, _ in pairs)
            what = f"{c.name}, off the boundary: {label}"
            rec.clear()
            try:
                got = c.route(**{**inputs, **moved})
            except (McorrUnsupported, ValueError) as e:
                assert c.name in REFUSES, f"{what}: refused ({e}); a route answers, only a listed direct case may not"
                assert len(rec.names) == 1, f"{what}: refused after {rec.names}, not from its first entry point"
                refused.append(label)
                continue
            torch.cuda.synchronize()
            same = rec.names == aligned_calls
            worst = _compare(got, want, same, c, what)
            kh.worse(align, c.name, worst / (c.rel or ALIGN_REL))
            print(f"ALIGN {what}: {worst:.3e}{'' if same else '; another sequence of entry points: ' + str(rec.names)}")
        if c.name in REFUSES:
            assert "all inputs" in refused, f"{c.name} is listed in REFUSES and answered"


# ------------------------------------------------------------------ the same call again, after anything else


def _same(got, want, c, what):
    if c.rel is None:
        kh.assert_same_bits(got, want, what)
    else:
        kh.assert_close_rel(got, want, c.rel, what)


@pytest.mark.gpu
def test_second_pass_equals_the_first(dev):
    """Every case in table order, its result kept on the CPU; no cache is cleared; every case again in reverse order:
    between a case's two runs every other configuration has been through plan._PLANS, plan._LINES, plan._TWIDDLES,
    engine._CONST and the plans' mhat.  Then the caches are cleared and the first and last three cases run a third
    time: engine._CONST holds a key by id(pl), and the rebuilt plans are other objects.  A case's inputs are made
    once (a RawMovie's statistics come from double atomics: a second make() would differ in their last bits)."""
    from torch_motion_correction_amd import engine, plan

    def run(c):
        out = [x.detach().cpu() for x in kh.leaves(c.route(**inputs[c.name]))]
        torch.cuda.synchronize()
        return out

    with torch.cuda.device(dev):
        inputs, first = {}, {}
        for c in CASES:
            inputs[c.name] = c.make(dev)
            torch.cuda.synchronize()
            first[c.name] = run(c)
        for c in reversed(CASES):
            _same(run(c), first[c.name], c, f"{c.name}, second pass")
        plan.clear_plan_cache()
        engine._CONST.clear()
        for c in CASES[:3] + CASES[-3:]:
            _same(run(c), first[c.name], c, f"{c.name}, after the caches were cleared")
