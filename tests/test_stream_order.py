"""Stream ordering: every stream-taking entry point of libmcorr behind a delayed producer on a side stream.

include/mcorr.h: every call is asynchronous on the `stream` it is given and never synchronises; the Python layer
launches on the current stream of the buffers' device (_lib.stream_ptr).  On the default stream a launch on the wrong
stream gives the right answer, so every other test is blind to it.  Here (kernel_harness.gated_run) a case's inputs
are staged and its result computed on the default stream; then, on a fresh side stream S, a sleep kernel (the gate) is
followed by copies of the true inputs over NaN / complemented twins and by the route on the twins.  Whatever the route
enqueues on another side stream runs at once on poison (the null stream not reliably so: see the control).  The
GatedRecorder holds, per entry-point call, the stream argument and whether the gate was still pending before and
after the call: an entry point is PROVEN when it was called and returned with the gate pending (so it did not wait
for the stream either), its stream argument was S, and the case's result matched.  A call after the gate has opened
proves nothing and fails as inconclusive.  Each case runs once; nothing is repeated to catch a race, no graph is
captured.

Where a Python route uploads a per-call table from host memory ahead of an entry point (which waits for the stream as
a read-back does), the entry point is called through `lib` on device tables staged beforehand.  EXEMPT holds the two
entry points that block the host by design; their stream argument is still asserted to be S and their result to
match.  The coverage check (no GPU) holds the claims and the exemptions against the header: an entry point nobody
claims fails it.

Figures (MI355X): torch.cuda._sleep runs at 0.42 ns per cycle; the gate is calibrated to DELAY_MS = 150 ms per case
(kernel_harness.calibrate_sleep, about 3.6e8 cycles).  Every proven case returned with the gate still pending, i.e.
in less than the delay; the two exempt cases take the delay itself (they wait for the gate).  The per-call
gate.query() is what tells that the delay sufficed, not these figures.  The whole file takes about 10 s, 7 s of it in
the gated cases, the slowest of them 0.6 s (the first, which loads the library); the test prints all three figures
(STREAM-ORDER lines)."""

import time

import pytest
import torch

import kernel_harness as kh
from kernel_harness import float_stack, gain, raw_movie, switches  # noqa: F401
from route_cases import CASES, E

DELAY_MS = 150.0

# The cases -- Case, CASES, ATOMIC_REL and their input helpers -- are tests/route_cases.py's, shared with
# tests/test_input_contract.py.

# ------------------------------------------------------------------ recorder over every module that binds `load`


@pytest.fixture
def rec(monkeypatch):
    from torch_motion_correction_amd import _lib, calibration, eer, mrc, tiff

    r = kh.GatedRecorder(_lib.load())
    for mod in (_lib, calibration, eer, mrc, tiff):
        monkeypatch.setattr(mod, "load", lambda: r)
    return r


@pytest.fixture(scope="module")
def cycles():
    """torch.cuda._sleep cycles for DELAY_MS, from one timing with two events."""
    with torch.cuda.device(torch.device("cuda:0")):
        per = kh.calibrate_sleep()
    c = kh.sleep_cycles_for(per, DELAY_MS)
    print(f"STREAM-ORDER gate: {per * 1e6:.3f} ns per cycle, {c} cycles for {DELAY_MS} ms")
    return c


@pytest.fixture(scope="module")
def timings():
    t = {}
    yield t
    if t:
        worst = max(t, key=lambda k: t[k][0])
        print(f"STREAM-ORDER slowest enqueue: {worst} {t[worst][0]:.1f} ms; total of the cases "
              f"{sum(v[1] for v in t.values()):.1f} s; slowest case {max(t, key=lambda k: t[k][1])} "
              f"{max(v[1] for v in t.values()):.2f} s")


# Entry points the gated run cannot prove, each with its reason: the entry point itself blocks the host by design
# before its launches.  Each still runs on S behind the gate in a case of route_cases.py, with its stream argument
# asserted to be S and its result compared; what is NOT shown for it is a launch on a stream that happens to be idle.
EXEMPT = {
    "mc_tiff_decode": "blocks: copies the strips' offset table from host memory with hipMemcpyWithStream ahead of its "
                      "kernels",
    "mc_eer_render": "blocks: copies the frames' offset table from host memory with hipMemcpyWithStream ahead of its "
                     "kernels",
}


# ------------------------------------------------------------------ coverage (no GPU)


def test_every_stream_taking_entry_point_is_claimed_or_exempt():
    """claims + exemptions == the entry points whose header declaration has a `stream` parameter, taken over
    _lib.SIGNATURES; no entry point is both; every exemption has its reason (the entry point blocks the host by design)
    and a case that runs it."""
    from torch_motion_correction_amd import _lib

    taking = kh.stream_entry_points(_lib.SIGNATURES)
    assert len(taking) >= 80 and "mc_abi_version" not in taking and "mc_xc_near_rows" not in taking
    claimed = {n for c in CASES for n in c.proves}
    ran_exempt = {n for c in CASES for n in c.after}
    assert not claimed & set(EXEMPT), sorted(claimed & set(EXEMPT))
    assert ran_exempt == set(EXEMPT), sorted(ran_exempt ^ set(EXEMPT))
    assert set(EXEMPT) == {"mc_tiff_decode", "mc_eer_render"}  # a new exemption is a decision, not an edit
    assert claimed | set(EXEMPT) == taking, (f"neither claimed nor exempt: {sorted(taking - claimed - set(EXEMPT))}; "
                                             f"no such entry point: {sorted((claimed | set(EXEMPT)) - taking)}")
    for name, why in EXEMPT.items():
        assert why.startswith("blocks: ") and len(why) > 40, name
    assert len({c.name for c in CASES}) == len(CASES)


# ------------------------------------------------------------------ the gated runs


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_entry_points_on_a_delayed_side_stream(dev, rec, cycles, timings, c):
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        inputs = c.make(dev)
        torch.cuda.synchronize()
        want = c.route(**inputs)
        torch.cuda.synchronize()
        _, got, S = kh.gated_run(c.route, inputs, rec, cycles, want=want)
    timings[c.name] = (rec.enqueue_ms, time.perf_counter() - t0)
    print(f"STREAM-ORDER {c.name}: pending {rec.pending()}; all {sorted(set(n for n, *_ in rec.log))}")
    if c.rel is None:
        kh.assert_same_bits(got, want, c.name)
    else:
        kh.assert_close_rel(got, want, c.rel, c.name)
    rec.streams_ok()  # every stream-taking call of the route, claimed or not
    rec.proven(*c.proves)
    rec.streams_ok(*c.after)


@pytest.mark.gpu
def test_negative_control_wrong_stream(dev, rec, cycles):
    """The method bites: mc_normalize behind the gate with ANOTHER stream as its stream argument reads the poisoned
    (allocated) twin at once and returns NaN; with S it matches.

    The wrong stream is a second side stream.  With the NULL stream as the argument the recorder refuses the call
    all the same (its stream argument is 0, not S), but what the output holds depends on the runtime: on the MI355X
    it came back NaN in one run and equal to the reference in another (there the null stream's launch, the first of
    the process, was ordered after S's pending work, and a wait for the null stream lasted as long as S's sleep).
    So a launch the C side itself put on stream 0 (a dropped `st`) is not certain to show in a result; the
    Python-visible stream argument is what is pinned.  Both outcomes of the null-stream launch are accepted below,
    and which one occurred is printed."""
    from torch_motion_correction_amd._lib import check, ptr

    with torch.cuda.device(dev):
        img = float_stack(3, 61, 67).to(dev)
        stats = torch.tensor([5.0, 0.5, 2.0], dtype=torch.float32, device=dev)
        want = E().normalize(img, stats)
        other = torch.cuda.Stream()
        torch.cuda.synchronize()

        def on(which):
            def route(img, stats):
                out = torch.empty_like(img)
                st = {"S": torch.cuda.current_stream().cuda_stream, "other": other.cuda_stream, "null": None}[which]
                check(rec.mc_normalize(ptr(img), ptr(out), img.numel(), ptr(stats), st), "mc_normalize")
                return out

            return route

        # the output is read after S is done: it was written once, from poison, while S slept
        for which in ("other", "null"):
            _, got, _ = kh.gated_run(on(which), dict(img=img, stats=stats), rec, cycles, want=want)
            torch.cuda.synchronize()
            assert len(rec.log) == 1 and rec.log[0][2:] == (True, True), rec.log  # called, returned: gate pending
            with pytest.raises(AssertionError, match="not on"):
                rec.streams_ok("mc_normalize")
            poisoned = bool(torch.isnan(got).all())
            print(f"STREAM-ORDER control on the {which} stream: output {'NaN' if poisoned else 'as the reference'}")
            if which == "other":
                assert poisoned, "a launch on another stream did not read the poisoned twin"
            else:
                assert rec.log[0][1] == 0
                assert poisoned or torch.equal(got, want)
        _, got, _ = kh.gated_run(on("S"), dict(img=img, stats=stats), rec, cycles, want=want)
        kh.assert_same_bits(got, want, "mc_normalize on S")
        rec.proven("mc_normalize")


# ------------------------------------------------------------------ the pipelines on a caller's side stream


def _results(results):
    return [x.clone() for r in results for x in (r.field, r.total, r.frames) if x is not None]


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "sequential"])
@pytest.mark.parametrize("kind", ["fp32", "raw"])
@pytest.mark.parametrize("n", [2, 3])
def test_pipelines_on_a_callers_side_stream(dev, rec, cycles, kind, overlap, n):
    """MoviePipeline.run / RawMoviePipeline.run with the caller's current stream S behind the gate and the movies
    copied over poisoned twins on S; the results are consumed by clone() on S right after run returns and equal the
    default-stream results bit for bit (whole-pixel shifts and a deterministic warp: the rule of test_rigid_routes).
    This pins deterministically that `start` is recorded on the CALLER's stream and that both pipeline streams wait
    for it: a pipeline stream that did not would read the twins while S sleeps.  It exercises the final
    caller.wait_event(done) too, but cannot make that wait fail deterministically: by the time the clones run on S
    the pipeline's own streams have usually finished.  (The pipelines launch on their own streams by design, so no
    stream argument is asserted here.)"""
    from torch_motion_correction_amd import pipeline

    with torch.cuda.device(dev):
        if kind == "fp32":
            movies = {f"m{i}": float_stack(3, 512, 512).to(dev) + float(i) for i in range(n)}

            def run(**m):
                return _results(pipeline.MoviePipeline(overlap=overlap).run(list(m.values())))
        else:
            movies = {f"m{i}": raw_movie(3, 512, 512, torch.uint8, 30 + i).to(dev) for i in range(n)}
            movies["g"] = gain(512, 512).to(dev)

            def run(g, **m):
                return _results(pipeline.RawMoviePipeline(gain=g, overlap=overlap).run(list(m.values())))

        want, got, _ = kh.gated_run(run, movies, rec, cycles)
        assert len(want) == 3 * n
        kh.assert_same_bits(got, want, f"{kind} pipeline, {n} movies, overlap={overlap}")


# ------------------------------------------------------------------ caches filled on one stream, read on another


@pytest.mark.gpu
def test_plan_cache_is_safe_to_read_from_another_stream(dev, cycles, switches):  # noqa: F811
    """plan.get_xc_plan builds mask, filter and chords with kernels on whichever stream is current at the first call
    and caches them; engine.mask_spectrum does the same with the plan's mhat.  Stream A: a NaN block filled and freed
    (the tables' fresh memory is poison), the gate, then estimate_global_motion (the first call for the key).  Stream
    B, which never waits for A: the same call at once.  B's field equals the default-stream field -- only if the
    builder finished its tables before publishing them.

    For A's call to return while A still sleeps without the fix, nothing else in it may block the host: the twiddle
    tables (a blocking copy from host memory) are put back after clear_plan_cache(), and the row chords are off,
    whose one-time check of the statistics box reads a flag back.  With either in place the unfixed code waits by
    accident, not by design."""
    import torch_motion_correction_amd as mc
    from torch_motion_correction_amd import plan

    engine, _ = switches
    engine.USE_ROW_CHORDS = False
    with torch.cuda.device(dev):
        img = float_stack(3, 512, 512).to(dev)
        kw = dict(pixel_spacing=1.0, reference_frame=1)
        want = mc.estimate_global_motion(img, **kw).clone()
        torch.cuda.synchronize()
        plan.clear_plan_cache()
        plan.get_twiddles(512, dev)
        torch.cuda.synchronize()
        A, B = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(A):
            block = torch.full((64 << 20,), float("nan"), dtype=torch.float32, device=dev)
            del block
            torch.cuda._sleep(cycles)
            a = mc.estimate_global_motion(img, **kw)
        with torch.cuda.stream(B):
            b = mc.estimate_global_motion(img, **kw).clone()
        torch.cuda.synchronize()
        kh.assert_same_bits(b, want, "stream B, cache filled on stream A")
        kh.assert_same_bits(a, want, "stream A")


@pytest.mark.gpu
def test_cached_tables_are_finished_before_they_are_stored(dev, cycles):
    """engine._cached: a builder that runs a device kernel on a sleeping stream.  When _cached returns, the stream has
    been waited for (the sleep ahead of the builder's kernels is over, and _cached returns from a wait for the whole
    stream), so any stream may read the entry; the second call finds it cached and waits for nothing."""
    from torch_motion_correction_amd import engine

    key = ("stream-order probe", str(dev))
    engine._CONST.pop(key, None)
    with torch.cuda.device(dev):
        A = torch.cuda.Stream()
        try:
            with torch.cuda.stream(A):
                torch.cuda._sleep(cycles)
                slept = torch.cuda.Event()
                slept.record(A)  # ahead of the builder's kernels on A, which runs in order
                built = engine._cached(key, lambda: (torch.arange(1000, device=dev, dtype=torch.int64) * 3, 7))
                assert slept.query(), "the table was stored while its builder was still queued behind the sleep"
                torch.cuda._sleep(cycles)
                gate = torch.cuda.Event()
                gate.record(A)
                again = engine._cached(key, lambda: 1 / 0)
                assert again is built and not gate.query(), "a cached entry waited for the stream"
            B = torch.cuda.Stream()
            with torch.cuda.stream(B):
                assert torch.equal(built[0].cpu(), torch.arange(1000) * 3)
            torch.cuda.synchronize()
        finally:
            engine._CONST.pop(key, None)
