"""The two host-side rules every raw entry point and every chunked engine loop goes through, pinned without a GPU or
the library: api._raw_or_conditioned (which movies take the fused RawMovie route, what falls back to condition_movie
and with which arguments, whose hot counts come back) and engine._chunks (the WORKSPACE_BYTES rule)."""

import pytest
import torch

from torch_motion_correction_amd import api, engine
from torch_motion_correction_amd._lib import McorrError, McorrUnsupported

SHAPE = (2, 8, 8)
RM_COUNTS = torch.tensor([3, 4], dtype=torch.int32)
CM_COUNTS = torch.tensor([5, 6], dtype=torch.int32)


class Route:
    """Stand-ins for engine.RawMovie / engine.condition_movie and the two callbacks, with everything they were
    handed written down."""

    def __init__(self, monkeypatch, ctor_error=None, fused_error=None):
        self.log, self.built, self.condition_kwargs = [], [], None
        route = self

        class FakeRawMovie:
            def __init__(self, raw, gain, mean_zero=True, hot_pixel_threshold=None):
                route.built.append((raw.dtype, mean_zero, hot_pixel_threshold))
                if ctor_error is not None:
                    raise ctor_error
                self.hot_counts = RM_COUNTS if hot_pixel_threshold is not None else None

        def condition_movie(raw, gain=None, mean_zero=True, hot_pixel_threshold=None, return_hot_counts=False):
            self.condition_kwargs = dict(mean_zero=mean_zero, hot_pixel_threshold=hot_pixel_threshold,
                                         return_hot_counts=return_hot_counts)
            img = raw.to(torch.float32)
            return (img, CM_COUNTS) if return_hot_counts else img

        monkeypatch.setattr(engine, "RawMovie", FakeRawMovie)
        monkeypatch.setattr(engine, "condition_movie", condition_movie)
        self.fused_error = fused_error

    def fused(self, rm):
        self.log.append("fused")
        if self.fused_error is not None:
            raise self.fused_error
        return ("fused", rm)

    def conditioned(self, img):
        self.log.append("conditioned")
        assert isinstance(img, torch.Tensor) and img.dtype == torch.float32 and tuple(img.shape) == SHAPE
        return ("conditioned", img)

    def run(self, dtype, thr=None, **kw):
        raw = torch.ones(SHAPE).to(dtype)
        return api._raw_or_conditioned(raw, None, True, thr, self.fused, self.conditioned, **kw)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
@pytest.mark.parametrize("thr", [None, 10.0])
def test_integer_movies_take_the_fused_route_with_the_raw_movies_counts(monkeypatch, dtype, thr):
    r = Route(monkeypatch)
    (tag, rm), counts = r.run(dtype, thr)
    assert tag == "fused" and r.log == ["fused"]
    assert r.built == [(dtype, True, thr)]
    assert r.condition_kwargs is None
    assert counts is rm.hot_counts
    assert (counts is None) if thr is None else (counts is RM_COUNTS)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("thr", [None, 10.0])
def test_float_movies_are_conditioned_without_a_raw_movie(monkeypatch, dtype, thr):
    r = Route(monkeypatch)
    (tag, _), counts = r.run(dtype, thr)
    assert tag == "conditioned" and r.log == ["conditioned"]
    assert r.built == []
    assert r.condition_kwargs == dict(mean_zero=True, hot_pixel_threshold=thr, return_hot_counts=thr is not None)
    assert (counts is None) if thr is None else (counts is CM_COUNTS)


@pytest.mark.parametrize("where", ["constructor", "fused"])
@pytest.mark.parametrize("thr", [None, 10.0])
def test_unsupported_falls_through_to_the_conditioned_route(monkeypatch, where, thr):
    err = McorrUnsupported("no fused kernel")
    r = Route(monkeypatch, **({"ctor_error": err} if where == "constructor" else {"fused_error": err}))
    (tag, _), counts = r.run(torch.uint8, thr)
    assert tag == "conditioned"
    assert r.log == (["conditioned"] if where == "constructor" else ["fused", "conditioned"])
    assert len(r.built) == 1
    # the counts are asked for exactly when a threshold is set, and they are condition_movie's
    assert r.condition_kwargs["return_hot_counts"] is (thr is not None)
    assert r.condition_kwargs["hot_pixel_threshold"] == thr
    assert (counts is None) if thr is None else (counts is CM_COUNTS)


@pytest.mark.parametrize("err", [ValueError("bad argument"), McorrError("a kernel failed")],
                         ids=["ValueError", "McorrError"])
def test_any_other_error_inside_fused_propagates(monkeypatch, err):
    assert not isinstance(err, McorrUnsupported)
    r = Route(monkeypatch, fused_error=err)
    with pytest.raises(type(err)) as got:
        r.run(torch.int16, 10.0)
    assert got.value is err
    assert r.log == ["fused"] and r.condition_kwargs is None


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.float32])
def test_allow_fused_false_never_builds_a_raw_movie(monkeypatch, dtype):
    r = Route(monkeypatch)
    (tag, _), counts = r.run(dtype, 10.0, allow_fused=False)
    assert tag == "conditioned" and r.log == ["conditioned"]
    assert r.built == []
    assert counts is CM_COUNTS


def test_hot_counts_out():
    out = api._hot_counts_out(None, 3, torch.device("cpu"))
    assert out.dtype == torch.int32 and out.tolist() == [0, 0, 0]
    assert api._hot_counts_out(CM_COUNTS, 2, torch.device("cpu")).tolist() == [5, 6]


@pytest.mark.parametrize("n, item_bytes, workspace, chunk, spans", [
    (5, 8, 16, 2, [(0, 2), (2, 2), (4, 1)]),
    (5, 8, 7, 1, [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1)]),
    (1, 8, 1 << 30, 1, [(0, 1)]),
    (4, 8, 32, 4, [(0, 4)]),
])
def test_chunks(monkeypatch, n, item_bytes, workspace, chunk, spans):
    monkeypatch.setattr(engine, "WORKSPACE_BYTES", workspace)  # read at call time
    assert engine._chunks(n, item_bytes) == (chunk, spans)
