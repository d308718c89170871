"""engine is ONE namespace over a module per kernel family: what a test or the benchmark assigns or replaces on the
package is what the family modules run.  Pinned without a GPU or the library:

(a) no family function binds a switch or the benchmark hook -- each reads it as an attribute of E, the package;
(b) engine._chunks follows engine.WORKSPACE_BYTES at call time;
(c) the five names tests replace (condition_movie, RawMovie, hot_list_capacity, _rows_forward, _raw_rows_forward)
    are reached through the package: by a call that ends in the replacement where the host gets that far before the
    library is loaded (condition_movie, RawMovie), else by the caller's bytecode (hot_list_capacity, _rows_forward,
    _raw_rows_forward: every caller loads the library first)."""

import dis
import importlib
import types

import pytest
import torch

import kernel_harness as kh
from kernel_harness import switches  # noqa: F401
from torch_motion_correction_amd import api, engine

FAMILIES = ("xc", "refine", "patches", "warps", "fourier", "raw", "condition")
MODULES = {name: importlib.import_module(f"torch_motion_correction_amd.engine.{name}") for name in FAMILIES}
REPLACED = ("condition_movie", "RawMovie", "hot_list_capacity", "_rows_forward", "_raw_rows_forward")


def codes(code):
    """The code object and those of everything nested in it (closures, lambdas, comprehensions)."""
    yield code
    for const in code.co_consts:
        if isinstance(const, types.CodeType):
            yield from codes(const)


def functions(module):
    """Every function object the module defines: its functions and the methods of its classes."""
    for obj in vars(module).values():
        if getattr(obj, "__module__", None) != module.__name__:
            continue
        if isinstance(obj, types.FunctionType):
            yield obj
        elif isinstance(obj, type):
            yield from (m for m in vars(obj).values() if isinstance(m, types.FunctionType))


def names_of(fn):
    return set().union(*(c.co_names for c in codes(fn.__code__)))


def readers(name):
    """(family, function) for every family function whose code names `name`."""
    return [(fam, fn) for fam, mod in MODULES.items() for fn in functions(mod) if name in names_of(fn)]


def assert_only_through_E(fn, name):
    """Every reference to `name` in `fn` (nested code included) is an attribute load whose object is the global E --
    never a global of the function's own module."""
    assert "E" in names_of(fn), f"{fn.__qualname__} names {name} without E"
    for code in codes(fn.__code__):
        prev = None
        for ins in dis.get_instructions(code):
            if ins.argval == name and ins.opname != "LOAD_CONST":
                assert ins.opname in ("LOAD_ATTR", "LOAD_METHOD"), f"{fn.__qualname__}: {ins.opname} {name}"
                assert prev is not None and prev.opname == "LOAD_GLOBAL" and prev.argval == "E", \
                    f"{fn.__qualname__}: {name} is an attribute of something other than E"
            prev = ins


def test_every_family_module_sees_the_package_as_E_and_is_re_exported_whole():
    for fam, mod in MODULES.items():
        assert mod.E is engine
        assert getattr(engine, fam) is mod  # no function of the namespace shadows a family module (hence warps.py)
        for name, obj in vars(mod).items():
            if getattr(obj, "__module__", None) == mod.__name__:  # defined there, not imported
                assert getattr(engine, name) is obj, f"engine.{name} is not {fam}.{name}"
    assert isinstance(engine.warp, types.FunctionType)


# ------------------------------------------------------------------ (a) switches and the hook


@pytest.mark.parametrize("name", kh.ENGINE_SWITCHES + ("RIGID_KERNEL_HOOK",))
def test_switches_and_the_hook_live_in_the_package_alone(name):
    assert name in vars(engine)
    for fam, mod in MODULES.items():
        assert name not in vars(mod), f"engine.{fam} has a {name} of its own"
    found = readers(name)
    for fam, fn in found:
        assert not hasattr(MODULES[fam], name)
        assert_only_through_E(fn, name)
    if name == "WORKSPACE_BYTES":  # its one reader is the chunker, in the package itself: (b)
        assert found == [] and name in engine._chunks.__code__.co_names and engine._chunks.__module__ == engine.__name__
    else:
        assert found, f"no family function reads {name}: the check above held for nothing"


# ------------------------------------------------------------------ (b) the chunker


def chunks_by_the_rule(workspace, n, item_bytes, most=None):
    chunk = max(1, min(n if most is None else min(n, most), workspace // item_bytes))
    return chunk, [(a, min(chunk, n - a)) for a in range(0, n, chunk)]


@pytest.mark.parametrize("n, item_bytes, most", [(7, 8, None), (7, 8, 2), (1, 8, None), (9, 24, None), (5, 64, 3)])
def test_chunks_follow_the_workspace_assigned_on_the_package(switches, n, item_bytes, most):  # noqa: F811
    eng, _ = switches
    assert eng is engine
    seen = []
    for workspace in (24, 50):
        eng.WORKSPACE_BYTES = workspace  # plainly, as the tests do
        got = eng._chunks(n, item_bytes, most)
        assert got == chunks_by_the_rule(workspace, n, item_bytes, most)
        first, count = got[1][-1]
        assert first + count == n and sum(c for _, c in got[1]) == n
        seen.append(got)
    if (n, item_bytes, most) == (7, 8, None):
        assert seen[0] == (3, [(0, 3), (3, 3), (6, 1)]) and seen[1] == (6, [(0, 6), (6, 1)])  # no stale binding


# ------------------------------------------------------------------ (c) the names tests replace


class Reached(Exception):
    """Raised by a replacement: the engine got to the name assigned on the package."""


def test_every_reference_to_a_replaced_name_goes_through_the_package():
    """The structural form, for all five names and every family function that names one: the name is loaded from E,
    and -- outside the module that defines it -- the function's module has no global of that name."""
    callers = {}
    for name in REPLACED:
        home = getattr(engine, name).__module__
        for fam, fn in readers(name):
            assert_only_through_E(fn, name)
            if MODULES[fam].__name__ != home:
                assert not hasattr(MODULES[fam], name), f"engine.{fam} binds {name}"
            callers.setdefault(name, set()).add(f"{fam}.{fn.__qualname__}")
    # the callers the suite's replacements rely on; condition_movie has none inside the engine (api.py calls it)
    assert "condition_movie" not in callers
    assert {"fourier.fast_shift_sums", "fourier.fourier_crop", "raw.corrected_sums", "raw.RawMovie.window"} \
        <= callers["RawMovie"]
    assert callers["hot_list_capacity"] == {"raw.RawMovie.__init__"}
    assert {"raw.warp_dose_weighted_sum_raw", "fourier.dose_weighted_sum", "fourier.warp_dose_weighted_sum",
            "fourier.fast_shift_sums", "fourier.fourier_crop"} <= callers["_rows_forward"]
    assert callers["_raw_rows_forward"] == {"fourier.fast_shift_sums", "fourier.fourier_crop"}
    assert engine._raw_rows_forward.__module__ == MODULES["raw"].__name__  # i.e. another family than its callers


def test_a_replaced_condition_movie_is_what_the_raw_routes_call(monkeypatch):
    seen = []

    def refuse(raw, *a, **kw):
        seen.append(raw.dtype)
        raise Reached

    assert engine.condition_movie is MODULES["condition"].condition_movie
    monkeypatch.setattr(engine, "condition_movie", refuse)
    with pytest.raises(Reached):
        api._raw_or_conditioned(torch.ones(2, 8, 8), None, True, None, lambda rm: rm, lambda img: img)
    assert seen == [torch.float32]


@pytest.mark.parametrize("call", [lambda src: engine.fast_shift_sums(src, torch.zeros(2, 2)),
                                  lambda src: engine.fourier_crop(src),
                                  lambda src: engine.corrected_sums(src, None, 1.0, True)],
                         ids=["fourier.fast_shift_sums", "fourier.fourier_crop", "raw.corrected_sums"])
def test_a_replaced_raw_movie_is_the_class_the_routes_test_against(monkeypatch, call):
    seen = []

    class Recorder(type):
        def __instancecheck__(cls, obj):
            seen.append(obj)
            raise Reached

    class FakeRawMovie(metaclass=Recorder):
        pass

    monkeypatch.setattr(engine, "RawMovie", FakeRawMovie)
    src = torch.zeros(2, 8, 8)
    with pytest.raises(Reached):
        call(src)
    assert len(seen) == 1 and seen[0] is src
