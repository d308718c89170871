"""tests/kernel_harness.py on the CPU: what "this entry point ran", "the header and the ctypes table agree", "the host
program passed under the sanitizers", "nothing was written outside the buffer" and "the same inputs as before" mean,
pinned once for every test that imports them."""

import pytest
import torch

import kernel_harness as kh
from kernel_harness import nan_empty, switches  # noqa: F401

CPU = torch.device("cpu")


# ------------------------------------------------------------------ Recorder


class _FakeLib:
    def mc_a(self, *a):
        return ("a", a)

    def mc_b(self, *a):
        return ("b", a)


def test_recorder_records_calls_not_lookups():
    rec = kh.Recorder(_FakeLib())
    fn = rec.mc_a  # looked up, never called
    assert rec.names == [] and rec.args == {} and rec.count("mc_a") == 0
    with pytest.raises(AssertionError, match="mc_a did not run"):
        rec.ran("mc_a")
    rec.ran(absent=("mc_a", "mc_b"))
    assert fn(1, "x") == ("a", (1, "x"))  # the call goes through, with its arguments, and is written down
    assert rec.mc_b(2) == ("b", (2,)) and rec.mc_a() == ("a", ())
    assert rec.names == ["mc_a", "mc_b", "mc_a"]
    assert rec.args == {"mc_a": [(1, "x"), ()], "mc_b": [(2,)]}
    assert rec.count("mc_a") == 2 and rec.count("mc_b") == 1 and rec.count("mc_c") == 0
    with pytest.raises(AttributeError):
        rec.mc_c  # a missing entry point stays an error
    assert rec._lib.mc_a(3) == ("a", (3,)) and rec.count("mc_a") == 2  # the library itself is not recorded


def test_recorder_ran_absent_only_and_clear():
    rec = kh.Recorder(_FakeLib())
    rec.mc_a(1)
    rec.mc_a(2)
    rec.ran("mc_a", absent=("mc_b",))
    rec.only("mc_a", 2)
    with pytest.raises(AssertionError, match="mc_b did not run"):
        rec.ran("mc_a", "mc_b")
    with pytest.raises(AssertionError, match="mc_a ran"):
        rec.ran(absent=("mc_a",))
    with pytest.raises(AssertionError, match="expected 1 x mc_a"):
        rec.only("mc_a", 1)
    rec.mc_b()
    with pytest.raises(AssertionError, match="expected 2 x mc_a"):
        rec.only("mc_a", 2)  # another entry point ran too
    rec.clear()
    assert rec.names == [] and rec.args == {} and rec.count("mc_a") == 0
    rec.only("mc_a", 0)
    rec.ran(absent=("mc_a", "mc_b"))


# ------------------------------------------------------------------ NaN-guarded buffers


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_nan_buffer_alignment_and_guards(offset):
    shape = (3, 5, 7)
    view, flat = kh.nan_buffer(shape, CPU, offset)
    n = 3 * 5 * 7
    lead = (view.data_ptr() - flat.data_ptr()) // 4
    assert tuple(view.shape) == shape and view.dtype == torch.float32 and view.is_contiguous()
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * offset
    assert lead >= kh.GUARD and flat.numel() - lead - n >= kh.GUARD and kh.GUARD >= 8
    assert bool(torch.isnan(flat).all())
    kh.assert_guards(view, flat, "untouched")
    view.fill_(1.0)  # writing all of the buffer, and nothing else, passes
    kh.assert_guards(view, flat, "filled")
    for at in (lead - 1, lead + n):  # one element before the view, one element past it
        saved = flat[at].clone()
        flat[at] = 0.0
        with pytest.raises(AssertionError, match="wrote outside its output buffer"):
            kh.assert_guards(view, flat, "one write")
        flat[at] = saved
    kh.assert_guards(view, flat, "restored")


@pytest.mark.parametrize("past", [0, 1, 3, 6, 12, 16, 17])
@pytest.mark.parametrize("nbytes", [1, 5, 64, 210])
def test_byte_buffer_alignment_and_guards(past, nbytes):
    view, whole = kh.byte_buffer(nbytes, CPU, past)
    lead = view.data_ptr() - whole.data_ptr()
    assert view.dtype == whole.dtype == torch.uint8 and view.shape == (nbytes,) and view.is_contiguous()
    assert whole.data_ptr() % 16 == 0 and view.data_ptr() % 16 == past % 16 and whole.numel() % 4 == 0
    assert lead >= 4 * kh.GUARD and whole.numel() - lead - nbytes >= 4 * kh.GUARD
    assert bool(torch.isnan(whole.view(torch.float32)).all())
    kh.assert_byte_guards(view, whole, "untouched")
    view.fill_(0)  # writing all of the buffer, and nothing else, passes
    kh.assert_byte_guards(view, whole, "filled")
    for at in (lead - 1, lead + nbytes, 0, whole.numel() - 1):  # the bytes next to the view, the allocation's ends
        saved = int(whole[at])
        whole[at] = saved ^ 1
        with pytest.raises(AssertionError, match="one write: wrote outside its buffer"):
            kh.assert_byte_guards(view, whole, "one write")
        whole[at] = saved
    kh.assert_byte_guards(view, whole, "restored")


def test_byte_buffer_typed_views():
    """A typed output is a view of the bytes; the guard check takes it as it is."""
    for dtype in (torch.int16, torch.float16, torch.float32):
        size = dtype.itemsize
        view, whole = kh.byte_buffer(3 * 5 * size, CPU, past=3 * size)
        out = view.view(dtype).view(3, 5)
        assert out.data_ptr() == view.data_ptr() and out.data_ptr() % size == 0 and out.data_ptr() % 16 == 3 * size
        out.fill_(1)
        kh.assert_byte_guards(out, whole, "typed")
        whole[out.data_ptr() - whole.data_ptr() + out.numel() * size] ^= 1
        with pytest.raises(AssertionError, match="wrote outside its buffer"):
            kh.assert_byte_guards(out, whole, "typed")


# ------------------------------------------------------------------ the header against the ctypes table

SYNTHETIC = """/* int mc_in_a_comment(int a); */
// int mc_in_a_line_comment(int a);
int mc_other(int a);  // one int
int mc_nothing(void);
int mc_made_up(const unsigned char* data, long long n,
    int h, unsigned seed, float x /* host */, int64_t m, double d,
    long long* out /* host */, const int64_t* off, const double m4[4], const mc_xc_geom* geom, void* stream);
int mc_odd(int a, size_t n);
"""


def test_header_signature():
    import ctypes as C

    from torch_motion_correction_amd import _lib

    assert kh.declared_entry_points(SYNTHETIC) == {"mc_other", "mc_nothing", "mc_made_up", "mc_odd"}
    assert kh.header_parameters("mc_made_up", SYNTHETIC) == [
        "const unsigned char* data", "long long n", "int h", "unsigned seed", "float x", "int64_t m", "double d",
        "long long* out", "const int64_t* off", "const double m4[4]", "const mc_xc_geom* geom", "void* stream"]
    vp = C.c_void_p
    assert kh.header_signature("mc_made_up", SYNTHETIC) == [
        vp, C.c_int64, C.c_int, C.c_uint, C.c_float, C.c_int64, C.c_double, vp, vp, vp, vp, vp]
    spelt_out = [vp, C.c_int64, C.c_int, C.c_uint, C.c_float, C.c_int64, C.c_double, C.POINTER(C.c_int64),
                 C.POINTER(C.c_int64), C.POINTER(C.c_double), _lib.GP, vp]
    assert kh.binding_disagreement("mc_made_up", spelt_out, SYNTHETIC) is None
    assert "parameter 0" in kh.binding_disagreement("mc_made_up", [C.POINTER(C.c_int64)] + spelt_out[1:], SYNTHETIC)
    assert kh.header_signature("mc_other", SYNTHETIC) == [C.c_int] and kh.header_signature("mc_nothing", SYNTHETIC) == []
    for absent in ("mc_absent", "mc_in_a_comment", "mc_in_a_line_comment"):
        with pytest.raises(KeyError):
            kh.header_signature(absent, SYNTHETIC)
    with pytest.raises(ValueError, match="size_t n"):
        kh.header_signature("mc_odd", SYNTHETIC)  # an unknown base type is no int


def test_every_declared_entry_point_is_bound_as_declared():
    from torch_motion_correction_amd import _lib

    declared = kh.declared_entry_points()
    assert declared == set(_lib.SIGNATURES) and len(declared) >= 89
    for name in sorted(declared):
        kh.assert_entry_point(name)
    for name in ("mc_eer_render", "mc_tiff_decode", "mc_tiff_encode", "mc_tiff_pack", "mc_mrc_decode", "mc_raw_orient"):
        assert kh.header_signature(name) == _lib.SIGNATURES[name]  # these bind every pointer as void*
    swapped = [_lib.GP if a is _lib.LP else a for a in _lib.SIGNATURES["mc_xcg_cols_forward"]]
    assert "parameter 3: the header says a pointer to XcLine" in kh.binding_disagreement("mc_xcg_cols_forward", swapped)
    with pytest.raises(AssertionError, match="not declared"):
        kh.assert_entry_point("mc_absent")


def test_assert_entry_point_refuses_a_binding_that_disagrees():
    import ctypes as C

    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    header = "int mc_t(const void* src, int n, float x, long long* out /* host */, void* stream);\n"
    good = [vp, i32, f32, C.POINTER(i64), vp]
    kh.assert_entry_point("mc_t", good, header=header, signatures={"mc_t": good})
    kh.assert_entry_point("mc_t", header=header, signatures={"mc_t": [vp, i32, f32, vp, vp]})  # a pointer as void*
    for bad, why in (([vp, i32, f32, C.POINTER(i64)], "5 parameters, the binding 4"),
                     ([vp, i32, i32, C.POINTER(i64), vp], "parameter 2: the header says c_float, the binding c_int"),
                     ([vp, i32, f32, C.POINTER(C.c_double), vp], "parameter 3: the header says a pointer to c_long"),
                     ([vp, i32, f32, i64, vp], "parameter 3"),  # a scalar for a pointer
                     ([vp, vp, f32, vp, vp], "parameter 1")):   # a pointer for a scalar
        with pytest.raises(AssertionError, match=why):
            kh.assert_entry_point("mc_t", header=header, signatures={"mc_t": bad})
    with pytest.raises(AssertionError, match="not bound"):
        kh.assert_entry_point("mc_t", header=header, signatures={})
    with pytest.raises(AssertionError, match="bound as"):
        kh.assert_entry_point("mc_t", [vp, i32, f32, vp, vp], header=header, signatures={"mc_t": good})
    with pytest.raises(AssertionError):
        kh.assert_entry_point("mc_abi_version", source=("no_such.hip", "no_such", []))


# ------------------------------------------------------------------ host programs

PROGRAM = """#include <cstdio>
int main(int argc, char** argv) {
  int* a = new int[4]();
  volatile int at = %d;
  int v = a[at];
  %s
  std::printf("%%d arguments OK\\n", argc - 1 + v);
  delete[] a;
  return 0;
}
"""


def test_run_host_program(tmp_path):
    def source(name, at, line=""):
        (tmp_path / name).write_text(PROGRAM % (at, line))
        return str(tmp_path / name)

    for sanitize in (True, False):
        res = kh.run_host_program(source("fine.cpp", 3), tmp_path, "a", 2, sanitize=sanitize)
        assert res.returncode == 0 and res.stdout == "2 arguments OK\n"
    with pytest.raises(AssertionError):
        kh.run_host_program(source("fails.cpp", 3, 'std::printf("case 1: FAIL\\n");'), tmp_path)
    with pytest.raises(AssertionError):
        kh.run_host_program(source("no_ok.cpp", 3, 'std::printf("OK\\n"); return 3;'), tmp_path)
    with pytest.raises(AssertionError, match="heap-buffer-overflow"):
        kh.run_host_program(source("past.cpp", 4), tmp_path)  # one int past new int[4]: the flags are in effect


def test_nan_and_nan_empty(nan_empty):
    assert bool(torch.isnan(kh.nan((2, 3), CPU)).all()) and kh.nan((2, 3), CPU).dtype == torch.float32
    assert bool(torch.isnan(torch.empty(4, 5)).all()) and bool(torch.isnan(torch.empty((3,), dtype=torch.float64)).all())
    assert torch.empty(6, dtype=torch.int32).dtype == torch.int32  # integer buffers are handed out as they are


# ------------------------------------------------------------------ inputs: the values every kernel test has seen so far

# Recorded from the functions of tests/test_rigid_kernels_float64.py before they moved here: (sum, first row of frame 0).
RAW_2x8x16 = {
    torch.uint8: (7844, [44, 17, 47, 43, 49, 17, 16, 37, 10, 50, 33, 34, 14, 36, 39, 38]),
    torch.int16: (37168, [252, 36, 273, 245, 289, 38, 30, 193, -16, 302, 167, 170, 12, 187, 215, 206]),
}
GAIN_8x16_ROW0 = ["0x1.ee46b60000000p+1", "0x1.1114c40000000p+1", "0x1.053e3c0000000p-1", "0x1.37c8c60000000p-2",
                  "0x1.6a49ce0000000p+1", "0x1.1e0dd20000000p-1", "0x1.aeca2a0000000p+1", "0x1.9c5ab20000000p-1",
                  "0x1.7a6e3c0000000p-1", "0x1.b2d9860000000p-1", "0x1.e2f79c0000000p-2", "0x1.3c2fe00000000p-1",
                  "0x1.1f78520000000p+0", "0x1.9a48700000000p-1", "0x1.43a7940000000p-1", "0x1.de7f040000000p+1"]
GAIN_8x16_SUM = float.fromhex("0x1.67a0204900000p+7")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["uint8", "int16"])
def test_raw_movie_is_the_recorded_one(dtype):
    total, row = RAW_2x8x16[dtype]
    raw = kh.raw_movie(2, 8, 16, dtype, 5)
    assert raw.dtype == dtype and tuple(raw.shape) == (2, 8, 16)
    assert int(raw.long().sum()) == total and raw[0, 0].tolist() == row
    # the static recipe is the drifting one at zero drift without a margin; a drift crops the same texture
    assert torch.equal(raw, kh.drifting_raw_movie([0, 0], [0, 0], 8, 16, dtype, 5, pad=0))
    assert not torch.equal(kh.drifting_raw_movie([0, 0], [0, 0], 8, 16, dtype, 5, pad=4), raw)
    if dtype == torch.int16:
        assert int(raw.min()) < 0  # negative counts occur


def test_gain_is_the_recorded_one():
    g = kh.gain(8, 16)
    assert g.dtype == torch.float32 and tuple(g.shape) == (8, 16)
    assert [float(v).hex() for v in g[0]] == GAIN_8x16_ROW0
    # 4 ** x differs in the last bit of a few elements between the scalar and the vector code of the CPU library: the
    # sum over all 128 is held to 128 such bits of its largest element, 4 (a different seed moves it by O(10))
    assert abs(float(g.double().sum()) - GAIN_8x16_SUM) <= 128 * 2.0 ** -22
    assert float(g.min()) >= 0.25 and float(g.max()) <= 4.0 and float(g.max() / g.min()) > 8
    assert torch.equal(kh.gain(8, 16, seed=9), g) and not torch.equal(kh.gain(8, 16, seed=10), g)


def test_gain_refuses_a_small_dynamic_range(monkeypatch):
    monkeypatch.setattr(torch, "rand", lambda h, w, generator=None: torch.full((h, w), 0.5))
    with pytest.raises(AssertionError):
        kh.gain(8, 16)


def test_float_stack_and_offset_copy():
    a = kh.float_stack(2, 5, 8)
    g = torch.Generator().manual_seed(2 * 7919 + 5 * 31 + 8)
    assert torch.equal(a, torch.randn(2, 5, 8, generator=g) * 2 + 5) and not bool((a == 0).any())
    assert torch.equal(kh.float_stack(2, 5, 8, torch.float16), a.half())
    for src, size in ((a, 4), (a.half(), 2)):
        for offset in (0, 1, 3):
            view = kh.offset_copy(src, offset)
            assert torch.equal(view, src) and view.data_ptr() % 16 == size * offset


def test_rel_err_and_assert_sum():
    import numpy as np

    want, bound = np.full((2, 3), 2.0), np.full((2, 3), 0.5)
    got = torch.full((2, 3), 2.0)
    got[0, 1], got[1, 2] = 2.25, 1.75
    assert kh.rel_err(got, torch.from_numpy(want)) == 0.125
    assert kh.assert_sum(got, want, bound, "sum") == 0.5
    border = np.zeros((2, 3), dtype=bool)
    border[0, 1] = border[1, 2] = True
    assert kh.assert_sum(got, want, bound, "sum", border) == 0.0
    got[1, 0] = 2.75
    with pytest.raises(AssertionError, match=r"1 pixels of the sum beyond the bound, first \(row, col\) \[\(1, 0\)\]"):
        kh.assert_sum(got, want, bound, "sum", border | True)  # the border only leaves pixels out of the ratio


# ------------------------------------------------------------------ ratios


def test_worse_keeps_the_maximum_and_returns_the_value():
    r = {}
    assert kh.worse(r, "k", 0.25) == 0.25 and kh.worse(r, "k", 0.125) == 0.125 and kh.worse(r, "a b", 1.0) == 1.0
    assert r == {"k": 0.25, "a b": 1.0}
    assert kh.ratio_lines(r) == ["RATIO a b: 1.000", "RATIO k: 0.250"]
    assert kh.ratio_lines(r, "RATIO fp32 stand-in") == ["RATIO fp32 stand-in a b: 1.000", "RATIO fp32 stand-in k: 0.250"]


ratios = kh.ratios_fixture("RATIO harness")


@pytest.mark.parametrize("visit", [0, 1])
def test_ratios_fixture_hands_out_one_dict_per_module(ratios, visit):
    before, value = ratios.get("seen", 0.0), 1.0 - visit / 2
    assert kh.worse(ratios, "seen", value) == value and ratios == {"seen": max(before, value)}


# ------------------------------------------------------------------ switches


def _switch_values():
    from torch_motion_correction_amd import engine, plan

    return {**{n: getattr(engine, n) for n in kh.ENGINE_SWITCHES}, "USE_DIRECT_LINES": plan.USE_DIRECT_LINES}


@pytest.fixture
def former():
    """Set up before `switches`, torn down after it: the values before the test against the values after."""
    before = _switch_values()
    yield before
    from torch_motion_correction_amd import plan

    assert _switch_values() == before and plan._LINES == {}


def test_switches_restores_every_switch_assigned_in_the_body(former, switches):
    engine, plan = switches
    assert set(former) == {"FUSED_SEARCH", "USE_ROW_CHORDS", "WORKSPACE_BYTES", "FULL_ROW_MAJOR", "DOSE_COLUMN_MAJOR",
                           "POLYPHASE_FOURIER_SHIFT", "USE_DIRECT_LINES"}
    assert plan._LINES == {}
    for name in kh.ENGINE_SWITCHES:
        value = getattr(engine, name)
        setattr(engine, name, value + 12345 if name == "WORKSPACE_BYTES" else not value)  # plainly, as the tests do
    plan.USE_DIRECT_LINES = not plan.USE_DIRECT_LINES
    plan._LINES["stale"] = None
    assert all(_switch_values()[k] != v for k, v in former.items())



# ------------------------------------------------------------------ stream ordering: the delayed-producer tools

_HEADER = """
/* a comment with void* stream in it */
int mc_a(const float* x, int n, void* stream);
int mc_b(int n);
int mc_c(void* stream, int n);  // the stream need not come last
"""


class _Gate:
    """An event whose query() answers True (the sleep has ended) from the `opens`-th question on."""

    def __init__(self, opens):
        self.asked, self.opens = 0, opens

    def query(self):
        self.asked += 1
        return self.asked > self.opens


def test_stream_parameter_and_stream_entry_points():
    assert kh.stream_parameter("mc_a", _HEADER) == 2 and kh.stream_parameter("mc_b", _HEADER) is None
    assert kh.stream_parameter("mc_c", _HEADER) == 0
    assert kh.stream_entry_points(["mc_a", "mc_b", "mc_c"], _HEADER) == {"mc_a", "mc_c"}
    with pytest.raises(KeyError):
        kh.stream_parameter("mc_d", _HEADER)
    taking = kh.stream_entry_points()  # the committed header over _lib.SIGNATURES
    assert {"mc_normalize", "mc_tiff_decode", "mc_xc_rows_forward"} <= taking
    assert not taking & {"mc_abi_version", "mc_xc_near_rows", "mc_warp_scratch_bytes", "mc_local_loss_tiles"}


def test_poisoned_twins():
    f = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    u = torch.tensor([0, 1, 254, 255], dtype=torch.uint8)
    i = torch.tensor([-32768, -1, 0, 5], dtype=torch.int16)
    idx = torch.tensor([3, 1, 2], dtype=torch.int64)
    assert bool(torch.isnan(kh.poisoned(f)).all()) and kh.poisoned(f).shape == f.shape
    assert kh.poisoned(u).tolist() == [255, 254, 1, 0] and kh.poisoned(i).tolist() == [32767, 0, -1, -6]
    assert torch.equal(kh.poisoned(idx), idx) and kh.poisoned(idx).data_ptr() != idx.data_ptr()  # an index table
    assert kh.poisoned(f.half()).dtype == torch.float16

    class Movie:
        pass

    m = Movie()
    m.raw, m.mu, m.kind, m.nothing = u, f, 0, None
    twins, pairs = kh.poisoned_twins(dict(x=f, m=m, n=7, none=None, name="catmull_rom"))
    assert twins["n"] == 7 and twins["none"] is None and twins["name"] == "catmull_rom"
    assert twins["m"] is not m and twins["m"].kind == 0 and twins["m"].nothing is None
    assert twins["m"].raw.tolist() == [255, 254, 1, 0] and bool(torch.isnan(twins["m"].mu).all())
    assert m.raw is u and m.mu is f and u.tolist() == [0, 1, 254, 255]  # the true inputs are untouched
    assert len(pairs) == 3
    m.frames = [u]  # a tensor in a container would be shared with the true input, unpoisoned
    with pytest.raises(AssertionError, match="Movie.frames holds tensors in a container"):
        kh.poisoned_twins(dict(m=m))
    m.frames = {"a": (1, [f])}
    with pytest.raises(AssertionError, match="Movie.frames holds tensors"):
        kh.poisoned_twins(dict(m=m))
    m.frames = [1, 2, (3, "x")]  # plain values in containers are shared, as every non-tensor is
    assert len(kh.poisoned_twins(dict(m=m))[1]) == 2
    for twin, true in pairs:  # what gated_run enqueues behind the gate
        twin.copy_(true)
    assert torch.equal(twins["x"], f) and torch.equal(twins["m"].raw, u) and torch.equal(twins["m"].mu, f)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bool, torch.int16, torch.float16, torch.int32, torch.float32,
                                   torch.int64, torch.float64, torch.complex64], ids=str)
@pytest.mark.parametrize("shape", [(1,), (3, 5, 7), (2, 16), (0,)], ids=str)
def test_relocated_starts_one_element_past_a_boundary(dtype, shape):
    n = 1
    for s in shape:
        n *= s
    x = torch.arange(n) % 120 + 1
    x = (x % 2 == 1).view(shape) if dtype == torch.bool else x.to(dtype).view(shape)
    size = x.element_size()
    if n == 0:  # nothing to start anywhere
        y = kh.relocated(x)
        assert y.dtype == dtype and y.shape == x.shape and y is not x
        return
    for lead in (16, 48):
        y = kh.relocated(x, lead)
        assert y.dtype == dtype and y.shape == x.shape and y.is_contiguous() and y.data_ptr() != x.data_ptr()
        assert y.data_ptr() % 16 == size  # one element past a boundary, never on one
        kh.assert_same_bits(y, x, "relocated")
        whole = y.untyped_storage()
        first, total = y.data_ptr() - whole.data_ptr(), whole.nbytes()
        assert whole.data_ptr() % 16 == 0 and first == lead + size  # `lead` bytes of whole pieces, then the element
        behind = total - first - n * size
        assert 16 <= behind < 48 and total % 16 == 0  # the rest of the last piece and one whole piece more
        assert (first + n * size + 15) // 16 * 16 + 16 == total
        pad = torch.empty(0, dtype=torch.uint8).set_(whole)
        assert bool((pad[:first] == 255).all()) and bool((pad[first + n * size:] == 255).all())  # all-ones padding
        if dtype.is_floating_point:  # what a load at the next lower boundary reads first: NaN
            assert bool(torch.isnan(pad[lead:lead + size].view(dtype)).all())
    y.view(torch.uint8).zero_() if dtype != torch.bool else y.zero_()
    assert bool((x.view(torch.uint8) if dtype != torch.bool else x).any())  # a copy: the source is left alone
    for bad in (0, 8, 20):
        with pytest.raises(AssertionError):
            kh.relocated(x, bad)


def test_relocated_of_a_view_and_of_a_gradient_leaf():
    base = torch.arange(24, dtype=torch.float32).view(4, 6)
    y = kh.relocated(base.t())  # not contiguous: the copy is, in the view's own order
    assert y.is_contiguous() and torch.equal(y, base.t()) and y.data_ptr() % 16 == 4
    leaf = base.clone().requires_grad_()
    assert not kh.relocated(leaf).requires_grad and torch.equal(kh.relocated(leaf), base)


def test_twins_applies_fn_to_every_tensor():
    f = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    u = torch.tensor([0, 1, 254, 255], dtype=torch.uint8)

    class Movie:
        pass

    m = Movie()
    m.raw, m.mu, m.kind, m.nothing = u, f, 0, None
    inputs = dict(x=f, m=m, n=7, none=None, name="catmull_rom", shape=(2, 3))
    seen = []

    def fn(x):
        seen.append(x)
        return kh.relocated(x)

    out, pairs = kh.twins(inputs, fn)
    assert [id(x) for x in seen] == [id(f), id(f), id(u)]  # x, then m's attributes in sorted order: mu, raw
    assert out["n"] == 7 and out["none"] is None and out["name"] == "catmull_rom" and out["shape"] == (2, 3)
    assert out["m"] is not m and type(out["m"]) is Movie and out["m"].kind == 0 and out["m"].nothing is None
    assert m.raw is u and m.mu is f  # the true object keeps its tensors
    assert [(a.data_ptr() % 16, b.data_ptr() == t.data_ptr()) for (a, b), t in zip(pairs, (f, f, u))] == \
        [(4, True), (4, True), (1, True)]
    assert pairs[0][0] is out["x"] and pairs[1][0] is out["m"].mu and pairs[2][0] is out["m"].raw
    assert torch.equal(out["x"], f) and torch.equal(out["m"].raw, u) and torch.equal(out["m"].mu, f)
    # poisoned_twins is twins with poisoned, pair for pair
    a, ap = kh.poisoned_twins(inputs)
    b, bp = kh.twins(inputs, kh.poisoned)
    assert len(ap) == len(bp) == 3 and all(x[1] is y[1] for x, y in zip(ap, bp))
    kh.assert_same_bits([x for x, _ in ap], [x for x, _ in bp], "poisoned twins")
    assert a.keys() == b.keys() == inputs.keys()
    m.frames = [u]  # the container assertion stays, whatever fn is
    with pytest.raises(AssertionError, match="Movie.frames holds tensors in a container"):
        kh.twins(dict(m=m), kh.relocated)
    assert kh.twins(dict(n=3, s="x"), lambda x: 1 / 0) == (dict(n=3, s="x"), [])  # no tensor: fn is never called


def test_snapshot_and_assert_inputs_unchanged():
    class Movie:
        pass

    m = Movie()
    m.raw, m.mu, m.kind = torch.tensor([0, 1, 254, 255], dtype=torch.uint8), torch.tensor([1.0, float("nan")]), 0
    idx = torch.tensor([3, 1, 2], dtype=torch.int64)
    z = torch.tensor([0.0, -0.0])
    inputs = dict(m=m, idx=idx, z=z, n=7, none=None)
    snap = kh.snapshot(inputs)
    assert [label for label, _, _ in snap] == ["m.mu", "m.raw", "idx", "z"]
    assert all(x is y for (_, x, _), y in zip(snap, (m.mu, m.raw, idx, z)))
    assert all(c.data_ptr() != x.data_ptr() and c.device.type == "cpu" for _, x, c in snap)
    kh.assert_inputs_unchanged(inputs, snap, "untouched")  # NaN included: bits are compared
    z[0] = -0.0  # equal as a number, another bit pattern
    with pytest.raises(AssertionError, match="case: the input z was written to"):
        kh.assert_inputs_unchanged(inputs, snap, "case")
    kh.assert_inputs_unchanged({k: v for k, v in inputs.items() if k != "z"}, snap, "the others")  # named inputs only
    z[0] = 0.0
    m.raw[2] = 253  # a tensor an object holds
    with pytest.raises(AssertionError, match=r"case: the input m.raw was written to:\[0\]: 1 of 4 elements differ"):
        kh.assert_inputs_unchanged(inputs, snap, "case")
    m.raw[2] = 254
    kh.assert_inputs_unchanged(inputs, snap, "restored")
    kept, m.mu = m.mu, m.mu.clone()  # rebound to an equal tensor: no longer the caller's
    with pytest.raises(AssertionError, match="the input m.mu was replaced by another tensor"):
        kh.assert_inputs_unchanged(inputs, snap, "case")
    m.mu = kept
    kh.assert_inputs_unchanged(inputs, snap, "restored")
    assert kh.snapshot(dict(n=3, none=None)) == []


class _StreamLib:
    def mc_a(self, *a):
        return 0

    def mc_b(self, *a):
        return 0

    def mc_c(self, *a):
        return 0


def test_gated_recorder_proves_only_with_the_gate_pending():
    import ctypes

    S = 0x7F00
    rec = kh.GatedRecorder(_StreamLib(), header=_HEADER)
    rec.mc_a(None, 1, ctypes.c_void_p(S))  # unarmed: a Recorder
    assert rec.names == ["mc_a"] and rec.log == []
    rec.arm(_Gate(opens=4), S)
    assert rec.names == []  # arming starts a new record
    rec.mc_a(None, 1, ctypes.c_void_p(S))  # questions 1, 2: pending before and after
    rec.mc_b(3)  # questions 3, 4: no stream parameter
    rec.mc_c(ctypes.c_void_p(S), 1)  # questions 5, 6: the gate has opened
    rec.disarm()
    rec.mc_a(None, 1, ctypes.c_void_p(S))  # not logged
    assert rec.log == [("mc_a", S, True, True), ("mc_b", None, True, True), ("mc_c", S, False, False)]
    assert rec.names == ["mc_a", "mc_b", "mc_c", "mc_a"]  # the Recorder's interface goes on
    rec.streams_ok()
    rec.streams_ok("mc_a", "mc_c")
    rec.proven("mc_a")
    assert rec.pending() == ["mc_a", "mc_b"]
    with pytest.raises(AssertionError, match="inconclusive: the gate had opened before mc_c"):
        rec.proven("mc_c")
    with pytest.raises(AssertionError, match="mc_d did not run"):
        rec.proven("mc_d")
    # pending when called, open when it returned: the entry point waited for the stream
    rec.arm(_Gate(opens=1), S)
    rec.mc_a(None, 1, ctypes.c_void_p(S))
    with pytest.raises(AssertionError, match="mc_a returned after the gate had opened"):
        rec.proven("mc_a")
    # the null stream (None, or a c_void_p of 0) and any other stream are not S
    for wrong in (None, ctypes.c_void_p(0), ctypes.c_void_p(0x1234)):
        rec.arm(_Gate(opens=10), S)
        rec.mc_a(None, 1, wrong)
        with pytest.raises(AssertionError, match="mc_a was launched on stream"):
            rec.proven("mc_a")
        with pytest.raises(AssertionError, match="mc_a was launched on stream"):
            rec.streams_ok()
    assert rec.log[-1][1] == 0x1234


def test_sleep_cycles_and_comparisons():
    assert kh.sleep_cycles_for(0.5e-6, 100.0) == 200_000_000 and kh.sleep_cycles_for(1.0, 0.2) == 1
    with pytest.raises(AssertionError):
        kh.sleep_cycles_for(0.0, 100.0)
    a = torch.tensor([1.0, float("nan"), -0.0])
    assert kh.leaves((a, None, [a, (a,)], 3.0)) == [a, a, a]
    kh.assert_same_bits((a, [a]), (a.clone(), [a.clone()]), "same")  # NaN equals NaN: bits are compared
    with pytest.raises(AssertionError, match=r"x\[0\]: 1 of 3 elements differ"):
        kh.assert_same_bits(a, torch.tensor([1.0, float("nan"), 0.0]), "x")  # -0.0 is not +0.0
    with pytest.raises(AssertionError, match="1 results, 2 wanted"):
        kh.assert_same_bits(a, (a, a), "x")
    with pytest.raises(AssertionError, match="0 results"):
        kh.assert_same_bits(None, None, "x")
    b = torch.tensor([1.0, 2.0, 100.0])
    kh.assert_close_rel(b + 5e-3, b, 1e-4, "close")
    with pytest.raises(AssertionError, match="relative error"):
        kh.assert_close_rel(b + 0.1, b, 1e-4, "far")
    with pytest.raises(AssertionError, match="relative error"):
        kh.assert_close_rel(torch.tensor([1.0, float("nan"), 100.0]), b, 1e-4, "poison")
    n = torch.tensor([3, 4], dtype=torch.int32)
    kh.assert_close_rel((b + 5e-3, n), (b, n.clone()), 1e-4, "integers exact")
    with pytest.raises(AssertionError, match=r"x\[1\]\[0\]: 1 of 2 elements differ"):
        kh.assert_close_rel((b, n + torch.tensor([0, 1], dtype=torch.int32)), (b, n), 1.0, "x")  # integers: exact
    with pytest.raises(AssertionError, match=r"x\[0\]\[0\]: 3 of 3"):
        kh.assert_close_rel((b + 5e-3, n), (b, n), 1e-4, "x", exact=(0,))  # a float leaf named exact
