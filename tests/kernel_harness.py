"""What the float64 kernel tests (tests/test_*_kernels_float64.py and their neighbours) measure with, defined once:
which entry points of libmcorr ran (Recorder, `calls`), what the header says of them and whether the ctypes table binds
them so (header_signature, assert_entry_point), a host program built and run under the sanitizers as a child process
(run_host_program), that nothing was written outside an output buffer (nan_buffer, assert_guards, nan_empty; byte_buffer, assert_byte_guards for the
byte-moving kernels), the inputs (float_stack, raw_movie, gain, raw_setup), the worst error over bound per
output family (ratios_fixture, worse) and the engine's test switches (`switches`).  tests/test_kernel_harness_host.py
pins every one of them on the CPU.

A test module takes a fixture with `from kernel_harness import calls  # noqa: F401`."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

GUARD = 8  # NaN words kept on either side of an output buffer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch_motion_correction_amd", "csrc")


# ------------------------------------------------------------------ the package, the library, which entry points ran


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


@pytest.fixture(scope="module")
def lib():
    from torch_motion_correction_amd import _lib

    return _lib.load()


class Recorder:
    """The loaded library with the names and the arguments of the entry points that are CALLED written down, in
    order.  Looking an entry point up records nothing."""

    def __init__(self, lib):
        self._lib, self.names, self.args = lib, [], {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.names.append(name)
            self.args.setdefault(name, []).append(a)
            return fn(*a)

        return call

    def count(self, name):
        return self.names.count(name)

    def clear(self):
        del self.names[:]
        self.args.clear()

    def ran(self, *want, absent=()):
        for name in want:
            assert self.count(name) >= 1, f"{name} did not run ({sorted(set(self.names))})"
        for name in absent:
            assert self.count(name) == 0, f"{name} ran ({sorted(set(self.names))})"

    def only(self, name, times):
        assert self.names == [name] * times, f"expected {times} x {name}, ran {self.names}"


@pytest.fixture
def calls(monkeypatch):
    from torch_motion_correction_amd import _lib

    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    return rec


# ------------------------------------------------------------------ the header against the ctypes table

SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_int64, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
           "unsigned": ctypes.c_uint, "double": ctypes.c_double}
POINTEES = {"long long": ctypes.c_int64, "int64_t": ctypes.c_int64, "double": ctypes.c_double}  # + the two structs


def header_text(header=None):
    """include/mcorr.h (or `header`, a header's text) without its /* */ and // comments."""
    if header is None:
        with open(os.path.join(ROOT, "include", "mcorr.h")) as fh:
            header = fh.read()
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)


def declared_entry_points(header=None):
    """The names of the entry points (`int mc_x(...);`) the header declares."""
    return set(re.findall(r"^int\s+(mc_\w+)\s*\(", header_text(header), flags=re.M))


def header_parameters(name, header=None):
    """The parameters of the entry point `name` as the header writes them, comments stripped and blanks folded:
    ["const void* src", "int h", "const double m[4]", ...]; [] for (void).  KeyError where `name` is not declared."""
    found = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header_text(header), flags=re.M | re.S)
    if found is None:
        raise KeyError(f"the header declares no {name}")
    params = [" ".join(p.split()) for p in found.group(1).split(",")]
    return [] if params in ([""], ["void"]) else params


def _declared(name, header=None):
    """Per parameter of `name`: (its ctypes type with every pointer and array as c_void_p, the ctypes pointee a
    binding may spell out instead -- POINTEES, mc_xc_geom, mc_xc_line -- or None)."""
    from torch_motion_correction_amd import _lib

    pointees = {**POINTEES, "mc_xc_geom": _lib.XcGeom, "mc_xc_line": _lib.XcLine}
    out = []
    for param in header_parameters(name, header):
        words = re.sub(r"\bconst\b", " ", re.split(r"[*\[]", param)[0]).split()  # `T` of `T* x`, `T x` otherwise
        base = " ".join(words if "*" in param else words[:-1])
        if "*" in param or "[" in param:
            out.append((ctypes.c_void_p, pointees.get(base)))
        elif base in SCALARS:
            out.append((SCALARS[base], None))
        else:
            raise ValueError(f"{name}: no ctypes twin for the parameter {param!r}")
    return out


def header_signature(name, header=None):
    """The ctypes argument types of the entry point `name` as the header declares it, for comparison with
    _lib.SIGNATURES[name]: a scalar is its ctypes twin (SCALARS), a pointer or an array c_void_p.  ValueError for a
    scalar of any other type: nothing falls back to int."""
    return [ctype for ctype, _ in _declared(name, header)]


def binding_disagreement(name, bound, header=None):
    """None where the ctypes list `bound` can stand for the header's declaration of `name`, else what is wrong.  A
    scalar is bound as itself; a pointer as c_void_p or, where the header names a pointee the binding may spell out,
    as the POINTER to it."""
    declared = _declared(name, header)
    if len(declared) != len(bound):
        return f"the header has {len(declared)} parameters, the binding {len(bound)}"
    for i, ((ctype, pointee), b) in enumerate(zip(declared, bound)):
        if b is not ctype and (pointee is None or b is not ctypes.POINTER(pointee)):
            what = ctype.__name__ if pointee is None else f"a pointer to {pointee.__name__}"
            return f"parameter {i}: the header says {what}, the binding {b.__name__}"
    return None


def assert_entry_point(name, want=None, source=None, header=None, signatures=None):
    """`name` is declared in include/mcorr.h, bound in _lib.SIGNATURES, exported by the loaded library, and bound as
    declared, parameter by parameter.  `want`: the literal ctypes list the binding must equal.  `source`: the
    (file, stem, flags) entry _build.SOURCES must hold.  `header`, `signatures`: a header's text and a table to check
    instead of the committed ones (nothing is looked up in the library then)."""
    from torch_motion_correction_amd import _build, _lib

    assert name in declared_entry_points(header), f"{name} is not declared in the header"
    table = _lib.SIGNATURES if signatures is None else signatures
    assert name in table, f"{name} is not bound"
    if header is None and signatures is None:
        assert getattr(_lib.load(), name) is not None
    wrong = binding_disagreement(name, table[name], header)
    assert wrong is None, f"{name}: {wrong}"
    if want is not None:
        assert table[name] == want, f"{name}: bound as {table[name]}"
    if source is not None:
        assert source in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, source[0])), source


# ------------------------------------------------------------------ host programs, run as child processes

SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
PLAIN = ["-O1", "-std=c++17"]


def run_host_program(source, tmp_path, *args, sanitize=True):
    """Builds tests/`source` (or `source` as it is where it is an absolute path) into `tmp_path` with clang++ -- the
    ROCm one, else the one on PATH, else the test is skipped -- against csrc/, under the address and
    undefined-behaviour sanitizers unless `sanitize` is False, and runs it with `args` as a child process: it must
    return 0, end its output with OK and print no FAIL.  -> the CompletedProcess.  Nothing sanitized is loaded into
    this process."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++")
    if not cxx:
        pytest.skip("no clang++ on this machine")
    exe = os.path.join(str(tmp_path), os.path.splitext(os.path.basename(source))[0])
    subprocess.run([cxx, *(SANITIZE if sanitize else PLAIN), "-I", CSRC, os.path.join(ROOT, "tests", source),
                    "-o", exe, *([] if sanitize else ["-lm"])], check=True)
    res = subprocess.run([exe, *(str(a) for a in args)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout[-2000:] + res.stderr[-4000:]
    assert "FAIL" not in res.stdout, res.stdout[-2000:]
    return res


# ------------------------------------------------------------------ NaN-filled and NaN-guarded buffers


@pytest.fixture
def nan_empty(monkeypatch):
    """torch.empty hands out NaN-filled floating-point buffers: what a kernel leaves unwritten fails its comparison."""
    real = torch.empty

    def empty(*a, **k):
        out = real(*a, **k)
        return out.fill_(float("nan")) if out.is_floating_point() else out

    monkeypatch.setattr(torch, "empty", empty)


def nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def nan_buffer(shape, dev, offset=0):
    """A NaN-filled fp32 buffer of `shape` that starts `offset` floats past a 16-byte boundary, inside a larger
    NaN-filled allocation -> (view, whole allocation)."""
    n = int(np.prod(shape))
    lead = 4 * ((GUARD + 3) // 4) + offset
    flat = torch.full((lead + n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    view = flat[lead:lead + n].view(*shape)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view, flat


def assert_guards(view, flat, what):
    n, lead = view.numel(), (view.data_ptr() - flat.data_ptr()) // 4
    assert bool(torch.isnan(flat[:lead]).all()) and bool(torch.isnan(flat[lead + n:]).all()), \
        f"{what}: wrote outside its output buffer"


def byte_buffer(nbytes, dev, past=0):
    """`nbytes` bytes that start `past` bytes beyond a 16-byte boundary, inside a larger NaN-filled allocation ->
    (the uint8 view, the whole allocation as bytes).  The byte tests' sibling of nan_buffer; a typed buffer is
    ``view.view(dtype).view(shape)``."""
    lead = 4 * GUARD + past
    flat = torch.full(((lead + nbytes + 3) // 4 + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    whole = flat.view(torch.uint8)
    view = whole[lead:lead + nbytes]
    assert whole.data_ptr() % 16 == 0 and view.data_ptr() % 16 == past % 16
    return view, whole


def assert_byte_guards(view, whole, what):
    """No byte of `whole` outside `view` (of any dtype) differs from the NaN words byte_buffer filled it with."""
    lead, n = view.data_ptr() - whole.data_ptr(), view.numel() * view.element_size()
    fresh = torch.full((whole.numel() // 4,), float("nan"), dtype=torch.float32).view(torch.uint8)
    got = whole.cpu()
    assert torch.equal(got[:lead], fresh[:lead]) and torch.equal(got[lead + n:], fresh[lead + n:]), \
        f"{what}: wrote outside its buffer"


def offset_copy(src, offset):
    """`src` copied to `offset` elements past a 16-byte boundary of a larger allocation."""
    flat = torch.zeros(src.numel() + 16, dtype=src.dtype, device=src.device)
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + src.numel()].view(src.shape)
    view.copy_(src)
    return view


# ------------------------------------------------------------------ inputs


def rng(*seed):
    """numpy's generator seeded with a tuple of integers (the reference modules' cases)."""
    return np.random.default_rng([int(s) for s in seed])


def float_stack(t, h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(t * 7919 + h * 31 + w)
    st = (torch.randn(t, h, w, generator=g) * 2 + 5).to(dtype)
    assert not bool((st == 0).any())  # the references divide the zeros of an output from its values
    return st


def drifting_raw_movie(dy, dx, h, w, dtype, seed, pad=64):
    """A texture in [10, 50) cropped at the integer drift (dy[f], dx[f]) + noise, rounded to the detector's integers
    (i16: scaled and offset so that negative counts occur)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(h + 2 * pad, w + 2 * pad, generator=g) * 40 + 10
    raw = torch.empty((len(dy), h, w), dtype=dtype)
    for f, (a, b) in enumerate(zip(dy, dx)):
        v = base[pad - a: pad - a + h, pad - b: pad - b + w] + 2 * torch.randn(h, w, generator=g)
        raw[f] = (v * 8 - 100).round().clamp(-32768, 32767).to(dtype) if dtype == torch.int16 else \
            v.round().clamp(0, 255).to(dtype)
    return raw


def raw_movie(t, h, w, dtype, seed):
    """drifting_raw_movie without a drift and without a margin: a static texture + noise."""
    return drifting_raw_movie([0] * t, [0] * t, h, w, dtype, seed, pad=0)


def gain(h, w, seed=9):
    """A gain reference with a large dynamic range, log-uniform in [0.25, 4]: a wrong gain row or column (a cache
    offset error) changes the output by a factor, which a constant or near-constant gain would hide."""
    g = torch.Generator().manual_seed(seed + h * 7 + w)
    out = 4.0 ** (2 * torch.rand(h, w, generator=g) - 1)
    assert float(out.min()) >= 0.25 and float(out.max()) <= 4.0 and float(out.max() / out.min()) > 8
    return out


def raw_setup(dev, t, h, w, dtype, with_gain, seed):
    """-> (raw, gain or None, engine.RawMovie of both on `dev`: kind, mu; the all-ones gain for None)."""
    from torch_motion_correction_amd import engine

    raw = raw_movie(t, h, w, dtype, seed)
    g = gain(h, w) if with_gain else None
    rm = engine.RawMovie(raw.to(dev), None if g is None else g.to(dev))
    torch.cuda.synchronize()
    return raw, g, rm


# ------------------------------------------------------------------ worst error / bound per output family


def ratio_lines(ratios, prefix="RATIO"):
    return [f"{prefix} {k}: {ratios[k]:.3f}" for k in sorted(ratios)]


def ratios_fixture(prefix="RATIO"):
    """`ratios = ratios_fixture()` in a test module: a dict filled through worse(), printed when the module is done."""

    @pytest.fixture(scope="module")
    def ratios():
        r = {}
        yield r
        for line in ratio_lines(r, prefix):
            print(line)

    return ratios


def worse(ratios, key, value):
    ratios[key] = max(ratios.get(key, 0.0), value)
    return value


def rel_err(a, b):
    """max |a - b| / max |b| in float64."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def assert_sum(total, want, bound, what, border=None):
    """Every pixel of a frame sum within its bound.  Returns the worst |got - want| / bound, over the pixels outside
    `border` where one is given (a kernel that writes the allowed 0 on the border sits at the end of its interval by
    design)."""
    got = total.detach().cpu().double().numpy()
    d = np.abs(got - want)
    ok = d <= bound
    if not bool(ok.all()):
        bad = np.argwhere(~ok)
        raise AssertionError(f"{what}: {len(bad)} pixels of the sum beyond the bound, first (row, col) "
                             f"{[tuple(int(v) for v in b) for b in bad[:8]]}: got {got[tuple(bad[0])]!r} "
                             f"want {want[tuple(bad[0])]!r} bound {bound[tuple(bad[0])]!r}")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.nan_to_num(d / bound, nan=0.0, posinf=0.0)
    return float(ratio.max() if border is None else np.where(border, 0.0, ratio).max())


# ------------------------------------------------------------------ the engine's test switches

ENGINE_SWITCHES = ("FUSED_SEARCH", "USE_ROW_CHORDS", "WORKSPACE_BYTES", "FULL_ROW_MAJOR", "DOSE_COLUMN_MAJOR",
                   "POLYPHASE_FOURIER_SHIFT")


@pytest.fixture
def switches(monkeypatch):
    """-> (engine, plan).  A test assigns the switches plainly; every one is back at its former value afterwards, and
    plan's line cache is cleared before and after the test."""
    from torch_motion_correction_amd import engine, plan

    for name in ENGINE_SWITCHES:
        monkeypatch.setattr(engine, name, getattr(engine, name))
    monkeypatch.setattr(plan, "USE_DIRECT_LINES", plan.USE_DIRECT_LINES)
    plan._LINES.clear()
    yield engine, plan
    plan._LINES.clear()
