"""What the float64 kernel tests (tests/test_*_kernels_float64.py and their neighbours) measure with, defined once:
which entry points of libmcorr ran (Recorder, `calls`), what the header says of them and whether the ctypes table binds
them so (header_signature, assert_entry_point), a host program built and run under the sanitizers as a child process
(run_host_program), that nothing was written outside an output buffer (nan_buffer, assert_guards, nan_empty; byte_buffer, assert_byte_guards for the
byte-moving kernels), the inputs (float_stack, raw_movie, gain, raw_setup), the worst error over bound per
output family (ratios_fixture, worse), the engine's test switches (`switches`), the delayed-producer run of
tests/test_stream_order.py (gated_run and its tools) and what tests/test_input_contract.py holds a route's inputs to
(relocated, twins, snapshot, assert_inputs_unchanged).  tests/test_kernel_harness_host.py pins every one of them on
the CPU.

A test module takes a fixture with `from kernel_harness import calls  # noqa: F401`."""

import ctypes
import os
import re
import shutil
import subprocess
import time

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


# ------------------------------------------------------------------ stream ordering: a delayed producer on a side stream
#
# tests/test_stream_order.py's method.  The inputs of a case are staged and the result `want` is computed on the
# default stream.  Then, on a fresh side stream S: a sleep kernel (the gate), device-to-device copies of the true
# inputs over POISONED twins, the `gate` event, and the route under test on the twins.  While S sleeps the rest of the
# GPU is idle, so whatever the route enqueues on another side stream runs at once, on poison or on accumulators nobody
# has cleared, and the result is grossly wrong.  (Not reliably so the null stream: on the MI355X runtime a null-stream
# launch was ordered after S's pending work in one run and not in the next; the stream ARGUMENT of every call is what
# pins it.)  GatedRecorder writes down, per entry-point
# call, the stream argument and whether the gate was still pending before and after the call: a call that was made
# after the sleep ended proves nothing and is reported as such, never counted.


def stream_parameter(name, header=None):
    """The index of the `stream` parameter of the entry point `name` in the header, None where it has none."""
    for i, param in enumerate(header_parameters(name, header)):
        if re.search(r"\bstream$", param):
            return i
    return None


def stream_entry_points(names=None, header=None):
    """The entry points among `names` (default: every name of _lib.SIGNATURES) whose header declaration has a
    `stream` parameter, and whose binding puts a c_void_p there: pure host functions fall out."""
    if names is None:
        from torch_motion_correction_amd import _lib

        names = _lib.SIGNATURES
    out = set()
    for name in names:
        i = stream_parameter(name, header)
        if i is not None:
            assert header_signature(name, header)[i] is ctypes.c_void_p, f"{name}: stream is no pointer"
            out.add(name)
    return out


def poisoned(x):
    """The poisoned twin of a device input, a new tensor: NaN for floating point, the bitwise complement for a u8 /
    i16 movie.  An int32 / int64 input is an index or offset table in this suite and is copied as it is: a launch on
    the wrong stream then still reads poisoned samples, but never indexes outside an allocation."""
    if x.is_floating_point():
        return torch.full_like(x, float("nan"))
    if x.dtype in (torch.uint8, torch.int16, torch.bool):
        return torch.bitwise_not(x) if x.dtype != torch.bool else torch.logical_not(x)
    assert x.dtype in (torch.int32, torch.int64), x.dtype
    return x.clone()


def _tensor_slots(obj):
    """(holder, key) of every tensor of a case's input: a tensor itself is slot (None, None); an object (a RawMovie,
    a DefectFill) holds its tensors as attributes.  A tensor inside a tuple, list or dict attribute would be shared
    with the true input and never poisoned: AssertionError."""
    if isinstance(obj, torch.Tensor):
        return [(None, None)]
    for k, v in vars(obj).items():
        assert not _holds_tensor(v), (f"{type(obj).__name__}.{k} holds tensors in a container: they would not be "
                                      "poisoned")
    return [(obj, k) for k, v in sorted(vars(obj).items()) if isinstance(v, torch.Tensor)]


def _holds_tensor(v):
    if isinstance(v, (tuple, list)):
        return any(isinstance(x, torch.Tensor) or _holds_tensor(x) for x in v)
    if isinstance(v, dict):
        return any(isinstance(x, torch.Tensor) or _holds_tensor(x) for x in v.values())
    return False


def _has_tensors(obj):
    """A tensor, or an object that may hold tensors as attributes; a scalar, a tuple, a string, None are not."""
    return obj is not None and (isinstance(obj, torch.Tensor) or hasattr(obj, "__dict__"))


def twins(inputs, fn):
    """{name: input} -> ({name: twin}, [(twin tensor, true tensor), ...]): a tensor's twin is fn(tensor); an object's
    twin is a shallow copy whose tensor attributes (_tensor_slots) are fn of the true ones (everything else is
    shared); a scalar, a tuple, a string, None is passed through."""
    import copy

    out, pairs = {}, []
    for name, obj in inputs.items():
        if not _has_tensors(obj):
            out[name] = obj
            continue
        if isinstance(obj, torch.Tensor):
            out[name] = fn(obj)
            pairs.append((out[name], obj))
            continue
        twin = copy.copy(obj)
        for _, k in _tensor_slots(obj):
            true = getattr(obj, k)
            setattr(twin, k, fn(true))
            pairs.append((getattr(twin, k), true))
        out[name] = twin
    return out, pairs


def poisoned_twins(inputs):
    """twins() with poisoned(): what gated_run copies the true inputs over behind the gate."""
    return twins(inputs, poisoned)


def relocated(x, lead_bytes=16):
    """A copy of the tensor `x` (any dtype narrower than 16 bytes, any device) that starts ONE ELEMENT past a 16-byte
    boundary of a larger allocation: contiguous, equal to `x`, data_ptr() % 16 == element_size().  In front of it lie
    `lead_bytes` (whole 16-byte pieces, at least one) and the one element, behind it the rest of its last piece and
    one whole piece more, so a kernel that rounds its pointer down or reads a whole last piece stays inside the
    allocation.  The padding is all-ones bytes: NaN for a floating-point reader, -1 / 255 for an integer one.  (An
    empty tensor has no start to speak of and is cloned.)"""
    if x.numel() == 0:
        return x.detach().clone()
    size = x.element_size()
    assert lead_bytes >= 16 and lead_bytes % 16 == 0 and size < 16, (lead_bytes, size)
    start, nbytes = lead_bytes + size, x.numel() * size
    total = (start + nbytes + 15) // 16 * 16 + 16
    flat = torch.full((total,), 255, dtype=torch.uint8, device=x.device)
    assert flat.data_ptr() % 16 == 0
    view = flat[start:start + nbytes].view(x.dtype).view(x.shape)
    view.copy_(x.detach())
    assert view.is_contiguous() and view.data_ptr() % 16 == size and total - start - nbytes >= 16
    return view


def snapshot(inputs):
    """{name: input} -> [(label, the tensor itself, a copy of it on the CPU), ...] over every tensor of the inputs,
    those an object holds (_tensor_slots) included; the label is `name` or `name.attribute`."""
    snap = []
    for name, obj in inputs.items():
        if _has_tensors(obj):
            for holder, k in _tensor_slots(obj):
                x = obj if holder is None else getattr(obj, k)
                snap.append((name if holder is None else f"{name}.{k}", x, x.detach().cpu().clone()))
    return snap


def assert_inputs_unchanged(inputs, snap, what):
    """Every tensor of `inputs` that snapshot() saw holds the bits it held then (the device is read here: the caller
    synchronises first), and every input still holds the SAME tensors: one rebound on an object fails too."""
    now = {label: x for label, x, _ in snapshot(inputs)}
    for label, x, then in snap:
        if label.split(".")[0] in inputs:
            assert now.get(label) is x, f"{what}: the input {label} was replaced by another tensor"
            assert_same_bits(x, then, f"{what}: the input {label} was written to:")


class GatedRecorder(Recorder):
    """Recorder that knows about the gate.  Armed with the `gate` event (anything with .query()) and the side
    stream's handle, it writes down per entry-point call, in `log`: (name, the `stream` argument as an int, 0 for the
    null stream, None where the entry point takes none; gate pending before the call; gate pending after it
    returned).  Unarmed it is a Recorder."""

    def __init__(self, lib, header=None):
        super().__init__(lib)
        self.log, self.gate, self.stream, self.enqueue_ms = [], None, None, None
        self._header, self._slot = header, {}

    def arm(self, gate, stream):
        self.clear()
        self.gate, self.stream = gate, int(stream)

    def disarm(self):
        """No call is logged from here on; the log and the armed stream stay for the assertions."""
        self.gate = None

    def clear(self):
        super().clear()
        del self.log[:]

    def _stream_of(self, name, a):
        if name not in self._slot:
            try:
                self._slot[name] = stream_parameter(name, self._header)
            except KeyError:
                self._slot[name] = None
        i = self._slot[name]
        if i is None:
            return None
        v = a[i]
        v = getattr(v, "value", v)
        return 0 if v is None else int(v)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.names.append(name)
            self.args.setdefault(name, []).append(a)
            if self.gate is None:
                return fn(*a)
            before = not self.gate.query()
            out = fn(*a)
            self.log.append((name, self._stream_of(name, a), before, not self.gate.query()))
            return out

        return call

    def streams_ok(self, *names):
        """Every recorded call of `names` (default: of every stream-taking entry point that ran) had the armed stream
        as its stream argument."""
        for name, st, _, _ in self.log:
            if st is not None and (not names or name in names):
                assert st == self.stream, f"{name} was launched on stream {st:#x}, not on {self.stream:#x}"
        for name in names:
            assert any(n == name for n, *_ in self.log), f"{name} did not run ({sorted(set(self.names))})"

    def proven(self, *names):
        """Every call of each of `names` ran at least once, on the armed stream, with the gate pending when it was
        called AND when it returned (the entry point did not wait for the stream).  A call after the sleep has ended
        proves nothing: AssertionError('inconclusive ...'), never a pass."""
        self.streams_ok(*names)
        for name in names:
            for n, _, before, after in self.log:
                if n == name:
                    assert before, f"inconclusive: the gate had opened before {name} was called"
                    assert after, f"{name} returned after the gate had opened: it waited for the stream"

    def pending(self):
        """The names whose every call had the gate pending before and after, in first-call order (a survey)."""
        bad = {n for n, _, b, a in self.log if not (b and a)}
        return [n for n in dict.fromkeys(n for n, *_ in self.log) if n not in bad]


def sleep_cycles_for(ms_per_cycle, target_ms):
    """The `cycles` argument of torch.cuda._sleep for a delay of `target_ms`, from a measured rate."""
    assert ms_per_cycle > 0 and target_ms > 0
    return max(1, int(round(target_ms / ms_per_cycle)))


def calibrate_sleep(cycles=20_000_000):
    """ms per cycle of torch.cuda._sleep on the current device, timed once with two events."""
    torch.cuda._sleep(1000)  # the kernel's first launch loads its code
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / cycles


def gated_run(route, inputs, rec, cycles, want=None):
    """The delayed-producer run of `route(**inputs)` -> (want, got, S).  `inputs`: {name: device tensor, object with
    device tensors as attributes (RawMovie), or plain value}, staged and synchronised by the caller.  `want` is
    route(**inputs) on the default stream (computed here unless given; it also fills every plan and table cache, so
    that nothing behind the gate copies from host memory).  Then on a fresh side stream S: sleep, copy the true
    inputs over their poisoned twins, record the gate, arm `rec`, run the route on the twins, synchronise S."""
    if want is None:
        want = route(**inputs)
    torch.cuda.synchronize()
    twins, pairs = poisoned_twins(inputs)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    gate = torch.cuda.Event()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        for twin, true in pairs:
            twin.copy_(true, non_blocking=True)
        gate.record(S)
        rec.arm(gate, S.cuda_stream)
        t0 = time.perf_counter()
        try:
            got = route(**twins)
        finally:
            rec.enqueue_ms = 1e3 * (time.perf_counter() - t0)  # the host's time in the route, read-backs included
            rec.disarm()
        S.synchronize()
    return want, got, S


def leaves(x):
    """The tensors of a route's result (a tensor, or nested tuples / lists with None allowed), in order."""
    if x is None:
        return []
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, (tuple, list)):
        return [t for v in x for t in leaves(v)]
    return []  # a float, a history on the CPU as a list ...


def assert_same_bits(got, want, what):
    """Every tensor of `got` equals its twin in `want` bit for bit (NaN included: compared as integers)."""
    g, w = leaves(got), leaves(want)
    assert len(g) == len(w) and len(w) >= 1, f"{what}: {len(g)} results, {len(w)} wanted"
    for i, (a, b) in enumerate(zip(g, w)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}[{i}]: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
        bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        if a.dtype == torch.bool:
            bits = torch.bool
        same = torch.equal(a.view(bits), b.view(bits))
        if not same:
            bad = int((a.view(bits) != b.view(bits)).sum())
            nans = int(torch.isnan(a).sum()) if a.is_floating_point() else 0
            raise AssertionError(f"{what}[{i}]: {bad} of {a.numel()} elements differ ({nans} NaN)")


def assert_close_rel(got, want, rel, what, exact=()):
    """Every floating-point tensor of `got` within rel * max |want| of its twin, NaN never; every integer tensor,
    and every tensor whose position is in `exact`, equal bit for bit."""
    g, w = leaves(got), leaves(want)
    assert len(g) == len(w) and len(w) >= 1, f"{what}: {len(g)} results, {len(w)} wanted"
    for i, (a, b) in enumerate(zip(g, w)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}[{i}]: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        if i in exact or not a.is_floating_point():
            assert_same_bits(a, b, f"{what}[{i}]")
            continue
        e = rel_err(a, b)
        assert e <= rel, f"{what}[{i}]: relative error {e!r} beyond {rel!r}"  # NaN fails: not <=
