"""The detector-defect fill on the GPU (DefectFill: mc_defect_donors; fill_defects_raw: mc_raw_fill_defects;
fill_defects_gain: mc_gain_fill_defects; csrc/defect_fill.hip) against the restatement of the rule in Python integers
(tests/defect_reference.py).  The rule is integer and copy-exact: every comparison is torch.equal / np.array_equal on
the elements' bits, and there are no tolerances -- except the composition's frame sums, whose bound is derived in
that test."""

import numpy as np
import pytest
import torch

import defect_reference as dr
from kernel_harness import (assert_guards, assert_sum, calls, drifting_raw_movie, gain as random_gain, mc,  # noqa: F401
                            nan_buffer)
from rigid_reference import condition_float64, conditioning_error, rigid_resample_gather_stack

pytestmark = pytest.mark.gpu

ENTRIES = ("mc_defect_donors", "mc_raw_fill_defects", "mc_gain_fill_defects")
DTYPES = {"u8": torch.uint8, "i16": torch.int16, "f16": torch.float16, "f32": torch.float32}
BITS = {torch.uint8: torch.uint8, torch.int16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
SEEDS = (0, 12345)


# ------------------------------------------------------------------ maps, movies, the restatement computed once


def planted_map(block=7):
    """(33, 927): the four corners, an edge pixel, full dead columns at x = 0 and x = 500, a full dead row, and a
    block x block square whose centre (7: rings 1 .. 3 are defects) finds its first good ring at exactly r = 4."""
    m = np.zeros((33, 927), dtype=bool)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    m[16, -1] = True
    m[:, 0] = m[:, 500] = True
    m[27, :] = True
    m[4:4 + block, 200:200 + block] = True
    return m


def small_map():
    m = np.zeros((8, 16), dtype=bool)
    m[0, 0] = m[7, 15] = m[3, 5] = m[3, 6] = m[4, 5] = True
    m[:, 9] = True
    return m


def wide_map():
    """(64, 4096): more than one workgroup of defects in a row (a dead row of 4096), a dead column, single pixels."""
    m = np.zeros((64, 4096), dtype=bool)
    m[40, :] = True
    m[:, 2085] = True
    m[0, 0] = m[63, 4095] = m[10, 10] = m[10, 11] = True
    return m


MAPS = {"33x927": planted_map, "8x16": small_map, "64x4096": wide_map}
FRAMES = {"33x927": 5, "8x16": 1, "64x4096": 3}
_TABLES = {}


def table(name, reach=4):
    """The restatement's (map, (pixels, donors, counts)) of a named map, computed once and left unchanged."""
    if (name, reach) not in _TABLES:
        m = MAPS[name]()
        tb = dr.donor_table(m, reach)
        for a in tb:
            a.setflags(write=False)
        _TABLES[name, reach] = (m, tb)
    return _TABLES[name, reach]


def random_movie(shape, dtype, seed):
    """A numpy movie of random bits (every value of the type, NaNs and infinities of the float types included)."""
    rs = np.random.RandomState(seed)
    if dtype == torch.uint8:
        return rs.randint(0, 256, size=shape).astype(np.uint8)
    if dtype == torch.float32:
        return rs.randint(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32).view(np.float32)
    a = rs.randint(-32768, 32768, size=shape).astype(np.int16)
    return a.view(np.float16) if dtype == torch.float16 else a


def bits(x):
    """A tensor or numpy array as a CPU tensor of same-sized integers."""
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x.detach().cpu().contiguous()
    return x.view(BITS[x.dtype])


def offset_view(src, offset=1):
    """`src` copied to `offset` elements past a 16-byte boundary of a larger allocation (any dtype)."""
    flat = torch.zeros(src.numel() + 16, dtype=src.dtype, device=src.device)
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + src.numel()].view(src.shape)
    view.copy_(src)
    assert view.is_contiguous() and view.data_ptr() % 16 == (offset * src.element_size()) % 16
    return view, flat


# ------------------------------------------------------------------ the donor table


def _device_tables(dev, dmap, reach):
    """mc_defect_donors through the C ABI on the test's own buffers (a reach at which a defect has no donor is a
    table like any other there) -> numpy (pixels, donors, counts)."""
    from torch_motion_correction_amd import _lib

    h, w = dmap.shape
    md = torch.from_numpy(dmap).to(dev)
    pixels = torch.nonzero(md.reshape(-1)).reshape(-1).to(torch.int32)
    n = int(pixels.numel())
    donors = torch.full((n, 8 * reach), -7, dtype=torch.int32, device=dev)
    counts = torch.full((n,), -7, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().mc_defect_donors(_lib.ptr(md.view(torch.uint8)), h, w, _lib.ptr(pixels), n, reach,
                                            _lib.ptr(donors), _lib.ptr(counts), _lib.stream_ptr(dev)),
               "mc_defect_donors")
    torch.cuda.synchronize()
    return pixels.cpu().numpy(), donors.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("reach", [1, 4, 16])
def test_donor_table_equals_the_restatement(mc, dev, reach):
    dmap, want = table("33x927", reach)
    got = _device_tables(dev, dmap, reach)
    for g, w_, name in zip(got, want, ("pixels", "donors", "counts")):
        assert g.dtype == np.int32 and g.shape == w_.shape and np.array_equal(g, w_), (name, reach)
    centre = got[0].tolist().index(7 * 927 + 203)
    if reach == 1:  # inside the 7 x 7 block ring 1 holds defects only
        assert got[2][centre] == 0 and dr.first_without_donor(dmap, 1) == (5, 201)
        with pytest.raises(ValueError, match=r"\(y, x\) = \(5, 201\).*reach=1"):
            mc.DefectFill(torch.from_numpy(dmap), reach=1, device=dev)
        return
    assert got[2][centre] == 8 * 4 and int(got[2].min()) >= 1  # the whole ring r = 4, nothing nearer
    plan = mc.DefectFill(torch.from_numpy(dmap), reach=reach, device=dev)
    assert (plan.shape, plan.reach, plan.n) == ((33, 927), reach, len(want[0])) and plan.device == dev
    for g, w_ in zip((plan.pixels, plan.donors, plan.counts), want):
        assert g.dtype == torch.int32 and g.device == dev and tuple(g.shape) == w_.shape
        assert np.array_equal(g.cpu().numpy(), w_)


def test_defect_without_a_donor_is_an_error(mc, dev):
    dmap = planted_map(block=9)
    first = dr.first_without_donor(dmap, 4)
    assert first == (8, 204)  # the 9 x 9 block's centre: rings 1 .. 4 are defects
    with pytest.raises(ValueError, match=r"\(y, x\) = \(8, 204\).*reach=4"):
        mc.DefectFill(torch.from_numpy(dmap), device=dev)
    movie = torch.zeros(2, 33, 927, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match=r"\(y, x\) = \(8, 204\).*reach=4"):  # the default reach, before the movie
        mc.fill_defects_raw(movie, torch.from_numpy(dmap), in_place=True)
    assert not bool(movie.any())
    with pytest.raises(ValueError, match=r"\(8, 204\)"):
        mc.fill_defects_gain(torch.ones(33, 927, device=dev), torch.from_numpy(dmap))
    assert mc.DefectFill(torch.from_numpy(dmap), reach=5, device=dev).n == int(dmap.sum())


# ------------------------------------------------------------------ the fill


@pytest.fixture(scope="module")
def plans(mc, dev):
    return {name: mc.DefectFill(torch.from_numpy(table(name)[0]), device=dev) for name in MAPS}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("name", list(MAPS))
def test_fill_equals_the_restatement(mc, dev, plans, name, kind, seed):
    dmap, tb = table(name)
    dtype = DTYPES[kind]
    m = random_movie((FRAMES[name],) + dmap.shape, dtype, seed=len(name) + seed)
    want = bits(dr.fill(m, dmap, 4, seed, table=tb))
    movie = torch.from_numpy(m).to(dev)
    keep = movie.clone()
    got = mc.fill_defects_raw(movie, plans[name], seed=seed)
    assert got.dtype == dtype and got.shape == movie.shape and got.device == movie.device
    assert got.data_ptr() != movie.data_ptr() and torch.equal(bits(movie), bits(keep))  # the input is left alone
    assert torch.equal(bits(got), want), (name, kind, seed)
    good = torch.from_numpy(~dmap)
    assert torch.equal(bits(got)[:, good], bits(m)[:, good])  # every non-defect element, bit for bit
    # in place: the same tensor object, the same values
    same = mc.fill_defects_raw(movie, plans[name], seed=seed, in_place=True)
    assert same is movie and torch.equal(bits(movie), want)
    if seed == SEEDS[0]:  # a bool map builds the same plan; a CPU movie comes back on the CPU; (h, w) is one frame
        from_map = mc.fill_defects_raw(torch.from_numpy(m), torch.from_numpy(dmap), seed=seed, device=dev)
        assert from_map.device.type == "cpu" and torch.equal(bits(from_map), want)
        one = mc.fill_defects_raw(torch.from_numpy(m[0]).to(dev), plans[name], seed=seed)
        assert one.shape == dmap.shape and torch.equal(bits(one), want[0])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", list(DTYPES))
def test_fill_of_a_view_one_element_off_a_16_byte_address(mc, dev, plans, kind, seed):
    name = "33x927"
    dmap, tb = table(name)
    m = random_movie((3,) + dmap.shape, DTYPES[kind], seed=99)
    want = bits(dr.fill(m, dmap, 4, seed, table=tb))
    view, flat = offset_view(torch.from_numpy(m).to(dev))
    got = mc.fill_defects_raw(view, plans[name], seed=seed)  # read from the view
    assert torch.equal(bits(got), want) and torch.equal(bits(view), bits(m))
    assert mc.fill_defects_raw(view, plans[name], seed=seed, in_place=True) is view  # filled in the view
    assert torch.equal(bits(view), want)
    assert not bool(flat[:1].any()) and not bool(flat[1 + view.numel():].any())  # nothing outside the view
    # a non-contiguous view is copied like any other movie, and refused in place
    rows = torch.from_numpy(random_movie((3, 66, 927), DTYPES[kind], seed=98)).to(dev)[:, ::2]
    assert not rows.is_contiguous()
    assert torch.equal(bits(mc.fill_defects_raw(rows, plans[name], seed=seed)),
                       bits(dr.fill(rows.cpu().numpy(), dmap, 4, seed, table=tb)))
    with pytest.raises(ValueError, match="in_place=True needs a contiguous movie"):
        mc.fill_defects_raw(rows, plans[name], in_place=True)


def test_nan_payloads_and_guarded_output(mc, dev, plans):
    """An fp32 movie with NaNs of distinct payloads at all six donors of a dead-column pixel: the filled values are
    those bit patterns.  The output sits 1 float off a 16-byte address between NaN guard words, which stay."""
    name, seed = "33x927", 0
    dmap, tb = table(name)
    pixels, donors, counts = tb
    t, (h, w) = 5, dmap.shape
    g = torch.Generator().manual_seed(5)
    m = torch.randn(t, h, w, generator=g).numpy()
    j = pixels.tolist().index(10 * w + 500)
    assert counts[j] == 6
    for k, d in enumerate(donors[j, :6]):
        m.view(np.uint32).reshape(t, -1)[:, d] = 0x7FC00001 + 0x111 * k  # quiet NaNs, payloads 1, 0x112, ...
        m.view(np.uint32).reshape(t, -1)[0, d] |= 0x80000000  # and a sign in frame 0
    want = dr.fill(m, dmap, 4, seed, table=tb)
    view, flat = nan_buffer((t, h, w), dev, offset=1)
    view.copy_(torch.from_numpy(m))
    got = mc.fill_defects_raw(view, plans[name], seed=seed, in_place=True)
    torch.cuda.synchronize()
    assert got is view and torch.equal(bits(view), bits(want))
    assert_guards(view, flat, "fill_defects_raw in place")
    filled = bits(view).reshape(t, -1)[:, 10 * w + 500].tolist()
    for f, v in enumerate(filled):
        k = dr.pick(seed, f, j, 6)
        assert v & 0xFFFFFFFF == (0x7FC00001 + 0x111 * k) | (0x80000000 if f == 0 else 0), (f, hex(v & 0xFFFFFFFF))
    good = torch.from_numpy(~dmap)
    assert torch.equal(bits(view)[:, good], bits(m)[:, good])
    # the gain's output between guards as well
    gain = random_gain(h, w)
    gview, gflat = nan_buffer((h, w), dev, offset=3)
    gview.copy_(gain)
    from torch_motion_correction_amd import _lib

    p = plans[name]
    _lib.check(_lib.load().mc_gain_fill_defects(_lib.ptr(gview), h, w, _lib.ptr(p.pixels), _lib.ptr(p.donors),
                                                _lib.ptr(p.counts), p.n, p.reach, _lib.stream_ptr(dev)),
               "mc_gain_fill_defects")
    torch.cuda.synchronize()
    assert_guards(gview, gflat, "mc_gain_fill_defects")
    assert torch.equal(bits(gview), bits(dr.gain_fill(gain.numpy(), dmap, 4, table=tb)))


def test_a_map_without_defects_launches_nothing(mc, dev, calls):
    empty = torch.zeros(33, 927, dtype=torch.bool)
    plan = mc.DefectFill(empty, device=dev)
    assert plan.n == 0 and plan.pixels.shape == (0,) and plan.donors.shape == (0, 32) and plan.counts.shape == (0,)
    m = random_movie((2, 33, 927), torch.float32, seed=1)
    movie = torch.from_numpy(m).to(dev)
    for fill in (plan, empty):
        got = mc.fill_defects_raw(movie, fill, seed=3)
        assert got.data_ptr() != movie.data_ptr() and torch.equal(bits(got), bits(m))
        assert mc.fill_defects_raw(movie, fill, in_place=True) is movie and torch.equal(bits(movie), bits(m))
        gain = random_gain(33, 927).to(dev)
        filled = mc.fill_defects_gain(gain, fill)
        assert filled.data_ptr() != gain.data_ptr() and torch.equal(filled, gain)
    calls.ran(absent=ENTRIES)
    # the recorder does see the three entry points of a map with defects
    one = empty.clone()
    one[5, 5] = True
    mc.fill_defects_gain(gain, one)
    mc.fill_defects_raw(movie, one)
    calls.ran("mc_defect_donors", "mc_raw_fill_defects", "mc_gain_fill_defects")
    assert calls.count("mc_defect_donors") == 2 and calls.count("mc_raw_fill_defects") == 1


# ------------------------------------------------------------------ the gain


def test_gain_of_a_planted_session(mc, dev):
    """estimate_gain_reference's gain (0 at defects) of a small session with a dead column, a hot and a stuck pixel:
    the filled gain equals the restatement bit for bit and is positive everywhere."""
    h, w = 33, 927
    rs = np.random.RandomState(3)
    sens = 0.8 + 0.4 * rs.rand(h, w)
    m = rs.poisson(40.0 * sens, size=(24, h, w)).clip(0, 255).astype(np.uint8)
    m[:, :, 311] = 0
    m[:, 7, 100] = 255
    m[:, 20, 600] = 41
    stats = mc.RawStatistics((h, w), device=dev).add(torch.from_numpy(m))
    gain, dmap = mc.estimate_gain_reference(stats, return_defect_map=True)
    planted = np.zeros((h, w), dtype=bool)
    planted[:, 311] = planted[7, 100] = planted[20, 600] = True
    assert np.array_equal(dmap.cpu().numpy(), planted) and not bool(gain[dmap].any())
    plan = mc.DefectFill(dmap)
    assert plan.device == dev and plan.n == h + 2
    got = mc.fill_defects_gain(gain, plan)
    assert got.dtype == torch.float32 and got.device == gain.device and got.data_ptr() != gain.data_ptr()
    assert torch.equal(bits(got), bits(dr.gain_fill(gain.cpu().numpy(), planted, 4)))
    assert float(got.min()) > 0 and not bool(gain[dmap].any())  # the input is left alone
    assert torch.equal(got[~dmap], gain[~dmap])
    assert torch.equal(mc.fill_defects_gain(gain, dmap), got)  # from the map itself


@pytest.mark.parametrize("name", list(MAPS))
def test_gain_equals_the_restatement_on_a_random_gain(mc, dev, plans, name):
    dmap, tb = table(name)
    gain = random_gain(*dmap.shape)
    want = bits(dr.gain_fill(gain.numpy(), dmap, 4, table=tb))
    got = mc.fill_defects_gain(gain.to(dev), plans[name])
    assert torch.equal(bits(got), want)
    cpu = mc.fill_defects_gain(gain, plans[name])  # a CPU gain comes back on the CPU
    assert cpu.device.type == "cpu" and torch.equal(bits(cpu), want)


# ------------------------------------------------------------------ in front of a raw route

ULP = 2.0 ** -24


def test_filled_movie_and_gain_through_motion_correct_raw(mc, dev):
    """A u8 movie of known whole-pixel drift with a dead column and three stuck pixels, gain ones:
    motion_correct_raw on the filled movie and the filled gain returns exactly the planted shifts, and its sum agrees
    with the sum of the filled movie's condition_movie -> estimate_global_motion -> motion_correct_sum route.

    The reference and the bound are those of tests/test_rigid_kernels_float64.py for a raw route: the float64 gather
    resampler of tests/rigid_reference.py on v = raw * gain - mu (mu = the kernels' fp32 frame means) at the shifts
    the route evaluates (the lattice over fp32(ps), read back), per frame 32 * 2^-24 * mag + the cubic weights' error
    term + the conditioning's two roundings, and for the sum those bounds added + t * 2^-24 * sum_f |ref_f|.  Each
    route's sum is held to that bound against the float64 sum, and the two sums to the same bound against each
    other at the former defects' positions."""
    from torch_motion_correction_amd import engine

    dy, dx = [-3, -5, 0, -6], [-6, -3, 0, -5]
    t, h, w = 4, 256, 4096
    raw = drifting_raw_movie(dy, dx, h, w, torch.uint8, seed=500)
    dmap = torch.zeros(h, w, dtype=torch.bool)
    dmap[:, 1000] = True
    stuck = ((17, 33), (100, 2000), (255, 4095))
    raw[:, :, 1000] = 0
    for y, x in stuck:
        dmap[y, x] = True
        raw[:, y, x] = 255
    plan = mc.DefectFill(dmap, device=dev)
    ones = torch.ones(h, w)
    filled = mc.fill_defects_raw(raw.to(dev), plan, seed=7)
    gain = mc.fill_defects_gain(ones.to(dev), plan)
    want_movie = dr.fill(raw.numpy(), dmap.numpy(), 4, 7)
    assert torch.equal(filled.cpu(), torch.from_numpy(want_movie)) and torch.equal(gain.cpu(), ones)
    assert int(filled[:, :, 1000].min()) > 0  # the stripe is gone

    field, total = mc.motion_correct_raw(filled, gain, 1.0)
    truth = torch.tensor([[a - dy[t // 2] for a in dy], [b - dx[t // 2] for b in dx]], dtype=torch.float32)
    assert torch.equal(field[:, :, 0, 0].cpu(), truth), field.flatten()

    img = mc.condition_movie(filled, gain)
    field_c = mc.estimate_global_motion(img, 1.0)
    total_c = mc.motion_correct_sum(img, field_c, 1.0)
    assert torch.equal(field_c, field)

    mu = engine.RawMovie(filled, gain).mu.cpu().numpy()
    sh = engine.frame_lattices(field, t, "catmull_rom")[:, :, 0, 0].cpu().numpy() / np.float32(1.0)
    ref, mag, err, wterm = rigid_resample_gather_stack(
        lambda f: condition_float64(want_movie[f], None, mu[f]), sh.astype(np.float32),
        extra=lambda f: conditioning_error(want_movie[f], None, mu[f]), weight_error=True)
    bound = 32 * ULP * mag + wterm + err
    sum_bound = bound.sum(0) + t * ULP * np.abs(ref).sum(0)
    r_raw = assert_sum(total, ref.sum(0), sum_bound, "motion_correct_raw on the filled movie")
    r_cond = assert_sum(total_c, ref.sum(0), sum_bound, "condition_movie route on the filled movie")
    at = dmap.numpy()
    r_both = assert_sum(total.cpu()[dmap], total_c.cpu().double().numpy()[at], sum_bound[at],
                        "raw route against the condition_movie route at the former defects")
    print(f"RATIO filled movie, |sum - float64| / bound: raw route {r_raw:.3f}, condition_movie route {r_cond:.3f}; "
          f"raw against conditioned at the defects / bound: {r_both:.3f}")


# ------------------------------------------------------------------ large movies


def _isolated_check(mc, dev, movie, seed):
    """Fills `movie` (t, h, w) in place with a map of isolated defects -- the first and the last pixel of the frame
    and eight more of the last row -- and checks every filled element of every frame against pick()
    applied to the donor values read back as single elements (donors are never written), the tables of the sampled
    defects against ring 1, and that the first and the last 4096 elements of the movie are otherwise untouched."""
    t, h, w = movie.shape
    defects = sorted({(0, 0), (h - 1, w - 1)} | {(h - 1, x) for x in (2, 77, 1001, w // 3, w // 2, w - 4097, w - 300,
                                                                     w - 3)})
    dmap = torch.zeros(h, w, dtype=torch.bool, device=dev)
    for y, x in defects:
        dmap[y, x] = True
    plan = mc.DefectFill(dmap)
    assert plan.n == len(defects) and plan.pixels.tolist() == [y * w + x for y, x in defects]
    donors, counts = plan.donors.cpu().numpy(), plan.counts.cpu().numpy()
    flat = movie.view(-1)
    head, tail = flat[:4096].clone(), flat[-4096:].clone()
    assert mc.fill_defects_raw(movie, plan, seed=seed, in_place=True) is movie
    torch.cuda.synchronize()
    hw = h * w
    for j, (y, x) in enumerate(defects):
        want = [yy * w + xx for yy, xx in dr.ring(y, x, 1, h, w)]  # isolated: all of ring 1
        assert counts[j] == len(want) and donors[j, :counts[j]].tolist() == want, (y, x)
        for f in range(t):
            d = want[dr.pick(seed, f, j, len(want))]
            assert int(flat[f * hw + y * w + x]) == int(flat[f * hw + d]), (f, y, x)
    filled_head = [f * hw + y * w + x for f in range(t) for y, x in defects if f * hw + y * w + x < 4096]
    filled_tail = [f * hw + y * w + x - (t * hw - 4096) for f in range(t) for y, x in defects
                   if f * hw + y * w + x >= t * hw - 4096]
    keep_head = torch.ones(4096, dtype=torch.bool, device=dev)
    keep_tail = keep_head.clone()
    keep_head[filled_head] = False
    keep_tail[filled_tail] = False
    assert len(filled_head) == 1 and len(filled_tail) == 3  # (0, 0) | the last three defects of the last row
    assert torch.equal(flat[:4096][keep_head], head[keep_head])
    assert torch.equal(flat[-4096:][keep_tail], tail[keep_tail])
    return plan


def test_large_frames(mc, dev):
    """(2, 8184, 11520) u8, the largest detector format: defects in the last row of the last frame."""
    t, h, w = 2, 8184, 11520
    movie = torch.empty((t, h, w), dtype=torch.uint8, device=dev)
    movie.view(-1).random_(0, 256)
    keep = movie.clone()
    _isolated_check(mc, dev, movie, seed=12345)
    changed = torch.nonzero((movie != keep).view(-1)).reshape(-1)
    assert int(changed.numel()) <= 2 * 10  # nothing but the 10 defects of each frame (a pick may equal the old value)
    assert int(changed.numel()) > 0


def _free_gpu_bytes():
    return torch.cuda.mem_get_info()[0]


def test_offsets_past_2_to_the_32(mc, dev):
    """Element and byte offsets beyond 32 bits, filled in place.  (2, 24577, 43691) u8: 2 147 587 414 elements, the
    second frame's last rows lie past 2^31 (a signed 32-bit element offset overflows).  (2, 32769, 32768) i16: the
    last element sits at byte offset 4 295 098 366 > 2^32 (an unsigned one does too)."""
    if _free_gpu_bytes() < 8 * 2**30:
        pytest.skip("less than 8 GB of GPU memory free")
    for shape, dtype in (((2, 24577, 43691), torch.uint8), ((2, 32769, 32768), torch.int16)):
        t, h, w = shape
        assert t * h * w > 2**31 and (dtype == torch.uint8 or 2 * t * h * w > 2**32)
        movie = torch.empty(shape, dtype=dtype, device=dev)
        movie.view(-1).random_(0, 256) if dtype == torch.uint8 else movie.view(-1).random_(-32768, 32768)
        _isolated_check(mc, dev, movie, seed=12345)
        del movie
        torch.cuda.empty_cache()
