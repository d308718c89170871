"""orient_raw on the GPU (mc_raw_orient, csrc/raw_orient.hip) against numpy.rot90 + numpy.flip
(tests/mrc_reference.py).  Elements are moved: torch.equal on the bits.  Every output lies inside a NaN-guarded
allocation (kernel_harness.byte_buffer) at an address aligned for its element and for nothing more."""

import numpy as np
import pytest
import torch

import mrc_reference as mr
from kernel_harness import assert_byte_guards, byte_buffer

pytestmark = pytest.mark.gpu

DTYPES = [torch.uint8, torch.int16, torch.float16, torch.float32]
# tile edges in both directions for every element size (tiles of 128, 64 and 32 elements), one row, one column, n > 1
SHAPES = [(1, 1), (1, 130), (130, 1), (65, 67), (3, 64, 128), (2, 33, 257)]
FLIPS = [None, "ud", "lr"]


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def values(shape, dtype, seed=0):
    """every element different from its neighbours: random bits (floats: any pattern, NaNs included)"""
    rng = np.random.default_rng([seed, *shape])
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[dtype.itemsize]
    raw = rng.integers(0, 2 ** (8 * dtype.itemsize), shape, dtype=np.uint64).astype(bits)
    return torch.from_numpy(raw.view({np.uint8: np.uint8, np.uint16: np.int16, np.uint32: np.int32}[bits])).view(dtype)


def as_bits(x):
    return x.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


def guarded(shape, dtype, dev):
    """An output of `shape` and `dtype` inside a NaN-filled allocation, starting three elements past a 16-byte boundary
    -> (the view, the whole allocation as bytes)"""
    view, whole = byte_buffer(int(np.prod(shape)) * dtype.itemsize, dev, past=3 * dtype.itemsize)
    view = view.view(dtype).view(*shape)
    assert view.data_ptr() % dtype.itemsize == 0 and view.data_ptr() % 16 != 0
    return view, whole


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_rotation_and_flip(mc, dev, dtype, shape):
    from torch_motion_correction_amd import mrc

    x = values(shape, dtype)
    bits = as_bits(x).numpy()
    on_dev = x.to(dev)
    for k in range(4):
        for flip in FLIPS:
            want = torch.from_numpy(mr.orient(bits, k, flip))
            what = f"{dtype} {shape} rot90 {k} flip {flip}"
            got = mc.orient_raw(on_dev, k, flip)
            assert got.dtype == dtype and got.device == dev and got.is_contiguous() and got.shape == want.shape, what
            assert got.data_ptr() != on_dev.data_ptr() and torch.equal(as_bits(got).cpu(), want), what
            out, whole = guarded(tuple(want.shape), dtype, dev)
            kk, ff = mrc._check_orient_args(on_dev, k, flip)
            res = mrc._orient(on_dev, kk, ff, dev, out=out)
            torch.cuda.synchronize()
            assert res.data_ptr() == out.data_ptr()
            assert_byte_guards(out, whole, what)
            assert torch.equal(as_bits(res).cpu(), want), what


def test_rot90_is_taken_mod_4_and_inputs_may_live_anywhere(mc, dev):
    x = values((2, 33, 70), torch.int16, seed=1)
    bits = x.numpy()
    for k in (-1, -6, 5, 4, 10**9 + 3):
        assert torch.equal(mc.orient_raw(x, k, "lr", device=dev).cpu(), torch.from_numpy(mr.orient(bits, k % 4, "lr")))
    # a CPU tensor, a non-contiguous view, a view at an odd element
    view = x.to(dev)[:, ::2, 1:]
    assert not view.is_contiguous()
    assert torch.equal(mc.orient_raw(view, 1, "ud").cpu(), torch.from_numpy(mr.orient(bits[:, ::2, 1:], 1, "ud")))
    flat = x.to(dev).reshape(-1)[1:1 + 33 * 69].view(33, 69)
    assert torch.equal(mc.orient_raw(flat, 3).cpu(), torch.from_numpy(mr.orient(bits.reshape(-1)[1:1 + 33 * 69]
                                                                               .reshape(33, 69), 3)))


@pytest.mark.parametrize("k,flip", [(k, f) for k in range(4) for f in FLIPS])
def test_a_gain_and_its_inverse_orientation(mc, dev, k, flip):
    from kernel_harness import gain as make_gain

    g = make_gain(67, 130).to(dev)
    there = mc.orient_raw(g, k, flip)
    assert torch.equal(there.cpu(), torch.from_numpy(mr.orient(g.cpu().numpy(), k, flip)))
    # undo the flip first (a flip is its own inverse), then turn back
    back = mc.orient_raw(mc.orient_raw(there, 0, flip), -k)
    assert back.shape == g.shape and torch.equal(back, g)
    # a defect map viewed as uint8 goes the same way
    defects = g > 2.0
    moved = mc.orient_raw(defects.view(torch.uint8), k, flip).view(torch.bool)
    assert torch.equal(moved.cpu(), torch.from_numpy(mr.orient(defects.cpu().numpy(), k, flip)))
