"""GPU suite: the ordered mask expansion (tavb_mask_expand / tavb_mask_pack, csrc/tavb_mask.hip) through `Engine.mask_to_rows` --
the allowed rows of a bit mask as an ascending int32 list in device memory, equal to np.flatnonzero in order and count, at every row
count where a word, a wave, a round of the workgroup or a workgroup chunk ends, from a host mask and from a device torch.bool tensor."""

import ctypes

import numpy as np
import pytest
import torch

from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

C = _native.MASK_ROWS_PER_WORKGROUP  # rows one workgroup covers
ROWS = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, C - 1, C, C + 1, 3 * C + 17]
KINDS = ["none", "all", "first", "last", "alternating", "random_0.01", "random_0.5", "last_word"]


@pytest.fixture(scope="module")
def eng():
    e = _native.Engine()
    yield e
    e.close()


def make_mask(kind: str, rows: int) -> np.ndarray:
    m = np.zeros(rows, dtype=bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind.startswith("random_"):
        m = np.random.default_rng(rows).random(rows) < float(kind.split("_")[1])
    elif kind == "last_word":
        m[(rows - 1) // 32 * 32:] = True  # only the bits of the last (partial) word
    return m


def check(dev_rows, count, mask):
    want = np.flatnonzero(mask)
    assert count == len(want)
    assert dev_rows.dtype == torch.int32 and dev_rows.is_cuda and tuple(dev_rows.shape) == (len(want),)
    np.testing.assert_array_equal(dev_rows.cpu().numpy(), want.astype(np.int32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", ROWS)
def test_expansion_equals_flatnonzero(eng, rows, kind):
    mask = make_mask(kind, rows)
    check(*eng.mask_to_rows(mask), mask)  # packed on the host
    dev_mask = torch.from_numpy(mask).to(f"cuda:{eng.device}")
    check(*eng.mask_to_rows(dev_mask), mask)  # packed on the device
    check(*eng.mask_to_rows(dev_mask.to(torch.uint8) > 0), mask)  # a mask computed on the device


@pytest.mark.parametrize("rows", ROWS)
def test_bits_at_or_beyond_rows_are_ignored(eng, rows):
    for kind in ("none", "random_0.5", "last_word"):
        mask = make_mask(kind, rows)
        words = _native.pack_mask_bits(mask).copy()
        if rows & 31:
            words[-1] |= np.uint32((0xFFFFFFFF << (rows & 31)) & 0xFFFFFFFF)  # every tail bit set
        # ... and a further all-ones word behind the last one: not part of the mask
        bits = torch.from_numpy(np.concatenate([words, np.array([0xFFFFFFFF], np.uint32)]).view(np.int32)).to(f"cuda:{eng.device}")
        check(*eng.expand_mask_bits(bits, rows), mask)
        check(*eng.expand_mask_bits(bits, rows, cap=int(mask.sum())), mask)


def test_input_forms_are_checked(eng):
    with pytest.raises(TypeError):
        eng.mask_to_rows(np.ones(10, dtype=np.uint8))
    with pytest.raises(TypeError):
        eng.mask_to_rows(torch.ones(10, dtype=torch.uint8, device=f"cuda:{eng.device}"))
    with pytest.raises(ValueError):
        eng.mask_to_rows(torch.ones(10, dtype=torch.bool))  # a host tensor is not a device mask
    dev_rows, count = eng.mask_to_rows(np.zeros(0, dtype=bool))
    assert count == 0 and dev_rows.numel() == 0


@pytest.mark.parametrize("rows", [33, 2049, C + 1])
def test_a_capacity_one_short_of_the_count_is_an_error_and_nothing_is_written_past_it(eng, rows):
    mask = make_mask("random_0.5", rows)
    count = int(mask.sum())
    bits = torch.from_numpy(_native.pack_mask_bits(mask).view(np.int32)).to(f"cuda:{eng.device}")
    with pytest.raises(ValueError, match=f"the mask has {count} rows set, dev_rows_out holds {count - 1}"):
        eng.expand_mask_bits(bits, rows, cap=count - 1)
    out = torch.full((count + 8,), -7, dtype=torch.int32, device=f"cuda:{eng.device}")
    torch.cuda.synchronize()
    got = ctypes.c_int64(0)
    rc = eng.lib.tavb_mask_expand(eng._h, ctypes.c_void_p(bits.data_ptr()), rows, ctypes.c_void_p(out.data_ptr()), count - 1, ctypes.byref(got))
    assert rc == -1 and got.value == count
    host = out.cpu().numpy()
    np.testing.assert_array_equal(host[: count - 1], np.flatnonzero(mask)[: count - 1])
    assert (host[count - 1:] == -7).all()
