"""lnw.keyed's uniforms on the GPU against direct lnw_fill_uniform_f32 calls
written out here: the absolute offset slot * 2^40 + row * (values per row), the
cut of a fill that starts inside a Philox block, the seed taken modulo 2^64 and
the empty result of no rows. The shapes are the smallest at which that
arithmetic can go wrong."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MASK = 2 ** 64 - 1


def direct_fill(count, seed, offset):
    """`count` floats of the Philox stream from absolute `offset` (a multiple of 4)."""
    from lnw import _abi
    L = _abi.load()
    u = torch.empty(count, dtype=torch.float32, device="cuda")
    _abi.check(L.lnw_fill_uniform_f32(u.data_ptr(), count, seed, offset,
                                      torch.cuda.current_stream(u.device).cuda_stream))
    return u


def direct_uniform4(row0, rows, seed, slot):
    """keyed_uniform4's body before it became keyed_uniform(cols=2)."""
    u = torch.empty((rows, 4), dtype=torch.float32, device="cuda")
    if rows:
        u = direct_fill(rows * 4, int(seed) & MASK, (int(slot) << 40) + 4 * int(row0)).reshape(rows, 4)
    return u


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("slot", [0, 13])
@pytest.mark.parametrize("row0", [0, 3, 2 ** 20 + 1])
@pytest.mark.parametrize("rows", [0, 1, 7])
def test_uniform4_equals_direct_fill(rows, row0, slot):
    from lnw.qlearn import keyed_uniform4
    got = keyed_uniform4(row0, rows, 2024, slot, "cuda")
    assert got.shape == (rows, 4) and same_bits(got, direct_uniform4(row0, rows, 2024, slot))


@pytest.mark.parametrize("seed", [2 ** 63 + 5, -3])
def test_uniform4_seed_is_taken_modulo_2_64(seed):
    from lnw.qlearn import keyed_uniform4
    got = keyed_uniform4(3, 7, seed, 13, "cuda")
    assert same_bits(got, direct_uniform4(3, 7, seed, 13))
    assert same_bits(got, keyed_uniform4(3, 7, seed & MASK, 13, "cuda"))
    assert not same_bits(got, keyed_uniform4(3, 7, 2024, 13, "cuda"))


def test_uniform_cuts_the_lead_of_an_odd_offset():
    """Row 1 of 2 * 7141 values starts at offset 14282 = 4 * 3570 + 2: the fill
    starts two values below and the lead is cut."""
    from lnw.rollout import keyed_uniform
    rows, cols, seed, slot = 3, 7141, 2 ** 63 + 5, 13
    off = (slot << 40) + 1 * 2 * cols
    assert off & 3 == 2
    want = direct_fill(2 + rows * 2 * cols, seed, off - 2)[2:].reshape(rows, 2 * cols)
    assert same_bits(keyed_uniform(1, rows, cols, seed, slot, "cuda"), want)
