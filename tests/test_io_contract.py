"""The I/O contract harness of test_io_contract_gpu.py bites (no GPU needed): check_regions is fed
host arenas in which one word was changed the way a wrong kernel would change it, and must name
the row, the column and the region; a payload with two channels swapped is told from the right
one. This is how a reader knows what the GPU tests detect without anyone running a broken kernel."""
import numpy as np
import pytest

from test_io_contract_gpu import IN_FILL, OUT_FILL, _host_arena, assert_same_bits, check_regions

C, N, LD_IN, LD_OUT = 3, 32, 32 + 36, 32 + 4


def _arenas():
    rng = np.random.default_rng(11)
    x = (rng.random((C, N)) * 2 - 1).astype(np.float32)
    y = (rng.random((C, N)) * 2 - 1).astype(np.float32)
    return x, y, _host_arena(C, LD_IN, IN_FILL, x), _host_arena(C, LD_OUT, OUT_FILL, y)


def test_clean_arenas_pass_and_return_the_payload():
    x, y, ia, oa = _arenas()
    got = check_regions(oa, C, N, OUT_FILL, ia.copy(), ia)
    assert got.dtype == np.float32 and got.shape == (C, N)
    assert_same_bits(got, y, "payload")
    # the layout: channels in rows 1..C, sentinels everywhere else, the input sentinel a quiet NaN
    assert np.array_equal(ia.view(np.float32)[1:C + 1, :N], x)
    assert (ia[0] == IN_FILL).all() and (ia[C + 1] == IN_FILL).all() and (ia[1:C + 1, N:] == IN_FILL).all()
    assert np.isnan(np.int32(IN_FILL).view(np.float32)) and IN_FILL & 0x00400000 and IN_FILL != OUT_FILL
    # in place inside one padded arena (B'): no separate input
    assert_same_bits(check_regions(ia, C, N, IN_FILL), x, "in-place payload")


@pytest.mark.parametrize("row,col,region", [(2, N, "output padding"), (1, LD_OUT - 1, "output padding"),
                                            (0, 5, "output guard row"), (C + 1, 0, "output guard row")])
def test_a_write_outside_the_output_is_named(row, col, region):
    _, _, ia, oa = _arenas()
    oa[row, col] = np.float32(0.0).view(np.int32)  # a stray zero, as a spare float4 store leaves
    with pytest.raises(AssertionError, match=f"row {row}, column {col} \\({region}\\)"):
        check_regions(oa, C, N, OUT_FILL, ia.copy(), ia)


@pytest.mark.parametrize("row,col,region", [(1, 7, "input payload"), (3, N + 2, "input padding"),
                                            (0, 0, "input guard row")])
def test_a_changed_input_word_is_named(row, col, region):
    _, _, ia, oa = _arenas()
    before = ia.copy()
    ia[row, col] ^= 1  # one bit: the comparison is on bit patterns, NaN sentinels included
    with pytest.raises(AssertionError, match=f"row {row}, column {col} \\({region}\\)"):
        check_regions(oa, C, N, OUT_FILL, before, ia)


def test_swapped_channel_rows_are_named():
    """the input rows of channels 0 and 1 swapped (an input used as scratch), and an output written
    with the channels in the wrong rows (a stride mixed up)"""
    x, y, ia, oa = _arenas()
    before = ia.copy()
    ia[[1, 2]] = ia[[2, 1]]
    with pytest.raises(AssertionError, match=r"row 1, column 0 \(input payload\)"):
        check_regions(oa, C, N, OUT_FILL, before, ia)
    oa[[1, 2]] = oa[[2, 1]]
    got = check_regions(oa, C, N, OUT_FILL)  # every word is inside the payload: the regions pass
    with pytest.raises(AssertionError, match="first at channel 0, column 0"):
        assert_same_bits(got, y, "B")


def test_a_padding_read_poisons_the_payload():
    """what a kernel that sums one column past the block would produce is not equal to anything"""
    x, _, ia, _ = _arenas()
    poisoned = x.copy()
    poisoned[1, N - 1] += ia.view(np.float32)[2, N]
    assert np.isnan(poisoned[1, N - 1])
    with pytest.raises(AssertionError, match="first at channel 1, column 31"):
        assert_same_bits(poisoned, x, "B")
