"""The coin selection's subset search on the GPU (csrc/kernels/coin_select.hip coin_select_kernel,
one lane per trial) against its CPU twin (csrc/wallet/coinselect.cpp, checked against a Python
oracle in tests/test_coin_select.py): the same (total, trial, pass, index) and the same coins,
exactly."""
import pytest

import coin_select_cases as cases
from bitcoincashplus_amd import ops

pytestmark = pytest.mark.gpu


def both(values, target, trials, seed, run):
    gpu = ops.coin_select(values, target, trials=trials, seed=seed, run=run)
    cpu = ops.coin_select(values, target, trials=trials, seed=seed, run=run, use_gpu=False)
    assert gpu == cpu
    cases.check_result(values, target, gpu)
    return gpu


@pytest.mark.parametrize("trials", cases.TRIAL_COUNTS)
@pytest.mark.parametrize("n", cases.COIN_COUNTS)
def test_kernel_equals_twin(n, trials):
    assert both(*cases.grid_case(n, trials)) is not None


@pytest.mark.parametrize("name", sorted(cases.shapes()))
def test_kernel_equals_twin_shapes(name):
    values, target, trials, seed, run = cases.shapes()[name]
    got = both(values, target, trials, seed, run)
    if name == "sum_below_target":
        assert got is None
    if name.startswith("exact"):
        assert got[0] == target
    if name == "all_equal_tie_break":
        assert got[:2] == (105, 0)
    if name == "pass1_forced":
        assert got[2] == 1
    # the same shape over sixteen waves: the winner may sit in any of them
    both(values, target, 1000, seed, run)


def test_tie_break_across_waves():
    """Equal amounts, a target no trial meets exactly: every trial of every wave ends at the same
    total, so the wave, workgroup and final reductions must all prefer the earliest trial."""
    got = both([7] * 130, 100, 1000, cases.SEED_WRAP, 0)
    assert got[:3] == (105, 0, 0)


def test_a_long_list_and_the_most_trials():
    values = cases.random_values(20000)
    both(values, sum(values) // 5, 1000, cases.SEED, 0)
    values = cases.random_values(300)
    both(values, sum(values) // 2, 65536, cases.SEED, 1)


def test_both_runs_equal_two_single_runs():
    values = cases.random_values(4097, 6)
    target = sum(values) // 4
    for trials in (65, 1000):
        pair = ops.coin_select(values, target, trials=trials, seed=cases.SEED_WRAP, both_runs=True, min_change=12345)
        assert len(pair) == 2
        assert pair[0] == ops.coin_select(values, target, trials=trials, seed=cases.SEED_WRAP, run=0)
        assert pair[1] == ops.coin_select(values, target + 12345, trials=trials, seed=cases.SEED_WRAP, run=1)
        assert pair == ops.coin_select(values, target, trials=trials, seed=cases.SEED_WRAP, both_runs=True, min_change=12345,
                                       use_gpu=False)
    # one run has a candidate, the other does not
    values = cases.random_values(65, 7)
    pair = ops.coin_select(values, sum(values), trials=65, seed=cases.SEED, both_runs=True, min_change=1)
    assert pair[0] is not None and pair[0][0] == sum(values) and pair[1] is None


def test_tensor_path_equals_host_path():
    import torch

    values = cases.random_values(4097, 8)
    target = sum(values) // 3
    x = torch.tensor(values, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        one = ops.coin_select(x, target, trials=1000, seed=cases.SEED)
        pair = ops.coin_select(x, target, trials=65, seed=cases.SEED, both_runs=True)
        none = ops.coin_select(x, sum(values) + 1, trials=65, seed=cases.SEED)
        # the stream goes on: later work on it sees the results
        after = one + 1
    side.synchronize()
    assert one.is_cuda and one.dtype == torch.int64 and one.shape == (4,) and pair.shape == (2, 4)
    host = ops.coin_select(values, target, trials=1000, seed=cases.SEED)
    assert tuple(one.tolist()) == host[:4]
    assert after.tolist() == [v + 1 for v in host[:4]]
    host_pair = ops.coin_select(values, target, trials=65, seed=cases.SEED, both_runs=True)
    assert [tuple(r) for r in pair.tolist()] == [r[:4] for r in host_pair]
    assert none.tolist() == [-1, -1, -1, -1]
    with pytest.raises(TypeError):
        ops.coin_select(x.to(torch.int32), target)
    with pytest.raises(ValueError):
        ops.coin_select(x, target, use_gpu=False)
