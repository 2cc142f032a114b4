"""The coin selection's batched subset search on the CPU (csrc/wallet/coinselect.cpp CoinSelectCpu,
the host twin of coin_select_kernel) against an independent Python implementation of the
algorithm fixed in csrc/kernels/coin_select.h: tuple for tuple and included set for included set."""
import struct

import pytest

import coin_select_cases as cases
from bitcoincashplus_amd import ops
from bitcoincashplus_amd.testing.messages import siphash24

M64 = (1 << 64) - 1


def oracle(values, target, trials, seed, run):
    """(total, trial, pass, index, included) of the smallest candidate, or None. Keeps the set of
    taken coins as the reference loop keeps vfIncluded."""
    k0, k1 = seed
    best = None
    for t in range(trials):
        words = {}

        def bit(i):
            w = i >> 6
            if w not in words:
                words[w] = siphash24(k0, (k1 + run) & M64, struct.pack("<Q", (t << 32) | w))
            return (words[w] >> (i & 63)) & 1

        total, taken, reached = 0, set(), False
        for pas in (0, 1):
            if pas == 1 and reached:
                break
            for i, v in enumerate(values):
                if (bit(i) == 1) if pas == 0 else (i not in taken):
                    total += v
                    taken.add(i)
                    if total >= target:
                        reached = True
                        if best is None or (total, t, pas, i) < best[:4]:
                            best = (total, t, pas, i, sorted(taken))
                        total -= v
                        taken.discard(i)
    return best


def twin(values, target, trials, seed, run):
    res = ops.coin_select(values, target, trials=trials, seed=seed, use_gpu=False, run=run)
    return None if res is None else (res[0], res[1], res[2], res[3], list(res[4]))


def check(case):
    values, target, trials, seed, run = case
    got = twin(values, target, trials, seed, run)
    assert got == oracle(values, target, trials, seed, run)
    cases.check_result(values, target, got)
    return got


@pytest.mark.parametrize("n", cases.COIN_COUNTS)
def test_twin_equals_oracle_coin_counts(n):
    assert check(cases.grid_case(n, 65)) is not None


@pytest.mark.parametrize("trials", cases.TRIAL_COUNTS)
def test_twin_equals_oracle_trial_counts(trials):
    assert check(cases.grid_case(130, trials)) is not None


@pytest.mark.parametrize("name", sorted(cases.shapes()))
def test_twin_equals_oracle_shapes(name):
    case = cases.shapes()[name]
    got = check(case)
    values, target = case[0], case[1]
    if name == "sum_below_target":
        assert got is None
    if name.startswith("exact"):
        assert got[0] == target
    if name == "all_equal_tie_break":
        # 15 coins of 7 make 105: every trial ties, trial 0 wins, at its fifteenth coin taken
        assert got[:2] == (105, 0) and len(got[4]) == 15
    if name == "pass1_forced":
        assert got[2] == 1 and got[0] in (sum(values), target)
    if name == "large_amounts":
        assert got[0] == 21 * 10 ** 14 * 501


def test_both_runs_are_two_single_runs():
    values = cases.random_values(130, 5)
    target = sum(values) // 4
    both = ops.coin_select(values, target, trials=65, seed=cases.SEED_WRAP, both_runs=True, use_gpu=False, min_change=12345)
    assert len(both) == 2
    assert both[0] == ops.coin_select(values, target, trials=65, seed=cases.SEED_WRAP, use_gpu=False, run=0)
    assert both[1] == ops.coin_select(values, target + 12345, trials=65, seed=cases.SEED_WRAP, use_gpu=False, run=1)
    assert both[1][:4] == oracle(values, target + 12345, 65, cases.SEED_WRAP, 1)[:4]
    # the runs draw different bits
    assert both[0][4] != ops.coin_select(values, target, trials=65, seed=cases.SEED_WRAP, use_gpu=False, run=1)[4]


def test_arguments_out_of_range(native):
    ok = dict(first_run=0, trials=10, k0=1, k1=2, use_gpu=False)
    assert native.coin_select([5, 3], [4], **ok)[0][0] == 5
    for values, targets, kw in (([], [4], {}), ([5, 0], [4], {}), ([5, -1], [4], {}), ([5, 3], [0], {}),
                                ([1 << 62, 1 << 62], [4], {}), ([5, 3], [4], dict(trials=0)),
                                ([5, 3], [4], dict(trials=65537)), ([5, 3], [4, 5], dict(first_run=1)),
                                ([5, 3], [], {})):
        with pytest.raises(ValueError):
            native.coin_select(values, targets, **{**ok, **kw})
    assert native.coin_select([5, 3], [4], **{**ok, "trials": 65536})[0][0] == 5


def test_option_and_counters_exist(native):
    st = native.coin_select_stats()
    assert st["threshold"] >= 2048 or st["threshold"] == 0
    assert {"gpu_selections", "cpu_selections", "gpu_failures"} <= set(st)
    assert "coin_select" in ops.__all__ and "coin_select" in ops.__doc__
