"""Shapes for the coin selection's subset search (csrc/kernels/coin_select.h), shared by
tests/test_coin_select.py (the CPU twin against a Python oracle) and tests/test_coin_select_gpu.py
(the kernel against the twin). A case is (values, target, trials, seed, run)."""
import random

# word boundaries of the random words (64 coins each), a tail shorter than the kernel's unrolled
# group of 16, and 64 whole words plus one coin
COIN_COUNTS = [1, 2, 63, 64, 65, 130, 4097]
# a partial wave, exactly one wave, a second wave (one lane of it), sixteen waves with a partial last
TRIAL_COUNTS = [1, 63, 64, 65, 1000]
SEED = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
SEED_WRAP = (0x736F6D6570736575, 0xFFFFFFFFFFFFFFFF)  # k1 + run wraps to 0 in run 1


def random_values(n, seed=1):
    rng = random.Random(1000 * n + seed)
    return sorted((rng.randrange(1, 10 ** 8) for _ in range(n)), reverse=True)


def grid_case(n, trials):
    v = random_values(n)
    return v, max(1, sum(v) // 3), trials, SEED, 0


def shapes():
    out = {}
    pow2 = [1 << k for k in range(9, -1, -1)]
    out["exact_powers_of_two"] = (pow2, (1 << 8) + (1 << 5) + (1 << 3) + 1, 1000, SEED, 0)
    out["exact_equal_values"] = ([5000] * 65, 3 * 5000, 64, SEED, 0)
    out["all_equal_tie_break"] = ([7] * 130, 100, 65, SEED, 0)  # every trial ends at 105
    v = random_values(130, 2)
    out["pass1_forced"] = (v, sum(v) - min(v), 65, SEED, 0)
    out["large_amounts"] = ([21 * 10 ** 14] * 1000, 21 * 10 ** 14 * 500 + 1, 64, SEED, 0)
    v = random_values(65, 3)
    out["sum_below_target"] = (v, sum(v) + 1, 65, SEED, 0)
    v = random_values(130, 4)
    out["run1"] = (v, sum(v) // 2, 65, SEED, 1)
    out["run1_key_wraps"] = (v, sum(v) // 2, 65, SEED_WRAP, 1)
    return out


def check_result(values, target, res):
    """What any result must satisfy: the set sums to the total, the total reaches the target, and
    the last coin taken is needed (every coin of a descending list that is worth less than the
    excess came before it, so the set without the last coin is below the target)."""
    if res is None:
        assert sum(values) < target
        return
    total, trial, pas, index, included = res
    included = list(included)
    assert included == sorted(set(included)) and index in included
    assert sum(values[i] for i in included) == total
    assert total >= target
    assert total - values[index] < target
    assert pas in (0, 1) and 0 <= index < len(values)
