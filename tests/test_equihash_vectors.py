"""Constructed near-valid Equihash solutions (tests/equihash_vectors.py, docs/EQUIHASH_VECTORS.md)
through the CPU verifier and every GPU path of eh_verify (csrc/kernels/equihash_verify.hip).

The expected masks come from R.check_mask, the property oracle in
bitcoincashplus_amd/utils/equihash_ref.py, never from the code under test. GPU entry points:
  * native.eh_verify_reasons_gpu -> EquihashVerifyReasons -> verify_lane with the kernel's `why`
    output: the mask itself, vector for vector;
  * native.eh_verify_batch_gpu -> EquihashVerifyBatch -> the same lane with why = nullptr;
  * native.eh_check_headers_gpu -> CheckHeaders -> eh_state_kernel + eh_verify: SOLUTION_VALID;
  * native.gpu_verify_equihash -> GpuVerifyService::Equihash -> VerifyLane::Equihash.
The (200,9) accept side comes from the GPU solver, so without a GPU that set has only the families
that need no valid solution (P, N, Z, G); the gpu-marked tests build the whole set and also run the
CPU checks on it.
"""
import pytest

import equihash_vectors as ev
from bitcoincashplus_amd.utils import equihash_ref as R

SOLUTION_VALID, HASH_VALID = 1, 8
REGTEST_LIMIT = b"\xff" * 31 + b"\x7f"
HEADER_PARAMS = [(48, 5), (96, 5), (200, 9)]

_SETS = {}


def vector_set(native, n, k, gpu=False):
    """Built once per process; the GPU build of (200,9) replaces the material-free one."""
    key = (n, k, gpu and (n, k) == (200, 9))
    if key not in _SETS:
        _SETS[key] = ev.build(native, n, k, gpu=gpu)
    return _SETS[key]


def _state(native, n, k, data):
    st = native.EquihashState(n, k)
    st.update(data)
    return st


def _check(what, labels, got, expect):
    """Fails with one line per vector whose result is not the expected one."""
    assert len(got) == len(expect) == len(labels)
    bad = [f"  {labels[i]}: got {got[i]}, expected {expect[i]}" for i in range(len(expect)) if got[i] != expect[i]]
    if bad:
        pytest.fail(f"{what}: {len(bad)} of {len(expect)} differ\n" + "\n".join(bad[:80]), pytrace=False)


# ------------------------------------------------------------------ CPU
def _cpu_checks(native, vs):
    """mask == 0 <=> R.is_valid_solution <=> the CPU verifier, for every vector; the CPU verifier's
    reason for the vectors of the isolating families whose mask is the isolated bit alone."""
    n, k = vs.n, vs.k
    states = {}
    labels, oracle, cpu, expect, why, reasons = [], [], [], [], [], []
    for v in vs.vectors:
        st = states.get(v.data)
        if st is None:
            st = states[v.data] = _state(native, n, k, v.data)
        ok, reason = native.eh_is_valid_solution(n, k, st, v.soln)
        labels.append(v.label)
        expect.append(v.mask == 0)
        oracle.append(R.is_valid_solution(n, k, v.data, v.soln))
        cpu.append(bool(ok))
        fam = v.label.split(".")[0]
        if v.mask == ev.LENGTH or (fam in ev.ISOLATES and v.mask == ev.ISOLATES[fam]):
            why.append((v.label, reason, ev.REASON[v.mask]))
        reasons.append(reason)
    _check(f"({n},{k}) R.is_valid_solution against check_mask == 0", labels, oracle, expect)
    _check(f"({n},{k}) CPU verifier against check_mask == 0", labels, cpu, expect)
    assert all((r == "") == ok for r, ok in zip(reasons, cpu))
    _check(f"({n},{k}) CPU verifier's reason", [w[0] for w in why], [w[1] for w in why], [w[2] for w in why])
    return len(why)


def _count_checks(vs):
    n, k, p = vs.n, vs.k, vs.p
    counts = vs.counts()
    print(f"({n},{k}): {len(vs.vectors)} vectors in {vs.seconds:.1f} s: {counts}; {vs.notes}")
    least = ev.min_counts(n, k, vs.material, vs.wagner)
    assert set(counts) == set(least), (counts, least)
    for f, c in least.items():
        assert counts[f] >= c, (f, counts[f], c)
    assert len({v.label for v in vs.vectors}) == len(vs.vectors)
    assert all(len(v.data) == 140 for v in vs.vectors)
    # Z's all-zero list is what verify_lane puts in place of a solution of another length
    assert any(v.soln == bytes(p.width) and v.mask == ev.ORDER | ev.DUP for v in vs.family("Z"))
    assert sorted(v.mask for v in vs.vectors if len(v.soln) != p.width) == [ev.LENGTH] * 2
    if vs.material:
        # every level in S (right-child swaps and the root: mask exactly ORDER) and in X, where at
        # least 90% of each level's vectors have mask exactly COLLISION
        right = [v for v in vs.family("S") if not v.label.startswith("S.left.")]
        assert all(v.mask == ev.ORDER for v in right)
        assert {int(v.label.split(".")[2][1:]) for v in right} == set(range(k))
        assert {int(v.label.split(".")[2][1:]) for v in vs.family("S") if v.label.startswith("S.left.")} == set(range(k - 1))
        for l in range(k - 1):
            level = [v for v in vs.family("X") if v.label.split(".")[2] == f"l{l}"]
            assert level and sum(v.mask == ev.COLLISION for v in level) >= 0.9 * len(level), (l, len(level))
        assert all(v.mask & ev.DUP for v in vs.family("D"))
        assert sum(v.label.startswith("G.graft.") for v in vs.vectors) == (0 if any(s.startswith("G:") for s in vs.notes) else k)
        assert {v.mask for v in vs.family("V")} == {0}
    if vs.wagner:
        assert all(v.mask == ev.FINAL for v in vs.family("F")) and all(v.mask == ev.COLLISION for v in vs.family("T"))
    assert all(v.mask == ev.DUP for v in vs.family("U"))
    # the pair-tiled lists: the colliding ones exactly ORDER|DUP, each with a twin that has COLLISION too
    tiled = vs.family("P")
    # and the tiled near-collisions: a bit away from colliding at one level below the top; at the top
    # level and in the last digit the lists are whole trees, with whatever else the oracle finds
    near = vs.family("N")
    tiled += [v for v in near if not v.label.startswith((f"N.l{k - 1}.", "N.final."))]
    assert all(v.mask == (ev.ORDER | ev.DUP if ".collide" in v.label else ev.COLLISION | ev.ORDER | ev.DUP) for v in tiled)
    assert all(v.mask & ev.COLLISION for v in near if v.label.startswith(f"N.l{k - 1}."))
    assert all(v.mask & ev.FINAL and not v.mask & ev.COLLISION for v in near if v.label.startswith("N.final."))
    if (n, k) in ((200, 9), (96, 3)):
        levels = {v.label.split(".")[1] for v in near}
        assert levels == {f"l{l}" for l in range(1, k)} | {"final"}, levels
    if (n, k) != (96, 3):
        assert sum(".collide." in v.label for v in tiled) >= 1


@pytest.mark.parametrize("n,k", ev.PARAMS)
def test_cpu_verdicts(native, n, k):
    vs = vector_set(native, n, k)
    isolating = _cpu_checks(native, vs)
    assert isolating >= 2 + (3 * k + 128 if vs.wagner else 0)


@pytest.mark.parametrize("n,k", ev.PARAMS)
def test_vector_counts(native, n, k):
    _count_checks(vector_set(native, n, k))


def test_check_mask_is_not_early_exit():
    """check_mask reports every failing property at once: a random list fails collision, order and
    the final digit together, and appending a copy of an index adds DUP without hiding the rest."""
    p = ev.Params(48, 5)
    data = ev.header_input(0)
    lst = [5, 3] + list(range(100, 130))
    mask = R.check_mask(48, 5, data, p.pack(lst))
    assert mask & ev.ORDER and mask & ev.COLLISION and not mask & ev.DUP
    lst[31] = lst[30]
    assert R.check_mask(48, 5, data, p.pack(lst)) & (ev.ORDER | ev.COLLISION | ev.DUP) == ev.ORDER | ev.COLLISION | ev.DUP
    assert R.check_mask(48, 5, data, p.pack(lst)[:-1]) == ev.LENGTH


# ------------------------------------------------------------------ GPU
def _arrange(vs, how):
    """(labels, inputs, solutions, masks) of one batch: as built, reversed, or every vector followed
    by a valid solution, so that an accepting workgroup runs next to every rejecting one."""
    items = [(v.label, v.data, v.soln, v.mask) for v in vs.vectors]
    if how == "reversed":
        items = items[::-1]
    elif how == "interleaved":
        valid = [(f"valid.{i}", d, s, 0) for i, (d, s) in enumerate(vs.valid)]
        assert valid
        items = [x for i, it in enumerate(items) for x in (it, valid[i % len(valid)])]
    return tuple(list(col) for col in zip(*items))


def _states(native, n, k, datas):
    made = {d: _state(native, n, k, d) for d in set(datas)}
    return [made[d] for d in datas]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["in_order", "reversed", "interleaved"])
@pytest.mark.parametrize("n,k", ev.PARAMS)
def test_gpu_reasons(native, n, k, how):
    """The kernel's mask and eh_verify_batch_gpu's verdict for the whole set, in one arrangement."""
    vs = vector_set(native, n, k, gpu=True)
    labels, datas, sols, masks = _arrange(vs, how)
    states = _states(native, n, k, datas)
    got = native.eh_verify_reasons_gpu(n, k, states, sols)
    _check(f"({n},{k}) {how}: eh_verify_reasons_gpu", labels, list(got), masks)
    ok = native.eh_verify_batch_gpu(n, k, states, sols)
    _check(f"({n},{k}) {how}: eh_verify_batch_gpu", labels, [bool(x) for x in ok], [m == 0 for m in masks])


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", HEADER_PARAMS)
def test_gpu_check_headers(native, n, k):
    """SOLUTION_VALID of the whole-header check (base states made on the device by
    eh_state_kernel) from each vector's own 140-byte input; HASH_VALID clear for a wrong length."""
    vs = vector_set(native, n, k, gpu=True)
    labels, datas, sols, masks = _arrange(vs, "interleaved")
    status, _ = native.eh_check_headers_gpu(n, k, datas, sols, REGTEST_LIMIT)
    _check(f"({n},{k}) SOLUTION_VALID", labels, [bool(s & SOLUTION_VALID) for s in status], [m == 0 for m in masks])
    _check(f"({n},{k}) HASH_VALID", labels, [bool(s & HASH_VALID) for s in status], [m != ev.LENGTH for m in masks])


@pytest.mark.gpu
def test_gpu_verify_service(native):
    """The node's verify service (VerifyLane::Equihash on its lanes) on the (48,5) set."""
    vs = vector_set(native, 48, 5, gpu=True)
    labels, datas, sols, masks = _arrange(vs, "in_order")
    got = native.gpu_verify_equihash(48, 5, _states(native, 48, 5, datas), sols)
    _check("(48,5) gpu_verify_equihash", labels, [bool(x) for x in got], [m == 0 for m in masks])


@pytest.mark.gpu
def test_cpu_verdicts_200_9_full(native):
    """The CPU checks and the counts on the whole (200,9) set, whose accept side needs the GPU solver."""
    vs = vector_set(native, 200, 9, gpu=True)
    assert vs.material == 3
    _count_checks(vs)
    _cpu_checks(native, vs)
