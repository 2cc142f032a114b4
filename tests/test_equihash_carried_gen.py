"""Equihash GPU solver: generation carried by the collision rounds of the previous nonce group.

BCP_EH_GROUPS=n (read when a solver is constructed) splits every launch into n nonce groups; the
stand-alone kernel generates group 0 and rounds 1..K-1 of each group generate the next one on
their generation waves. One group is the whole batch generated up front. A grouped solver must
return, nonce by nonce, what the one-group solver returns; which rows or pairs an overflowing
bucket or pair list drops follows the order of the atomics, so for a nonce with a drop in one solver
only the inclusion that still holds is checked (a solver without drops finds every solution the
other finds), and for a nonce with drops in both only that its solutions verify.

That the grouped solver really ran carrying rounds is asserted from its `carry_launches` stat: K-1
carrying round kernels for every group that has a next one.
"""
import struct

import pytest

pytestmark = pytest.mark.gpu


def header_input(nonce: int, salt: bytes = b"") -> bytes:
    # CEquihashInput (108 B) || nNonce (32 B), as tests/test_equihash.py builds it
    body = (salt + bytes(108))[:108]
    return body + struct.pack("<I", nonce) + bytes(28)


def _states(native, n, k, nonces, salt):
    out = []
    for nonce in nonces:
        st = native.EquihashState(n, k)
        st.update(header_input(nonce, salt))
        out.append(st)
    return out


def _solve(native, monkeypatch, n, k, batch, groups, states, debug=False):
    """Solve `states` in launches of `batch`; per nonce: (solutions, pair drops, row drops).
    Also returns the candidate drops and the solver (its last batch is still on the device)."""
    monkeypatch.setenv("BCP_EH_GROUPS", str(groups))
    solver = native.EquihashGpuSolver(n, k, batch)
    solver.set_debug(debug)
    per = []
    carrying = 0  # groups with a next group, over all launches
    for b0 in range(0, len(states), batch):
        chunk = states[b0:b0 + batch]
        res = solver.solve(chunk)
        st = solver.stats()
        if groups > 1:
            gsz = -(-len(chunk) // min(groups, batch))
            if gsz >= 8:
                gsz = -(-gsz // 8) * 8
            carrying += -(-len(chunk) // gsz) - 1
        assert st["carry_launches"] == carrying * (k - 1), (st["carry_launches"], carrying)
        assert len(st["pair_dropped_nonce"]) == len(chunk) == len(st["stage_dropped_nonce"])
        for sols, pd, rd in zip(res, st["pair_dropped_nonce"], st["stage_dropped_nonce"]):
            per.append((sols, pd, rd))
    return per, solver.stats()["cand_dropped"], solver


def _check_against(native, n, k, states, got, ref):
    """Every solution verifies; the solution sets are equal for every nonce without a drop in
    either solver, and a solver without a drop on a nonce finds all the other finds there.
    Returns the number of nonces compared for equality."""
    compared = 0
    for st, (gs, gpd, grd), (rs, rpd, rrd) in zip(states, got, ref):
        for s in gs:
            assert native.eh_is_valid_solution(n, k, st, s)[0]
        if gpd == 0 and grd == 0:
            assert set(rs) <= set(gs)
        if rpd == 0 and rrd == 0:
            assert set(gs) <= set(rs)
        if gpd == 0 and grd == 0 and rpd == 0 and rrd == 0:
            compared += 1
    return compared


@pytest.fixture(scope="module")
def ref_96_5(native):
    mp = pytest.MonkeyPatch()
    try:
        states = _states(native, 96, 5, range(8), b"gpu")
        per, cdrop, _ = _solve(native, mp, 96, 5, 4, 1, states)
    finally:
        mp.undo()
    return states, per, cdrop


@pytest.fixture(scope="module")
def ref_200_9(native):
    mp = pytest.MonkeyPatch()
    try:
        states = _states(native, 200, 9, range(16), b"main")
        per, cdrop, _ = _solve(native, mp, 200, 9, 16, 1, states)
    finally:
        mp.undo()
    return states, per, cdrop


@pytest.mark.parametrize("batch,groups", [(2, 2), (3, 3)])
def test_carried_generation_96_5(native, monkeypatch, ref_96_5, batch, groups):
    """(96,5), one nonce per group. The one-group solver drops nothing on these nonces (zero over
    10 repeats since the extra pair slot, profiles/equihash_r6.md), which is asserted. The grouped
    solver's pair list is as large ((5 + 1) * 256 = (7 + 1) * 192 pairs) and its areas are the
    same, so it must drop nothing either and all 8 nonces are compared."""
    states, ref, ref_cdrop = ref_96_5
    assert ref_cdrop == 0 and all(pd == 0 and rd == 0 for _, pd, rd in ref), [(pd, rd) for _, pd, rd in ref]
    got, cdrop, _ = _solve(native, monkeypatch, 96, 5, batch, groups, states)
    compared = _check_against(native, 96, 5, states, got, ref)
    print("compared", compared, "of", len(states), "candidate drops", cdrop)
    assert cdrop == 0 and all(pd == 0 and rd == 0 for _, pd, rd in got), [(pd, rd) for _, pd, rd in got]
    assert compared == len(states) == 8
    assert sum(len(s) for s, _, _ in got) > 0


@pytest.mark.parametrize("batch,groups", [(16, 2), (4, 2), (3, 2)])
def test_carried_generation_200_9(native, monkeypatch, ref_200_9, batch, groups):
    """(200,9): two groups of 8 (every nonce's kernels on one XCD), two groups of 2 (no XCD map),
    groups of 2 + 1 (carrying workgroups without a partner nonce). No row of these nonces is
    dropped (test_gpu_solver_200_9_no_overflow); nonces with a pair drop in either solver are not
    compared, and at least 12 of the 16 must be comparable."""
    states, ref, ref_cdrop = ref_200_9
    got, cdrop, _ = _solve(native, monkeypatch, 200, 9, batch, groups, states)
    assert ref_cdrop == 0 and cdrop == 0
    assert all(rd == 0 for _, _, rd in ref) and all(rd == 0 for _, _, rd in got)
    compared = _check_against(native, 200, 9, states, got, ref)
    print("comparable nonces", compared, "of 16; pair drops", [pd for _, pd, _ in got], [pd for _, pd, _ in ref])
    assert compared >= 12
    assert sum(len(s) for s, _, _ in got) >= 16  # ~1.9 per nonce


@pytest.mark.parametrize("n,k,nb,salt", [(96, 5, 128, b"gpu"), (200, 9, 512, b"main")])
def test_carried_stage0_equals_standalone(native, monkeypatch, n, k, nb, salt):
    """Nonce 1 of a batch of 2: generated by nonce 0's rounds (two groups) or by the stand-alone
    kernel (one group). The stage-0 bucket fills do not depend on the order of the atomics and
    must be equal; so must the set of leaf indices in the stage-0 slots. No stage-0 bucket of
    these nonces is past its capacity (asserted), so every leaf is in a slot."""
    import numpy as np
    states = _states(native, n, k, range(2), salt)
    _, _, carried = _solve(native, monkeypatch, n, k, 2, 2, states, debug=True)
    _, _, alone = _solve(native, monkeypatch, n, k, 2, 1, states, debug=True)
    fc, fa = carried.debug_fills(1)[:nb], alone.debug_fills(1)[:nb]
    assert fa == fc
    init = 1 << (n // (k + 1) + 1)
    assert sum(fa) == init
    assert carried.stats()["stage_dropped_nonce"][1] == 0 and alone.stats()["stage_dropped_nonce"][1] == 0

    def leaves(solver):
        dump = np.asarray(solver.debug_dump(1), dtype=np.uint64)
        stage0 = dump[:len(dump) // k]
        return np.sort(stage0[stage0 != np.uint64(0xFFFFFFFF)])

    lc, la = leaves(carried), leaves(alone)
    assert len(la) == init and np.array_equal(la, np.arange(init, dtype=np.uint64))
    assert np.array_equal(lc, la)
