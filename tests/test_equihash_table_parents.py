"""Equihash GPU solver: the "table parents" stage layout of (200,9).

Stages 1, 2, 3, 4, 6 and 7 of (200,9) keep no parent word in their slots: the slot is the row with
the producing bucket d in its padding bits, the (j << 16 | i) word of output ordinal t goes to a
pair table P[stage][nonce][d][t], and a run-base table B[stage][nonce][d][b] turns a slot's
position in area b back into t. Only the tree expansion and DebugDump read P and B. (96,5) and
(48,5) prune from round 2 and never use the layout, so every case here is (200,9) at tiny batches.
"""
import concurrent.futures as cf
import struct

import pytest

pytestmark = pytest.mark.gpu

N, K, NB, AREA = 200, 9, 512, 6016


def header_input(nonce: int, salt: bytes = b"") -> bytes:
    # CEquihashInput (108 B) || nNonce (32 B), as tests/test_equihash.py builds it
    body = (salt + bytes(108))[:108]
    return body + struct.pack("<I", nonce) + bytes(28)


@pytest.fixture(scope="module")
def main16(native):
    """Nonces 0-15 of the b"main" inputs and the CPU solver's solution set of each."""
    states = []
    for nonce in range(16):
        st = native.EquihashState(N, K)
        st.update(header_input(nonce, b"main"))
        states.append(st)
    with cf.ThreadPoolExecutor(8) as ex:  # the binding releases the GIL
        cpu = list(ex.map(lambda st: set(native.eh_solve_cpu(N, K, st)[0]), states))
    assert sum(map(len, cpu)) >= 16  # ~1.7-1.9 per nonce
    return states, cpu


@pytest.mark.parametrize("batch,groups", [(3, 1), (16, 2)])
def test_table_parents_solutions_200_9(native, monkeypatch, main16, batch, groups):
    """Batch 3 in one group (plain kernels, no XCD mapping) and batch 16 in two groups of 8
    (carrying kernels, XCD mapping): every solution verifies and is one of the CPU solver's, at
    least 97% of the CPU's are found, and nothing is dropped at a candidate list or a bucket."""
    states, cpu = main16
    monkeypatch.setenv("BCP_EH_GROUPS", str(groups))
    solver = native.EquihashGpuSolver(N, K, batch)
    total = 0
    carrying = 0
    for b0 in range(0, 16, batch):
        chunk = states[b0:b0 + batch]
        res = solver.solve(chunk)
        if groups > 1:
            carrying += 1  # 16 nonces in two groups of 8: one group has a next one
        for st, sols, c in zip(chunk, res, cpu[b0:]):
            for s in sols:
                assert native.eh_is_valid_solution(N, K, st, s)[0]
                assert s in c
            total += len(sols)
    stats = solver.stats()
    cpu_total = sum(map(len, cpu))
    print("gpu", total, "cpu", cpu_total, "pair drops", stats["pair_dropped_all"], "row drops", stats["stage_dropped_all"])
    assert total >= 0.97 * cpu_total, (total, cpu_total)
    assert stats["cand_dropped"] == 0
    assert sum(stats["stage_dropped_all"]) == 0, stats["stage_dropped_all"]
    assert stats["carry_launches"] == carrying * (K - 1)
    if groups > 1:
        assert stats["carry_launches"] > 0  # the carrying kernels really ran


def test_table_parents_tree_dump_200_9(native, main16):
    """Batch 1, debug mode: every written slot of stages 1..8 names a producing bucket < 512 and
    two different LDS rows < 6016 of it, and more than a quarter of each stage's slots are
    written (test_gpu_solver_tree_dump_96_5's assertion on the layout that test cannot reach)."""
    import numpy as np
    states, _ = main16
    solver = native.EquihashGpuSolver(N, K, 1)
    solver.set_debug(True)
    for s in solver.solve(states[:1])[0]:
        assert native.eh_is_valid_solution(N, K, states[0], s)[0]
    dump = np.asarray(solver.debug_dump(), dtype=np.uint64).reshape(K, NB * AREA)
    for stage in range(1, K):
        tri = dump[stage][dump[stage] != np.uint64((1 << 64) - 1)]
        assert len(tri) > NB * AREA // 4, stage
        d, i, j = tri >> np.uint64(32), tri & np.uint64(0xFFFF), (tri >> np.uint64(16)) & np.uint64(0xFFFF)
        bad = (d >= NB) | (i >= AREA) | (j >= AREA) | (i == j)
        assert not bad.any(), (stage, [hex(int(x)) for x in tri[bad][:8]])


def test_table_parents_expand_rejects_corrupt_tables(native):
    """The tree expansion range-checks every step of the table walk. Mode 3 plants an out-of-range
    producing bucket in the padding of a stage-(K-2) parent row of the first candidate, mode 4 a
    run base that puts the slot's ordinal past its pair table; only the expansion is re-run. The
    corrupted candidate is rejected, no other turns valid, and the nonce then solves as before."""
    solver = native.EquihashGpuSolver(N, K, 1)
    for nonce in range(64):
        st = native.EquihashState(N, K)
        st.update(header_input(nonce, b"expand-probe"))
        first = solver.solve([st])
        base = solver.debug_expand_corrupt(0)
        if len(base) >= 2:
            break
    assert len(base) >= 2, "no nonce with two final-round candidates"
    for mode in (3, 4):
        solver.solve([st])  # fresh, uncorrupted stage arrays (candidate order varies per solve)
        base = solver.debug_expand_corrupt(0)
        got = solver.debug_expand_corrupt(mode)
        assert got[0] == 0, (mode, got[:4])  # the corrupted candidate is rejected
        # no other candidate turns valid (one sharing the corrupted slot may turn invalid too)
        assert all(g <= b for g, b in zip(got[1:], base[1:]))
    # the same nonce solves to the same solutions (compared as sets: a nonce's solutions are unordered)
    assert [sorted(x) for x in solver.solve([st])] == [sorted(x) for x in first]
