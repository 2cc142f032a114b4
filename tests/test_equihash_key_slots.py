"""Equihash GPU solver: the "slot rounds" (EhCfg::ks).

Rounds 3-8 of (200,9) and every collision round of (96,5) have no key sort: the commit writes each
row's id into slot `rank` of its key (8 slots per key), a row then reads all its partners with one
16-byte LDS load, and the rows whose key already holds 8 go through a small overflow list. Rounds
1-2 of (200,9), the final rounds and (48,5) keep the sort. Plain and carrying kernels are separate
instantiations, so both run here, and `overflow_rows_all` (rows that went through the list, per
round) shows that the overflow path ran: about a seventh of the solutions pass through such a row.
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


def cpu_sets(native, n, k, states):
    with cf.ThreadPoolExecutor(8) as ex:  # the binding releases the GIL
        return list(ex.map(lambda st: set(native.eh_solve_cpu(n, k, st)[0]), states))


@pytest.fixture(scope="module")
def main16(native):
    """Nonces 0-15 of the b"main" inputs and the CPU solver's solution set of each."""
    states = []
    for nonce in range(16):
        st = native.EquihashState(N, K)
        st.update(header_input(nonce, b"main"))
        states.append(st)
    cpu = cpu_sets(native, N, K, states)
    assert sum(map(len, cpu)) >= 16  # ~1.7-1.9 per nonce
    return states, cpu


@pytest.mark.parametrize("batch,groups", [(3, 1), (16, 2)])
def test_key_slots_solutions_200_9(native, monkeypatch, main16, batch, groups):
    """Batch 3 in one group (plain slot rounds 3-8, sorted rounds 1-2) and batch 16 in two groups
    of 8 (carrying slot rounds): every solution verifies and is one of the CPU solver's, at least
    97% of the CPU's are found, nothing is dropped at a bucket or the candidate list, and every
    slot round sent rows through its overflow list."""
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
    print("gpu", total, "cpu", cpu_total, "pair drops", stats["pair_dropped_all"], "row drops", stats["stage_dropped_all"],
          "overflow rows", stats["overflow_rows_all"], "most in a bucket", stats["overflow_bucket_max"])
    assert total >= 0.97 * cpu_total, (total, cpu_total)
    assert stats["cand_dropped"] == 0
    assert sum(stats["stage_dropped_all"]) == 0, stats["stage_dropped_all"]
    assert stats["carry_launches"] == carrying * (K - 1)
    if groups > 1:
        assert stats["carry_launches"] > 0  # the carrying kernels really ran
    ovf, most = stats["overflow_rows_all"], stats["overflow_bucket_max"]
    assert len(ovf) == K + 1 and len(most) == K + 1
    for rnd in range(1, K + 1):
        if 3 <= rnd <= 8:
            assert ovf[rnd] > 0 and 0 < most[rnd] <= ovf[rnd], (rnd, ovf, most)
        else:  # rounds 1, 2 and the final round sort their keys
            assert ovf[rnd] == 0 and most[rnd] == 0, (rnd, ovf, most)


def test_key_slots_solutions_96_5(native):
    """(96,5), 8 nonces at batch 8: every collision round is a slot round (512 keys, ~1024 rows per
    bucket). The solution sets equal the CPU solver's, no pair is dropped, and rows went through
    the overflow list."""
    n, k = 96, 5
    states = []
    for nonce in range(8):
        st = native.EquihashState(n, k)
        st.update(header_input(nonce, b"main"))
        states.append(st)
    cpu = cpu_sets(native, n, k, states)
    solver = native.EquihashGpuSolver(n, k, 8)
    res = solver.solve(states)
    stats = solver.stats()
    print("pair drops", stats["pair_dropped_all"], "overflow rows", stats["overflow_rows_all"],
          "most in a bucket", stats["overflow_bucket_max"])
    assert sum(stats["pair_dropped_all"]) == 0, stats["pair_dropped_all"]
    assert sum(stats["stage_dropped_all"]) == 0 and stats["cand_dropped"] == 0
    for nonce, (st, sols, c) in enumerate(zip(states, res, cpu)):
        for s in sols:
            assert native.eh_is_valid_solution(n, k, st, s)[0]
        assert set(sols) == c, (nonce, len(sols), len(c))
    assert sum(map(len, cpu)) > 0
    assert sum(stats["overflow_rows_all"][1:k]) > 0
    assert stats["overflow_rows_all"][k] == 0  # the final round sorts


def test_key_slots_tree_dump_200_9(native, main16):
    """Batch 1, debug mode: every written slot of stages 3..8 (the slot rounds' output) names a
    producing bucket < 512 and two different LDS rows < 6016 of it, and more than a quarter of each
    stage's slots are written."""
    import numpy as np
    states, _ = main16
    solver = native.EquihashGpuSolver(N, K, 1)
    solver.set_debug(True)
    for s in solver.solve(states[:1])[0]:
        assert native.eh_is_valid_solution(N, K, states[0], s)[0]
    dump = np.asarray(solver.debug_dump(), dtype=np.uint64).reshape(K, NB * AREA)
    for stage in range(3, K):
        tri = dump[stage][dump[stage] != np.uint64((1 << 64) - 1)]
        assert len(tri) > NB * AREA // 4, stage
        d, i, j = tri >> np.uint64(32), tri & np.uint64(0xFFFF), (tri >> np.uint64(16)) & np.uint64(0xFFFF)
        bad = (d >= NB) | (i >= AREA) | (j >= AREA) | (i == j)
        assert not bad.any(), (stage, [hex(int(x)) for x in tri[bad][:8]])
