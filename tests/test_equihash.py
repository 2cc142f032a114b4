"""Equihash: CPU reference vs the pure-Python oracle, bit packing, and the gfx950 kernels.

The reference ships no Equihash unit tests; parity is pinned against
an independent hashlib-based oracle implementing the reference's byte-level
rules (bitcoincashplus_amd/utils/equihash_ref.py).
"""
import os
import struct

import pytest

from bitcoincashplus_amd.utils import equihash_ref as R


def header_input(nonce: int, salt: bytes = b"") -> bytes:
    # CEquihashInput (108 B) || nNonce (32 B)
    body = (salt + bytes(108))[:108]
    return body + struct.pack("<I", nonce) + bytes(28)


def test_params(native):
    assert native.eh_solution_width(200, 9) == 1344
    assert native.eh_solution_width(48, 5) == 36
    assert native.eh_solution_width(96, 5) == 68
    assert native.eh_solution_width(96, 3) == 25


@pytest.mark.parametrize("bit_len,pad", [(20, 0), (21, 1), (8, 0), (9, 3), (25, 0)])
def test_expand_compress_roundtrip(native, bit_len, pad):
    width = (bit_len + 7) // 8 + pad
    nbytes = bit_len * 8  # multiple of bit_len bits
    raw = os.urandom(nbytes)
    exp = native.eh_expand_array(raw, bit_len, pad)
    assert exp == R.expand_array(raw, bit_len, pad)
    assert len(exp) == (8 * nbytes // bit_len) * width
    assert native.eh_compress_array(exp, bit_len, pad) == raw


def test_minimal_roundtrip(native):
    import random
    rnd = random.Random(1)
    idx = [rnd.randrange(1 << 21) for _ in range(512)]
    m = native.eh_minimal_from_indices(idx, 20)
    assert len(m) == 1344
    assert m == R.minimal_from_indices(idx, 20)
    assert native.eh_indices_from_minimal(m, 20) == idx


def test_base_state_matches_hashlib(native):
    data = header_input(7, b"abc")
    st = native.EquihashState(200, 9)
    st.update(data)
    base = R.base_hasher(200, 9, data)
    for g in (0, 1, 12345, (1 << 20) - 1):
        assert st.hash(g) == R.generate_hash(base, g)


@pytest.mark.parametrize("nonce", range(12))
def test_cpu_solver_matches_oracle_48_5(native, nonce):
    data = header_input(nonce)
    st = native.EquihashState(48, 5)
    st.update(data)
    sols, stats = native.eh_solve_cpu(48, 5, st)
    assert sorted(sols) == R.solve(48, 5, data)
    for s in sols:
        assert R.is_valid_solution(48, 5, data, s)
        assert native.eh_is_valid_solution(48, 5, st, s)[0]


def _find_solved(native, n, k, tries=40):
    for nonce in range(tries):
        data = header_input(nonce, b"find")
        st = native.EquihashState(n, k)
        st.update(data)
        sols, _ = native.eh_solve_cpu(n, k, st)
        if sols:
            return data, st, sols
    raise AssertionError("no solution found")


def test_verifier_rejections_96_5(native):
    data, st, sols = _find_solved(native, 96, 5)
    s = sols[0]
    assert R.is_valid_solution(96, 5, data, s)
    assert native.eh_is_valid_solution(96, 5, st, s) == (True, "")
    # wrong length
    assert native.eh_is_valid_solution(96, 5, st, s + b"\0")[1] == "invalid-solution-length"
    idx = native.eh_indices_from_minimal(s, 16)
    # swap the two halves of the first pair -> ordering violation
    bad = list(idx)
    bad[0], bad[1] = bad[1], bad[0]
    ok, why = native.eh_is_valid_solution(96, 5, st, native.eh_minimal_from_indices(bad, 16))
    assert not ok and why == "index-tree-incorrectly-ordered"
    assert not R.is_valid_solution(96, 5, data, native.eh_minimal_from_indices(bad, 16))
    # duplicate a whole subtree -> collision passes, distinctness fails
    dup = idx[:2] + idx[:2] + idx[4:]
    ok, why = native.eh_is_valid_solution(96, 5, st, native.eh_minimal_from_indices(dup, 16))
    assert not ok
    # corrupt one index -> collision failure
    cor = list(idx)
    cor[5] ^= 1
    assert not native.eh_is_valid_solution(96, 5, st, native.eh_minimal_from_indices(cor, 16))[0]
    # different header -> invalid
    st2 = native.EquihashState(96, 5)
    st2.update(header_input(999999, b"other"))
    assert not native.eh_is_valid_solution(96, 5, st2, s)[0]


@pytest.mark.slow
def test_cpu_solver_200_9(native):
    data = header_input(1, b"mainnet")
    st = native.EquihashState(200, 9)
    st.update(data)
    sols, stats = native.eh_solve_cpu(200, 9, st)
    for s in sols:
        assert len(s) == 1344
        assert R.is_valid_solution(200, 9, data, s)


# ------------------------------------------------------------------ GPU (gfx950)

@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(48, 5), (96, 5)])
def test_gpu_solver_matches_cpu(native, n, k):
    solver = native.EquihashGpuSolver(n, k, 4)
    states, cpu = [], []
    for nonce in range(8):
        st = native.EquihashState(n, k)
        st.update(header_input(nonce, b"gpu"))
        states.append(st)
        cpu.append(set(native.eh_solve_cpu(n, k, st)[0]))
    got = solver.solve(states[:4]) + solver.solve(states[4:])
    found = 0
    for st, c, g in zip(states, cpu, got):
        for s in g:
            assert native.eh_is_valid_solution(n, k, st, s)[0]
        found += len(g)
        # the GPU may drop rows on bucket overflow but must not invent solutions
        assert set(g) <= c or not c
    assert found >= 0.97 * sum(len(c) for c in cpu)


@pytest.mark.gpu
def test_gpu_solver_tree_dump_96_5(native):
    """SetDebug + DebugDump decode the slot arrays (rows with compact or two-word parent triples):
    every written stage-s (s >= 1) slot names a producing bucket < NB and two LDS rows < AREA of
    it, every written stage-0 slot a leaf index < 2^(DB+1); never-written slots read all-ones."""
    n, k, nb, area = 96, 5, 128, 1280
    solver = native.EquihashGpuSolver(n, k, 1)
    solver.set_debug(True)
    st = native.EquihashState(n, k)
    st.update(header_input(3, b"dump"))
    sols = solver.solve([st])[0]
    for s_ in sols:
        assert native.eh_is_valid_solution(n, k, st, s_)[0]
    dump = solver.debug_dump()
    rows = len(dump) // k
    assert rows == nb * area
    leaves = [x for x in dump[:rows] if x != 0xFFFFFFFF]
    assert len(leaves) > rows // 2 and max(leaves) < 1 << (n // (k + 1) + 1)
    for stage in range(1, k):
        tri = [x for x in dump[stage * rows:(stage + 1) * rows] if x != (1 << 64) - 1]
        assert len(tri) > rows // 4, stage
        for x in tri:
            d, i, j = x >> 32, x & 0xFFFF, (x >> 16) & 0xFFFF
            assert d < nb and i < area and j < area and i != j, (stage, hex(x))


@pytest.mark.gpu
def test_gpu_solver_200_9(native):
    """Recall pinned against the CPU reference solver over 16 mainnet-parameter nonces: the GPU
    never reports a solution the CPU does not find, and finds at least 97% of the CPU's
    (measured: 54 of 54 over 32 nonces, gpurun_out r3a/recall.json)."""
    import concurrent.futures as cf
    states = []
    for nonce in range(16):
        st = native.EquihashState(200, 9)
        st.update(header_input(nonce, b"main"))
        states.append(st)
    with cf.ThreadPoolExecutor(8) as ex:  # the binding releases the GIL
        cpu = list(ex.map(lambda st: set(native.eh_solve_cpu(200, 9, st)[0]), states))
    solver = native.EquihashGpuSolver(200, 9, 8)
    res = solver.solve(states[:8]) + solver.solve(states[8:])
    total = 0
    for st, sols, c in zip(states, res, cpu):
        for s in sols:
            assert len(s) == 1344
            assert native.eh_is_valid_solution(200, 9, st, s)[0]
            assert s in c
        total += len(sols)
    cpu_total = sum(map(len, cpu))
    assert cpu_total >= 16  # ~1.7-1.9 per nonce
    assert total >= 0.97 * cpu_total, (total, cpu_total)


@pytest.mark.gpu
def test_gpu_solver_200_9_no_overflow(native):
    """No row of any nonce is dropped at a bucket's capacity and no final candidate past the list,
    on the 32 nonces of tools/eh_recall.py. The bucket fills do not depend on the order of the
    atomics, so this is deterministic. With the final round at 5120 rows, about 12 stage-8 buckets
    of these nonces overflowed by 2-140 rows, and the dropped rows, chosen by the atomics, cost a
    solution in 3 of 17 solves (profiles/equihash_r5.md, final-round capacity)."""
    states = []
    for nonce in range(32):
        st = native.EquihashState(200, 9)
        st.update(header_input(nonce, b"main"))
        states.append(st)
    solver = native.EquihashGpuSolver(200, 9, 8)
    solver.set_debug(True)
    found = 0
    for b0 in range(0, 32, 8):
        found += sum(map(len, solver.solve(states[b0:b0 + 8])))
    st = solver.stats()
    assert sum(st["stage_dropped_all"]) == 0, (st["stage_dropped_all"], st["overflow_fills"][:16])
    assert st["cand_dropped"] == 0 and st["cand_max"] < 256
    assert found >= 50  # 54 from the CPU solver


@pytest.mark.gpu
def test_gpu_solver_200_9_every_claimed_slot_written(native):
    """In every bucket area of every stage the written slots are one prefix: a round emits a row
    into each slot it claims. The inputs are the benchmark's step 5 at 8 nonces per batch, where
    a pair filter that counted a kept pair with equal first words but never placed it left three
    claimed slots of nonce 0 unwritten (bucket 0 of stages 4, 6 and 8); such a slot keeps an
    earlier batch's row, and 3 of 108,017 solutions were invalid that way."""
    import numpy as np
    k, nb, area = 9, 512, 6016
    header = bytes((i * 37 + 11) & 0xFF for i in range(108))
    states = []
    for b in range(8):
        st = native.EquihashState(200, 9)
        st.update(header + struct.pack("<QQQQ", 5 * 8 + b, 0, 0, 0))
        states.append(st)
    solver = native.EquihashGpuSolver(200, 9, 8)
    solver.set_debug(True)
    solver.solve(states)
    dump = np.asarray(solver.debug_dump(), dtype=np.uint64).reshape(k, nb, area)
    pos = np.arange(area)[None, :]
    for stage in range(k):
        written = dump[stage] != np.uint64(0xFFFFFFFF if stage == 0 else (1 << 64) - 1)
        assert written.sum() > nb * area // 2, stage
        last = (written * pos).max(axis=1)
        holes = np.argwhere(~written & (pos < last[:, None]))
        assert len(holes) == 0, (stage, holes[:8].tolist())


@pytest.mark.gpu
def test_gpu_solver_recall_small(native):
    """(48,5) / (96,5): GPU recall >= 0.97 of the CPU solver over 64 nonces."""
    for n, k in [(48, 5), (96, 5)]:
        solver = native.EquihashGpuSolver(n, k, 16)
        cpu_total = gpu_total = 0
        for b0 in range(0, 64, 16):
            states = []
            for nonce in range(b0, b0 + 16):
                st = native.EquihashState(n, k)
                st.update(header_input(nonce, b"recall"))
                states.append(st)
            for st, g in zip(states, solver.solve(states)):
                c = set(native.eh_solve_cpu(n, k, st)[0])
                assert set(g) <= c
                cpu_total += len(c)
                gpu_total += len(g)
        assert cpu_total > 0 and gpu_total >= 0.97 * cpu_total, (n, k, gpu_total, cpu_total)


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(48, 5), (96, 5), (200, 9)])
def test_gpu_verify_batch(native, n, k):
    states, sols, expect = [], [], []
    solver = native.EquihashGpuSolver(n, k, 1)
    nonce = 0
    while len(sols) < 6 and nonce < 64:
        st = native.EquihashState(n, k)
        st.update(header_input(nonce, b"verify"))
        nonce += 1
        for s in solver.solve([st])[0]:
            states.append(st)
            sols.append(s)
            expect.append(True)
    assert sols, "solver produced nothing"
    cbl = n // (k + 1)
    # negative cases
    s0, st0 = sols[0], states[0]
    idx = native.eh_indices_from_minimal(s0, cbl)
    swapped = list(idx)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    corrupt = list(idx)
    corrupt[3] ^= 1
    for bad in (swapped, corrupt, idx[:2] + idx[:2] + idx[4:]):
        states.append(st0)
        sols.append(native.eh_minimal_from_indices(bad, cbl))
        expect.append(False)
    states.append(st0)
    sols.append(s0[:-1])
    expect.append(False)
    got = native.eh_verify_batch_gpu(n, k, states, sols)
    assert list(got) == expect
    cpu = [native.eh_is_valid_solution(n, k, st, s)[0] for st, s in zip(states, sols)]
    assert cpu == expect


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(96, 5), (200, 9)])
def test_gpu_miner_search(native, n, k):
    """The built-in miner's multi-GPU search (EquihashSearchGpu): every visible device, two
    double-buffered solvers each; the accepted solution is valid for its nonce, which lies in
    the searched range."""
    body = bytes((i * 7 + 3) & 0xFF for i in range(108))
    nonce0 = (5).to_bytes(32, "little")
    r = native.eh_search_gpu(n, k, body, nonce0, 256)
    assert r["found"]
    nonce = int.from_bytes(r["nonce"], "little")
    assert 6 <= nonce <= 5 + 256
    assert r["nonces"] >= 1 and r["solutions"] >= 1
    st = native.EquihashState(n, k)
    st.update(body + r["nonce"])
    assert native.eh_is_valid_solution(n, k, st, r["solution"])[0]
    # explicit device list, and an exhausted range reports not found
    r0 = native.eh_search_gpu(n, k, body, nonce0, 0, [0])
    assert not r0["found"] and r0["nonces"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(96, 5), (200, 9)])
def test_gpu_expand_rejects_out_of_range_parent(native, n, k):
    # The tree expansion must reject a candidate whose parent triple points outside the stage
    # arrays (a bucket >= NB or an LDS row >= AREA) instead of reading through it: the fault of
    # round 4's timing build (gpurun_out/kt5) came from an unchecked parent. Plant both kinds
    # in the first candidate's left stage-(K-1) parent and re-run only the expansion.
    solver = native.EquihashGpuSolver(n, k, 1)
    for nonce in range(64):
        st = native.EquihashState(n, k)
        st.update(header_input(nonce, b"expand-probe"))
        first = solver.solve([st])
        base = solver.debug_expand_corrupt(0)
        if len(base) >= 2:
            break
    assert len(base) >= 2, "no nonce with two final-round candidates"
    for mode in (1, 2):
        solver.solve([st])  # fresh, uncorrupted stage arrays (candidate order varies per solve)
        base = solver.debug_expand_corrupt(0)
        got = solver.debug_expand_corrupt(mode)
        assert got[0] == 0, (mode, got[:4])  # the corrupted candidate is rejected
        # no other candidate turns valid (one sharing the corrupted slot may turn invalid too)
        assert all(g <= b for g, b in zip(got[1:], base[1:]))
    # and the device is fine afterwards: the same nonce solves to the same solutions
    # (the solver does not order a nonce's solutions: compare them as sets)
    assert [sorted(x) for x in solver.solve([st])] == [sorted(x) for x in first]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(96, 5), (200, 9)])
def test_stamped_rounds_match_plain(native, n, k):
    # The phase-stamped diagnostic round kernels (set_stamp_mode, read by tools/eh_diag.py and
    # tools/eh_phases.py) solve like the plain ones, and phase_cycles reports one entry per round:
    # [0] the whole bucket, [1..6] its phases, [7..8] the two halves of phase 4.
    st = native.EquihashState(n, k)
    st.update(header_input(0, b"main"))
    solver = native.EquihashGpuSolver(n, k, 1)
    plain = solver.solve([st])
    solver.set_stamp_mode(True)
    stamped = solver.solve([st])
    assert [sorted(x) for x in stamped] == [sorted(x) for x in plain]
    cycles = solver.phase_cycles(1)
    assert len(cycles) == k
    for stage, ph in enumerate(cycles):
        print(stage + 1, [round(x) for x in ph])
        assert len(ph) == 9
        assert ph[0] > 0
        # the phases lie inside the bucket (a phase the round does not have counts as 0); the means
        # are sums of at most 2^9 integers below 2^40 in doubles: 1e-9 covers their rounding
        assert ph[0] >= sum(ph[1:7]) * (1 - 1e-9), (stage + 1, ph)
