"""Device-side block hash and target filter of the Equihash miner (csrc/kernels/equihash_pow.h).

Oracles: hashlib for the block hash, SHA256d(in140 || compactsize || solution) read as a
little-endian 256-bit integer, and the CPU solver / verifier for the solutions.
"""
import functools
import hashlib
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

ALL_FF = b"\xff" * 32
REGTEST_LIMIT = b"\xff" * 31 + b"\x7f"


def header_input(nonce: int, salt: bytes = b"") -> bytes:
    # CEquihashInput (108 B) || nNonce (32 B)
    body = (salt + bytes(108))[:108]
    return body + struct.pack("<I", nonce) + bytes(28)


def compact_size(n: int) -> bytes:
    return bytes([n]) if n < 253 else b"\xfd" + struct.pack("<H", n)


def block_hash(in140: bytes, sol: bytes) -> bytes:
    return hashlib.sha256(hashlib.sha256(in140 + compact_size(len(sol)) + sol).digest()).digest()


def as_int(h: bytes) -> int:
    return int.from_bytes(h, "little")


def le32(v: int) -> bytes:
    return v.to_bytes(32, "little")


def state_of(native, n, k, in140):
    st = native.EquihashState(n, k)
    st.update(in140)
    return st


@functools.lru_cache(maxsize=None)
def cpu_solutions(n, k, salt, count):
    """[(in140, set of CPU solutions)] of the nonces 0..count-1; computed once per module."""
    from bitcoincashplus_amd import native
    out = []
    for nonce in range(count):
        inp = header_input(nonce, salt)
        out.append((inp, frozenset(native.eh_solve_cpu(n, k, state_of(native, n, k, inp))[0])))
    return out


# ------------------------------------------------------------------ 1. hash and compare
@pytest.mark.parametrize("n,k,solw", [(48, 5, 36), (96, 5, 68), (200, 9, 1344)])
def test_pow_check_hash_and_boundaries(native, n, k, solw):
    rng = random.Random(1000 * n + k)
    ins = [bytes(rng.getrandbits(8) for _ in range(140)) for _ in range(8)]
    sols = [bytes(rng.getrandbits(8) for _ in range(solw)) for _ in range(8)]
    want = [block_hash(a, b) for a, b in zip(ins, sols)]
    hashes, passed = native.eh_pow_check_gpu(n, k, ins, sols, ALL_FF)
    assert list(hashes) == want
    assert list(passed) == [True] * 8
    # one pair whose top byte can move both ways
    i = next(j for j, h in enumerate(want) if 0 < h[31] < 255)
    h = as_int(want[i])
    top = want[i][31]
    cases = [
        (le32(h), True),
        (le32(h - 1), False),
        (b"\xff" * 31 + bytes([top - 1]), False),
        (b"\x00" * 31 + bytes([top + 1]), True),
        (bytes(32), False),
    ]
    for target, expect in cases:
        hs, ps = native.eh_pow_check_gpu(n, k, [ins[i]], [sols[i]], target)
        assert hs[0] == want[i]
        assert ps[0] == expect, (target.hex(), want[i].hex())
    # the whole batch against one mid-range target
    mid = sorted(want, key=as_int)[4]
    _, ps = native.eh_pow_check_gpu(n, k, ins, sols, mid)
    assert list(ps) == [as_int(x) <= as_int(mid) for x in want]


def test_pow_check_ops_front_end(native):
    from bitcoincashplus_amd import ops
    inp, sol = header_input(3, b"ops"), bytes(range(68))
    hashes, passed = ops.equihash_pow_check(96, 5, [inp], [sol], ALL_FF)
    assert hashes[0] == block_hash(inp, sol) and passed[0]
    with pytest.raises(Exception):
        native.eh_pow_check_gpu(96, 5, [inp], [sol[:-1]], ALL_FF)


# ------------------------------------------------------------------ 2. the filter is exact
@pytest.mark.parametrize("n,k", [(48, 5), (96, 5)])
def test_pow_filter_exact(native, n, k):
    salt = b"powfilter"
    cpu = cpu_solutions(n, k, salt, 64)
    cpu_hashes = sorted(as_int(block_hash(inp, s)) for inp, sols in cpu for s in sols)
    cpu_total = len(cpu_hashes)
    assert cpu_total >= 2
    tint = cpu_hashes[cpu_total // 2]  # one CPU solution sits exactly on the boundary
    target = le32(tint)
    by_nonce = {inp[108:]: (inp, sols) for inp, sols in cpu}
    solver = native.EquihashGpuSolver(n, k, 16)
    solver.set_debug(True)
    prefix = header_input(0, salt)[:108]
    every, hits, solutions = [], [], 0
    for b0 in range(0, 64, 16):
        solver.launch_pow(prefix, le32(b0), 16, target)
        r = solver.collect_pow()
        assert r["solutions"] == len(r["all"])
        # the stated order: by nonce, then by hash
        keys = [(as_int(nonce), as_int(h)) for nonce, _, h, _ in r["all"]]
        assert keys == sorted(keys)
        assert all(b0 <= kn < b0 + 16 for kn, _ in keys)
        every += r["all"]
        hits += r["hits"]
        solutions += r["solutions"]
    for nonce, sol, h, passed in every:
        inp, sols = by_nonce[nonce]
        assert native.eh_is_valid_solution(n, k, state_of(native, n, k, inp), sol)[0]
        assert h == block_hash(inp, sol)
        assert passed == (as_int(h) <= tint)
        assert sol in sols
    assert len({(nonce, sol) for nonce, sol, _, _ in every}) == len(every)
    assert hits == [(nonce, sol, h) for nonce, sol, h, passed in every if passed]
    print(f"({n},{k}): GPU {solutions} of CPU {cpu_total} solutions, {len(hits)} at or below the median")
    assert solutions == len(every) and solutions >= 0.97 * cpu_total, (solutions, cpu_total)
    assert any(p for *_, p in every) and not all(p for *_, p in every)
    assert solver.stats()["solutions"] == solutions and solver.stats()["nonces"] == 64


# ------------------------------------------------------------------ 3. (200,9) against the unfiltered path
def test_pow_200_9_equals_solve(native):
    prefix = header_input(0, b"main")[:108]
    inputs = [header_input(nonce, b"main") for nonce in range(8)]
    plain = native.EquihashGpuSolver(200, 9, 8)
    res = plain.solve([state_of(native, 200, 9, inp) for inp in inputs])
    want = {(inp[108:], s) for inp, sols in zip(inputs, res) for s in sols}
    assert want
    solver = native.EquihashGpuSolver(200, 9, 8)
    solver.launch_pow(prefix, le32(0), 8, ALL_FF)
    r = solver.collect_pow()
    assert r["all"] == []  # not in debug mode
    assert {(nonce, sol) for nonce, sol, _ in r["hits"]} == want
    assert len(r["hits"]) == len(want) == r["solutions"]
    for nonce, sol, h in r["hits"]:
        assert len(sol) == 1344
        assert h == block_hash(prefix + nonce, sol)
    assert solver.stats()["solutions"] == plain.stats()["solutions"]
    assert solver.stats()["candidates"] == plain.stats()["candidates"]
    # the median hash as the target: exactly the solutions at or below it
    hashes = sorted(as_int(h) for _, _, h in r["hits"])
    tint = hashes[len(hashes) // 2]
    solver.launch_pow(prefix, le32(0), 8, le32(tint))
    r2 = solver.collect_pow()
    assert r2["hits"] == [x for x in r["hits"] if as_int(x[2]) <= tint]
    assert 0 < len(r2["hits"]) and r2["solutions"] == len(want)
    if len(hashes) > 1:
        assert len(r2["hits"]) < len(r["hits"])


# ------------------------------------------------------------------ 4. nonce arithmetic
@pytest.mark.parametrize("first", [2**64 - 3, 2**192 - 2, 2**256 - 2])
def test_pow_nonce_arithmetic(native, first):
    prefix = header_input(0, b"carry")[:108]
    expected = {le32((first + i) % 2**256) for i in range(8)}
    solver = native.EquihashGpuSolver(48, 5, 8)
    solver.set_debug(True)
    solver.launch_pow(prefix, le32(first), 8, ALL_FF)
    r = solver.collect_pow()
    assert len(r["all"]) >= 1
    for nonce, sol, h, passed in r["all"]:
        assert nonce in expected
        # fails if the device hashed another nonce than the one it reports
        assert native.eh_is_valid_solution(48, 5, state_of(native, 48, 5, prefix + nonce), sol)[0]
        assert h == block_hash(prefix + nonce, sol) and passed
    # in range order, also across the wrap
    order = [(as_int(nonce) - first) % 2**256 for nonce, *_ in r["all"]]
    assert order == sorted(order)


# ------------------------------------------------------------------ 5. pipelined and partial batches
def test_pow_mine_pipelined_partial(native):
    from bitcoincashplus_amd import ops
    n, k = 96, 5
    prefix = header_input(0, b"pipeline")[:108]
    first = 1000
    got = ops.equihash_mine(n, k, prefix, first, 40, REGTEST_LIMIT, batch=16, device=0)
    solver = native.EquihashGpuSolver(n, k, 16)
    want = []
    for off, cnt in [(0, 16), (16, 16), (32, 8)]:
        solver.launch_pow(prefix, le32(first + off), cnt, REGTEST_LIMIT)
        want += solver.collect_pow()["hits"]
    assert got == want and len(got) >= 1
    for nonce, sol, h in got:
        assert first <= as_int(nonce) < first + 40
        assert as_int(h) <= as_int(REGTEST_LIMIT) and h == block_hash(prefix + nonce, sol)
    # the two launch/collect pairs do not mix
    solver.launch_pow(prefix, le32(first), 16, REGTEST_LIMIT)
    with pytest.raises(RuntimeError):
        solver.collect()
    assert solver.collect_pow()["hits"] == [x for x in want if as_int(x[0]) < first + 16]
    solver.launch([state_of(native, n, k, prefix + le32(first))])
    with pytest.raises(RuntimeError):
        solver.collect_pow()
    solver.collect()
    with pytest.raises(Exception):
        solver.launch_pow(prefix, le32(first), 17, REGTEST_LIMIT)  # count > batch


# ------------------------------------------------------------------ 6. the built-in miner's target overload
@pytest.mark.parametrize("n,k", [(96, 5), (200, 9)])
def test_gpu_miner_search_target(native, n, k):
    body = bytes((i * 7 + 3) & 0xFF for i in range(108))
    nonce0 = le32(5)
    r = native.eh_search_gpu_target(n, k, body, nonce0, 256, REGTEST_LIMIT)
    assert r["found"]
    nonce = as_int(r["nonce"])
    assert 6 <= nonce <= 5 + 256
    assert r["nonces"] >= 1 and r["solutions"] >= 1 and r["hits"] >= 1
    assert native.eh_is_valid_solution(n, k, state_of(native, n, k, body + r["nonce"]), r["solution"])[0]
    assert r["hash"] == block_hash(body + r["nonce"], r["solution"])
    assert as_int(r["hash"]) <= as_int(REGTEST_LIMIT)
    r0 = native.eh_search_gpu_target(n, k, body, nonce0, 0, REGTEST_LIMIT, [0])
    assert not r0["found"] and r0["nonces"] == 0
