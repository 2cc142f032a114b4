"""Whole header checks on the device (csrc/kernels/equihash_header.h): solution, block hash,
nBits decode, target against the pow limit, hash <= target and the link to the header before.

Oracles: hashlib for the block hash, SHA256d(in140 || compactsize || solution); the consensus
code for everything else (`native.eh_check_headers_cpu`: EhIsValidSolution, GetHash,
CheckProofOfWork; `native.compact_to_target_hex` / `check_proof_of_work`: SetCompact), and a
SetCompact written out below.
"""
import functools
import hashlib
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

SOLUTION_VALID, TARGET_LEGAL, HASH_MEETS, HASH_VALID, LINKED = 1, 2, 4, 8, 16
REGTEST_LIMIT = b"\xff" * 31 + b"\x7f"
REGTEST_BITS = 0x207FFFFF
PARAMS = [(48, 5, 36), (96, 5, 68), (200, 9, 1344)]


def compact_size(n: int) -> bytes:
    return bytes([n]) if n < 253 else b"\xfd" + struct.pack("<H", n)


def block_hash(in140: bytes, sol: bytes) -> bytes:
    return hashlib.sha256(hashlib.sha256(in140 + compact_size(len(sol)) + sol).digest()).digest()


def as_int(h: bytes) -> int:
    return int.from_bytes(h, "little")


def set_compact(nbits: int):
    """arith_uint256::SetCompact: (target mod 2^256, negative, overflow)."""
    size, word = nbits >> 24, nbits & 0x007FFFFF
    if size <= 3:
        word >>= 8 * (3 - size)
        target = word
    else:
        target = (word << (8 * (size - 3))) & ((1 << 256) - 1)
    negative = word != 0 and (nbits & 0x00800000) != 0
    overflow = word != 0 and (size > 34 or (word > 0xFF and size > 33) or (word > 0xFFFF and size > 32))
    return target, negative, overflow


def header_input(rng, nbits: int, prev: bytes = None) -> bytes:
    """140 random bytes with hashPrevBlock (4..35) and nBits (104..107) chosen."""
    b = bytearray(rng.getrandbits(8) for _ in range(140))
    if prev is not None:
        b[4:36] = prev
    b[104:108] = struct.pack("<I", nbits)
    return bytes(b)


def state_of(native, n, k, in140):
    st = native.EquihashState(n, k)
    st.update(in140)
    return st


def solve(native, n, k, inputs):
    """One valid solution per input where there is one: CPU solver for the small sets, the GPU
    solver (confirmed by the CPU verifier) for (200,9)."""
    states = [state_of(native, n, k, inp) for inp in inputs]
    if (n, k) == (200, 9):
        found = native.EquihashGpuSolver(n, k, len(inputs)).solve(states)
    else:
        found = [native.eh_solve_cpu(n, k, st)[0] for st in states]
    out = []
    for st, sols in zip(states, found):
        sol = bytes(sols[0]) if sols else None
        if sol is not None:
            assert native.eh_is_valid_solution(n, k, st, sol)[0]
        out.append(sol)
    return out


# ------------------------------------------------------------------ 1. compact decode
MANTISSAS = [0, 1, 0x7F, 0x80, 0xFF, 0x100, 0xFFFF, 0x10000, 0x7FFFFF]
ALL_NBITS = [(size << 24) | sign | m for size in range(256) for m in MANTISSAS for sign in (0, 0x00800000)]


def test_compact_decode_every_size(native):
    got = native.eh_compact_decode_gpu(ALL_NBITS)
    assert len(got) == len(ALL_NBITS) == 256 * 9 * 2
    for nbits, (target, negative, overflow) in zip(ALL_NBITS, got):
        want = set_compact(nbits)
        assert (as_int(target), negative, overflow) == want, hex(nbits)
        hx, neg, ovf = native.compact_to_target_hex(nbits)
        assert (int(hx, 16), neg, ovf) == want, hex(nbits)
    assert native.eh_compact_decode_gpu([]) == []


def test_target_legal_every_size(native):
    """TARGET_LEGAL of eh_header_check over the same nBits values against the regtest limit:
    CheckProofOfWork of an all-zero hash is exactly the legality of the target."""
    rng = random.Random(11)
    extra = [0x2100FFFF, REGTEST_BITS, 0x2000FFFF, 0x1D00FFFF, 0x03000001, 0x02000100, 0x01010000]
    bits = ALL_NBITS + extra
    ins = [header_input(rng, b) for b in bits]
    sol = bytes(36)
    status, _ = native.eh_check_headers_gpu(48, 5, ins, [sol] * len(ins), REGTEST_LIMIT)
    limit = as_int(REGTEST_LIMIT)
    zero = "00" * 32
    for b, s in zip(bits, status):
        target, negative, overflow = set_compact(b)
        legal = not negative and target != 0 and not overflow and target <= limit
        assert bool(s & TARGET_LEGAL) == legal, hex(b)
        assert native.check_proof_of_work(zero, b, True, "regtest") == legal, hex(b)
        assert s & HASH_VALID and not s & SOLUTION_VALID
        if not legal:
            assert not s & HASH_MEETS
    # 0x2100ffff: 0xffff << 240 does not overflow 256 bits and is above the regtest limit
    assert set_compact(0x2100FFFF) == (0xFFFF << 240, False, False)
    assert not status[len(ALL_NBITS)] & TARGET_LEGAL
    # a target equal to the limit is legal, one above it by the last mantissa bit is not
    exact = (0x7FFFFF << 232).to_bytes(32, "little")
    below = (0x7FFFFE << 232).to_bytes(32, "little")
    one = [header_input(rng, REGTEST_BITS)]
    assert native.eh_check_headers_gpu(48, 5, one, [sol], exact)[0][0] & TARGET_LEGAL
    assert not native.eh_check_headers_gpu(48, 5, one, [sol], below)[0][0] & TARGET_LEGAL


# ------------------------------------------------------------------ 2. hash and verdicts
@functools.lru_cache(maxsize=None)
def header_batch(n, k, solw):
    """(inputs, solutions) of 14 headers: solved ones and random-byte ones with nBits on both
    sides of their hash, illegal targets, and one solution of another length. Built once."""
    from bitcoincashplus_amd import native
    rng = random.Random(100 * n + k)
    # candidates at two legal targets (0x7fffff << 232 and 0x1fffff << 232: about 1/2 and 1/8 of
    # the hashes are at or below them); keep solved headers on both sides of their target
    want_solved = 4 if (n, k) != (200, 9) else 2
    cands = [header_input(rng, bits) for bits in [REGTEST_BITS, 0x201FFFFF] * (12 if (n, k) != (200, 9) else 8)]
    solved = [(inp, sol) for inp, sol in zip(cands, solve(native, n, k, cands)) if sol is not None]

    def meets(inp, sol):
        return as_int(block_hash(inp, sol)) <= set_compact(struct.unpack("<I", inp[104:108])[0])[0]

    above = [p for p in solved if not meets(*p)][:want_solved // 2]
    below = [p for p in solved if meets(*p)][:want_solved // 2]
    assert len(above) == len(below) == want_solved // 2, (len(solved), len(above), len(below))
    pairs = above + below
    # random-byte solutions: two above and two at or below their target
    rnd_above, rnd_below = [], []
    while len(rnd_above) < 2 or len(rnd_below) < 2:
        inp = header_input(rng, rng.choice([REGTEST_BITS, 0x203FFFFF]))
        sol = bytes(rng.getrandbits(8) for _ in range(solw))
        (rnd_below if meets(inp, sol) else rnd_above).append((inp, sol))
    pairs += rnd_above[:2] + rnd_below[:2]
    # illegal targets under a valid-length solution: negative, zero, above the limit, overflow
    for bits in (0x20800001 | 0x7F, 0x20000000, 0x2100FFFF, 0x23000001):
        pairs.append((header_input(rng, bits), bytes(rng.getrandbits(8) for _ in range(solw))))
    # a solution one byte short: the device cannot hash it
    pairs.append((header_input(rng, REGTEST_BITS), bytes(rng.getrandbits(8) for _ in range(solw - 1))))
    # and a solved header again at the end, so a valid header follows the bad length
    pairs.append(below[0])
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("n,k,solw", PARAMS)
def test_hash_and_verdicts(native, n, k, solw):
    ins, sols = header_batch(n, k, solw)
    assert 8 <= len(ins) <= 16
    status, hashes = native.eh_check_headers_gpu(n, k, ins, sols, REGTEST_LIMIT)
    want_status, want_hashes = native.eh_check_headers_cpu(n, k, ins, sols, REGTEST_LIMIT)
    print([f"{s:02x}" for s in status])
    for i, (inp, sol) in enumerate(zip(ins, sols)):
        if len(sol) == solw:
            assert hashes[i] == block_hash(inp, sol), i
            assert status[i] & HASH_VALID
        else:
            assert hashes[i] == bytes(32) and not status[i] & (HASH_VALID | HASH_MEETS | SOLUTION_VALID)
    assert list(hashes) == list(want_hashes)
    assert list(status) == list(want_status)
    # the batch holds every verdict both ways
    for bit in (SOLUTION_VALID, TARGET_LEGAL, HASH_MEETS, HASH_VALID):
        assert any(s & bit for s in status) and not all(s & bit for s in status), bit
    assert any(s & SOLUTION_VALID and not s & HASH_MEETS for s in status)  # a valid solution with a high hash
    assert any(s & SOLUTION_VALID and s & HASH_MEETS for s in status)
    assert any(s & TARGET_LEGAL and not s & SOLUTION_VALID and s & HASH_MEETS for s in status)


def test_unsupported_parameters_throw(native):
    rng = random.Random(3)
    with pytest.raises(Exception):
        native.eh_check_headers_gpu(96, 3, [header_input(rng, REGTEST_BITS)], [bytes(26)], REGTEST_LIMIT)
    with pytest.raises(Exception):
        native.eh_check_headers_gpu(48, 5, [bytes(139)], [bytes(36)], REGTEST_LIMIT)


# ------------------------------------------------------------------ 3. links
@functools.lru_cache(maxsize=None)
def chain_of_six():
    rng = random.Random(6)
    ins, sols, prev = [], [], bytes(rng.getrandbits(8) for _ in range(32))
    for _ in range(6):
        inp = header_input(rng, REGTEST_BITS, prev)
        sol = bytes(rng.getrandbits(8) for _ in range(68))
        ins.append(inp)
        sols.append(sol)
        prev = block_hash(inp, sol)
    return ins, sols


def test_links(native):
    n, k = 96, 5
    ins, sols = chain_of_six()

    def linked(a, b):
        status, hashes = native.eh_check_headers_gpu(n, k, a, b, REGTEST_LIMIT)
        want, want_hashes = native.eh_check_headers_cpu(n, k, a, b, REGTEST_LIMIT)
        assert list(status) == list(want) and list(hashes) == list(want_hashes)
        return [bool(s & LINKED) for s in status]

    assert linked(ins, sols) == [True] * 6
    # header 3 names another predecessor: one bit of its hashPrevBlock
    broken = list(ins)
    b = bytearray(broken[3])
    b[35] ^= 0x80
    broken[3] = bytes(b)
    # its own hash changes with it, so header 4 no longer follows either
    assert linked(broken, sols) == [True, True, True, False, False, True]
    # header 2 with a solution of another length: no hash, so neither it nor header 3 is linked
    short = list(sols)
    short[2] = short[2][:-1]
    assert linked(ins, short) == [True, True, False, False, True, True]


# ------------------------------------------------------------------ 4. tensor path
def test_tensor_path_on_a_side_stream(native):
    import torch
    from bitcoincashplus_amd import ops
    n, k, solw = 96, 5, 68
    ins, sols = header_batch(n, k, solw)
    cnt = len(ins)
    want_status, want_hashes = ops.check_headers(n, k, ins, sols, REGTEST_LIMIT)
    assert (list(want_status), list(want_hashes)) == tuple(map(list, native.eh_check_headers_gpu(n, k, ins, sols, REGTEST_LIMIT)))
    dev = torch.device("cuda", 0)
    lenok = torch.tensor([len(s) == solw for s in sols], dtype=torch.uint8, device=dev)
    x = torch.tensor(list(b"".join(ins)), dtype=torch.uint8, device=dev).view(cnt, 140)
    s = torch.tensor(list(b"".join(sl.ljust(solw, b"\0") for sl in sols)), dtype=torch.uint8, device=dev).view(cnt, solw)
    # outputs larger than the batch, filled with a sentinel
    status = torch.full((cnt + 5,), 0xA5, dtype=torch.uint8, device=dev)
    hashes = torch.full((cnt + 5, 32), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        st, hs = ops.check_headers(n, k, x, s, REGTEST_LIMIT, lenok=lenok, out=(status, hashes))
        fresh_st, fresh_hs = ops.check_headers(n, k, x, s, REGTEST_LIMIT, lenok=lenok)
    side.synchronize()
    assert st.is_cuda and hs.is_cuda and fresh_st.is_cuda and fresh_hs.shape == (cnt, 32)
    assert status[:cnt].cpu().tolist() == list(want_status)
    assert [bytes(r) for r in hashes[:cnt].cpu().tolist()] == list(want_hashes)
    assert fresh_st.cpu().tolist() == list(want_status)
    assert [bytes(r) for r in fresh_hs.cpu().tolist()] == list(want_hashes)
    assert status[cnt:].cpu().tolist() == [0xA5] * 5
    assert hashes[cnt:].cpu().flatten().tolist() == [0xA5] * (5 * 32)
    # n = 0: accepted, nothing written
    with torch.cuda.stream(side):
        e_st, e_hs = ops.check_headers(n, k, x[:0], s[:0], REGTEST_LIMIT, out=(status, hashes))
        z_st, z_hs = ops.check_headers(n, k, x[:0], s[:0], REGTEST_LIMIT)
    side.synchronize()
    assert status[:cnt].cpu().tolist() == list(want_status) and status[cnt:].cpu().tolist() == [0xA5] * 5
    assert z_st.numel() == 0 and z_hs.numel() == 0
    assert ops.check_headers(n, k, [], [], REGTEST_LIMIT) == ([], [])
    # the CPU twin behind the same front end
    cpu_status, cpu_hashes = ops.check_headers(n, k, ins, sols, REGTEST_LIMIT, use_gpu=False)
    assert (list(cpu_status), list(cpu_hashes)) == (list(want_status), list(want_hashes))


# ------------------------------------------------------------------ 5. sharding
def test_sharded_over_two_lanes(native):
    n, k = 96, 5
    rng = random.Random(12)
    ins, sols = [list(x) for x in chain_of_six()]
    prev = block_hash(ins[-1], sols[-1])
    for i in range(6):  # headers 6..11 continue the chain: the shard boundary (6) lies inside it
        inp = header_input(rng, REGTEST_BITS, prev)
        sol = bytes(rng.getrandbits(8) for _ in range(68))
        ins.append(inp)
        sols.append(sol)
        prev = block_hash(inp, sol)
    single = native.eh_check_headers_gpu(n, k, ins, sols, REGTEST_LIMIT)
    assert all(s & LINKED for s in single[0])
    try:
        native.gpu_verify_set_devices([0, 0])
        native.gpu_verify_set_min_shard(1, 6)
        native.gpu_verify_set_min_device_shard(1, 6)
        plan = native.gpu_verify_plan(12, True)
        assert [(lo, hi) for _, lo, hi in plan] == [(0, 6), (6, 12)] and plan[0][0] != plan[1][0], plan
        sharded = native.gpu_verify_check_headers(n, k, ins, sols, REGTEST_LIMIT)  # starts the two lanes
        assert (list(sharded[0]), list(sharded[1])) == (list(single[0]), list(single[1]))
        before = native.gpu_verify_stats()
        assert native.gpu_verify_check_headers(n, k, ins, sols, REGTEST_LIMIT) == sharded
        after = native.gpu_verify_stats()
        assert after["sharded_batches"] == before["sharded_batches"] + 1
        assert [b["header_hashes"] - a["header_hashes"] for a, b in zip(before["lanes"], after["lanes"])] == [6, 6]
        # a broken link exactly at the shard boundary, and a bad length just before it
        b = bytearray(ins[6])
        b[4] ^= 1
        cut = ins[:6] + [bytes(b)] + ins[7:]
        for a, s_ in ((cut, sols), (ins, sols[:5] + [sols[5][:-1]] + sols[6:])):
            got = native.gpu_verify_check_headers(n, k, a, s_, REGTEST_LIMIT)
            want = native.eh_check_headers_cpu(n, k, a, s_, REGTEST_LIMIT)
            assert (list(got[0]), list(got[1])) == (list(want[0]), list(want[1]))
            assert not got[0][6] & LINKED
    finally:
        native.gpu_verify_set_min_shard(65536, 2048)
        native.gpu_verify_set_min_device_shard(4096, 256)
        native.gpu_verify_set_devices([])
