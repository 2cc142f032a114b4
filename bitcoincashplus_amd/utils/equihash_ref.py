"""Pure-Python Equihash oracle (hashlib BLAKE2b) used to cross-check the C++/HIP code.

It follows the reference's byte-level formulation (src/crypto/equihash.cpp):
ExpandArray to CollisionByteLength-wide big-endian digits, collision on the
next CollisionByteLength bytes, lexicographic index-list ordering,
distinct indices and an all-zero final hash.  Deliberately slow and simple.
"""
from __future__ import annotations

import hashlib
import struct
from typing import List


def personal(n: int, k: int) -> bytes:
    return b"ZcashPoW" + struct.pack("<II", n, k)


def hash_output_len(n: int) -> int:
    return (512 // n) * n // 8


def base_hasher(n: int, k: int, data: bytes):
    h = hashlib.blake2b(digest_size=hash_output_len(n), person=personal(n, k))
    h.update(data)
    return h


def generate_hash(base, g: int) -> bytes:
    h = base.copy()
    h.update(struct.pack("<I", g))
    return h.digest()


def expand_array(inp: bytes, bit_len: int, byte_pad: int = 0) -> bytes:
    out_width = (bit_len + 7) // 8 + byte_pad
    bits = int.from_bytes(inp, "big")
    total = len(inp) * 8
    groups = total // bit_len
    out = bytearray()
    for g in range(groups):
        v = (bits >> (total - (g + 1) * bit_len)) & ((1 << bit_len) - 1)
        out += bytes(byte_pad) + v.to_bytes(out_width - byte_pad, "big")
    return bytes(out)


def indices_from_minimal(minimal: bytes, cbl: int) -> List[int]:
    nb = cbl + 1
    v = int.from_bytes(minimal, "big")
    total = len(minimal) * 8
    cnt = total // nb
    return [(v >> (total - (i + 1) * nb)) & ((1 << nb) - 1) for i in range(cnt)]


def minimal_from_indices(indices: List[int], cbl: int) -> bytes:
    nb = cbl + 1
    v = 0
    for i in indices:
        v = (v << nb) | i
    return v.to_bytes(len(indices) * nb // 8, "big")


def is_valid_solution(n: int, k: int, data: bytes, soln: bytes) -> bool:
    cbl = n // (k + 1)
    cbytes = (cbl + 7) // 8
    iph = 512 // n
    if len(soln) != (1 << k) * (cbl + 1) // 8:
        return False
    base = base_hasher(n, k, data)
    rows = []
    for i in indices_from_minimal(soln, cbl):
        h = generate_hash(base, i // iph)
        sl = h[(i % iph) * n // 8:(i % iph + 1) * n // 8]
        rows.append((expand_array(sl, cbl), [i]))
    while len(rows) > 1:
        nxt = []
        for a, b in zip(rows[0::2], rows[1::2]):
            ha, ia = a
            hb, ib = b
            if ha[:cbytes] != hb[:cbytes]:
                return False
            if ib < ia:  # lexicographic list comparison == reference IndicesBefore
                return False
            if set(ia) & set(ib):
                return False
            nxt.append((bytes(x ^ y for x, y in zip(ha, hb))[cbytes:], ia + ib))
        rows = nxt
    return all(c == 0 for c in rows[0][0])


COLLISION, ORDER, DUP, FINAL, LENGTH = 1, 2, 4, 8, 16

_LEAVES = {}  # (n, k, data) -> {index: the leaf's n-bit hash slice as an integer}


def leaf_value(n: int, k: int, data: bytes, index: int) -> int:
    """The n-bit string of leaf `index` (digit 0 in the top bits), cached per (header, index)."""
    entry = _LEAVES.get((n, k, data))
    if entry is None:
        if len(_LEAVES) >= 64:  # a test module's headers; the map does not grow without bound
            _LEAVES.clear()
        entry = _LEAVES[(n, k, data)] = (base_hasher(n, k, data), {})
    base, leaves = entry
    v = leaves.get(index)
    if v is None:
        iph = 512 // n
        h = generate_hash(base, index // iph)
        for s in range(iph):
            leaves[index - index % iph + s] = int.from_bytes(h[s * n // 8:(s + 1) * n // 8], "big")
        v = leaves[index]
    return v


def check_mask(n: int, k: int, data: bytes, soln: bytes) -> int:
    """Which properties of a valid solution `soln` lacks, all of them evaluated (no early exit);
    0 iff is_valid_solution. With X(node) the XOR of the leaf strings under a node and digit d
    the d-th group of n/(k+1) bits:
      COLLISION  some node at level l (children of 2^l leaves): digit l of X(left) != digit l of X(right)
      ORDER      some node: first index of its left child >= first index of its right child
      DUP        two positions hold the same index
      FINAL      digit k of X(root) != 0
      LENGTH     wrong byte length; nothing else is evaluated
    """
    cbl = n // (k + 1)
    if len(soln) != (1 << k) * (cbl + 1) // 8:
        return LENGTH
    idx = indices_from_minimal(soln, cbl)
    mask = DUP if len(set(idx)) != len(idx) else 0
    xs = [leaf_value(n, k, data, i) for i in idx]
    firsts = idx
    digit = (1 << cbl) - 1
    for level in range(k):
        shift = n - (level + 1) * cbl
        for a in range(0, len(xs), 2):
            if ((xs[a] ^ xs[a + 1]) >> shift) & digit:
                mask |= COLLISION
            if firsts[a] >= firsts[a + 1]:
                mask |= ORDER
        xs = [xs[a] ^ xs[a + 1] for a in range(0, len(xs), 2)]
        firsts = firsts[0::2]
    if (xs[0] >> (n - (k + 1) * cbl)) & digit:
        mask |= FINAL
    return mask


def solve(n: int, k: int, data: bytes) -> List[bytes]:
    """Full-index-list Wagner solver (reference BasicSolve semantics). Small params only."""
    cbl = n // (k + 1)
    cbytes = (cbl + 7) // 8
    iph = 512 // n
    base = base_hasher(n, k, data)
    init = 1 << (cbl + 1)
    X = []
    g = 0
    while len(X) < init:
        h = generate_hash(base, g)
        for s in range(iph):
            if len(X) >= init:
                break
            X.append((expand_array(h[s * n // 8:(s + 1) * n // 8], cbl), (g * iph + s,)))
        g += 1
    for _ in range(1, k):
        X.sort(key=lambda r: r[0][:cbytes])
        nxt = []
        i = 0
        while i < len(X):
            j = i + 1
            while j < len(X) and X[j][0][:cbytes] == X[i][0][:cbytes]:
                j += 1
            for a in range(i, j):
                for b in range(a + 1, j):
                    ha, ia = X[a]
                    hb, ib = X[b]
                    if set(ia) & set(ib):
                        continue
                    x = bytes(p ^ q for p, q in zip(ha, hb))[cbytes:]
                    nxt.append((x, ia + ib if ia < ib else ib + ia))
            i = j
        X = nxt
    X.sort(key=lambda r: r[0])
    sols = set()
    i = 0
    while i < len(X):
        j = i + 1
        while j < len(X) and X[j][0] == X[i][0]:
            j += 1
        for a in range(i, j):
            for b in range(a + 1, j):
                ia, ib = X[a][1], X[b][1]
                if set(ia) & set(ib):
                    continue
                idx = ia + ib if ia < ib else ib + ia
                sols.add(minimal_from_indices(list(idx), cbl))
        i = j
    return sorted(sols)
