#!/usr/bin/env python3
"""Near-collisions of a whole Wagner run, for the constructed Equihash vectors
(tests/equihash_vectors.py, family N): for each level l >= 2 (l >= 1 at (96,3)) and each bit of digit l, two subtrees
of 2^l leaves that collide on every level below and whose XORs differ in that bit of digit l alone;
and for each bit of the last digit a full tree that collides on every level and whose last digit is
that bit alone. A verifier that compares a digit over too few bits accepts what these lists fail.

The run is a plain numpy Wagner over all 2^(DB+1) leaves (rows of K+1 digits, sorted by the digit
of the round, all pairs up to eight places apart in a run of equal digits, parents kept per round).
It takes too long for a test, so the tests do not run it: the lists
are written to tests/data/equihash_near_N_K.json as index lists, and the tests take every expected
mask from the Python oracle, never from this file.

    python tools/eh_near_collisions.py 200 9
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import equihash_vectors as V  # noqa: E402
from bitcoincashplus_amd.utils import equihash_ref as R  # noqa: E402

CAP = 40 << 20  # rows kept per round (the whole (96,3) table)


def leaf_digits(p, data):
    """[2^(DB+1), K+1] uint32: every leaf's digits."""
    base = R.base_hasher(p.n, p.k, data)
    count = 1 << p.index_bits
    nbytes = p.n // 8
    out = np.zeros((count, p.k + 1), dtype=np.uint32)
    hashes = (count + p.iph - 1) // p.iph
    for c0 in range(0, hashes, 1 << 16):
        c1 = min(hashes, c0 + (1 << 16))
        raw = np.frombuffer(b"".join(R.generate_hash(base, g) for g in range(c0, c1)), dtype=np.uint8)
        rows = np.zeros(((c1 - c0) * p.iph, nbytes + 4), dtype=np.uint32)
        rows[:, :nbytes] = raw.reshape(-1, nbytes)
        lo, hi = c0 * p.iph, min(count, c1 * p.iph)
        for d in range(p.k + 1):
            byte, off = (d * p.db) // 8, (d * p.db) % 8
            word = (rows[:, byte] << 24) | (rows[:, byte + 1] << 16) | (rows[:, byte + 2] << 8) | rows[:, byte + 3]
            out[lo:hi, d] = ((word << off) >> (32 - p.db))[:hi - lo]
    return out


def one_bit_apart(col, order, diff):
    """Yields (a, b): two rows whose values in `col` differ by exactly `diff`. `order` sorts col;
    the first of the two is looked for among 2^18 rows spread over the table."""
    sc = col[order]
    probe = order[::max(1, len(order) >> 18)]
    target = col[probe] ^ np.uint32(diff)
    pos = np.minimum(np.searchsorted(sc, target), len(sc) - 1)
    for h in np.flatnonzero(sc[pos] == target):
        a, b = int(probe[h]), int(order[pos[h]])
        if a != b:
            yield a, b


def distinct_first(candidates, tries=32):
    """The first of the candidate index lists without a repeated index (rows of the later rounds
    often share a subtree), else the first."""
    kept = None
    for _, idx in zip(range(tries), candidates):
        if kept is None:
            kept = idx
        if len(set(idx)) == len(idx):
            return idx
    return kept


def main():
    n, k = int(sys.argv[1]), int(sys.argv[2])
    p = V.Params(n, k)
    data = V.header_input(0)
    t0 = time.time()
    X = leaf_digits(p, data)
    first = np.arange(len(X), dtype=np.int64)
    parents = []  # per round: (left rows, right rows) of the round before
    print(f"{len(X)} leaves in {time.time() - t0:.0f} s", flush=True)

    def leaves(level, row):
        if level == 0:
            return [int(row)]
        left, right = parents[level - 1]
        return leaves(level - 1, left[row]) + leaves(level - 1, right[row])

    # the tests scan a small index space themselves and build levels 0 and 1 from it
    first_level = 2 if p.index_bits <= 22 else 1
    entries = []
    for level in range(p.k + 1):
        # rows are subtrees of 2^level leaves whose digits below `level` are zero
        col = np.ascontiguousarray(X[:, level])
        order = np.argsort(col, kind="stable")
        if level >= first_level:
            for bit in range(p.db):
                if level < p.k:
                    idx = distinct_first(leaves(level, a) + leaves(level, b)
                                         for a, b in (sorted(hit, key=lambda r: first[r])
                                                      for hit in one_bit_apart(col, order, 1 << bit)))
                else:
                    idx = distinct_first(leaves(level, row) for row in np.flatnonzero(col == (1 << bit)))
                if idx is not None:
                    entries.append({"level": level if level < p.k else "final", "bit": bit, "indices": idx})
        if level == p.k:
            break
        sk = col[order]
        lefts, rights = [], []
        for d in range(1, 9):
            eq = np.flatnonzero(sk[:-d] == sk[d:])
            lefts.append(order[eq])
            rights.append(order[eq + d])
        left, right = np.concatenate(lefts)[:CAP], np.concatenate(rights)[:CAP]
        swap = first[left] > first[right]  # the smaller first index in front
        left, right = np.where(swap, right, left), np.where(swap, left, right)
        parents.append((left, right))
        X = X[left] ^ X[right]
        first = first[left]
        assert not X[:, :level + 1].any()
        print(f"round {level}: {len(X)} rows, {time.time() - t0:.0f} s", flush=True)
    for e in entries:
        assert len(e["indices"]) == (p.leaves if e["level"] == "final" else 2 << e["level"])
    out = os.path.join(ROOT, "tests", "data", f"equihash_near_{n}_{k}.json")
    with open(out, "w") as f:
        json.dump({"n": n, "k": k, "input": data.hex(), "lists": entries}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(entries)} lists -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
