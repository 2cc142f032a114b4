"""Constructed near-valid Equihash solutions for the verifiers (csrc/consensus/equihash.cpp on the
CPU, eh_verify of csrc/kernels/equihash_verify.hip on the MI355X), judged by the pure-Python oracle.

A plain helper module (imported by tests/test_equihash_vectors.py, like tests/ecdsa_vectors.py).
`build(native, n, k)` makes the vectors of one parameter set. Each vector is (label, 140-byte
header input, solution bytes, expected mask); the mask is R.check_mask's, and where a construction
promises a mask (the isolating families) `_Builder.add` asserts the promise against the oracle, so a
construction that does not do what its label says fails on the CPU before any kernel runs. The code
under test supplies valid solutions (the solvers; each one is confirmed by R.is_valid_solution
before use), never a verdict or a mask.

Families (docs/EQUIHASH_VECTORS.md): V valid; S subtree swap (ORDER at one level); X cross-pairing
(COLLISION at one level); F / T near-solutions of a Wagner run (FINAL alone / top-level COLLISION
alone, and pairs one bit away from colliding); U duplicates alone; D duplicate position sweep;
P pair-tiled lists of edge indices; N subtrees one bit away from colliding at one level, or in
the last digit (level 1 built here, the levels above from tools/eh_near_collisions.py's files);
Z constant lists; G grafts, random lists, first indices one bit apart, wrong lengths.
"""
import collections
import json
import os
import random
import struct
import time

import numpy as np

from bitcoincashplus_amd.utils import equihash_ref as R

COLLISION, ORDER, DUP, FINAL, LENGTH = R.COLLISION, R.ORDER, R.DUP, R.FINAL, R.LENGTH
SEED = 0xE901
SALT = b"near"
PARAMS = [(48, 5), (96, 5), (200, 9), (96, 3)]
DATA_96_3 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "equihash_96_3.json")

# the CPU verifier's reason for a vector whose mask is exactly one bit
REASON = {COLLISION: "invalid-collision", ORDER: "index-tree-incorrectly-ordered", DUP: "duplicate-indices",
          FINAL: "nonzero-final-xor", LENGTH: "invalid-solution-length"}
# family -> the one mask it isolates (S: its right-child and root swaps, label S.right. / S.root.)
ISOLATES = {"S": ORDER, "X": COLLISION, "F": FINAL, "T": COLLISION, "U": DUP}

Vector = collections.namedtuple("Vector", "label data soln mask")


def header_input(nonce: int, salt: bytes = SALT) -> bytes:
    # CEquihashInput (108 B) || nNonce (32 B), as tests/test_equihash.py
    return (salt + bytes(108))[:108] + struct.pack("<I", nonce) + bytes(28)


class Params:
    def __init__(self, n, k):
        self.n, self.k = n, k
        self.db = n // (k + 1)          # bits of a digit
        self.iph = 512 // n             # indices per hash
        self.leaves = 1 << k
        self.index_bits = self.db + 1
        self.width = self.leaves * self.index_bits // 8

    def pack(self, idx):
        assert len(idx) == self.leaves and all(0 <= i < 1 << self.index_bits for i in idx)
        return R.minimal_from_indices(list(idx), self.db)

    def unpack(self, soln):
        return R.indices_from_minimal(soln, self.db)


def min_counts(n, k, material, wagner):
    """The least number of vectors of each family in a set built from `material` valid solutions
    (0: no accept side) and, if `wagner`, the near-solutions of a Wagner run; worked out from the
    constructions. Per solution: S has, at each level l < k-1, min(3, 2^(k-2-l)) right-child nodes
    (first, middle, last) and as many left-child ones, plus the root; X has two re-pairings of
    min(3, 2^(k-2-l)) nodes at each level l < k-1; D has (0,1), (0,L-1), (L/2-1,L/2), (L-2,L-1),
    two pairs per distance 2^m (those of distance 1 are among the four) and 16 random ones."""
    per_level = sum(min(3, 1 << (k - 2 - l)) for l in range(k - 1))
    db = n // (k + 1)
    # P: a twin per edge index and a near partner for at least half the bits of digit 0 (at (96,3)
    # the capped scan finds one for a bit with probability 1 - exp(-7/4), about 0.8). N: the 2^DB
    # pairs of a whole index space hold many pairs of pairs for every bit.
    counts = {"P": (7 if 512 // n > 2 else 6) + db // 2, "Z": 3, "G": 32 + 4 + 2}
    # from the committed near-collisions of a whole run: every bit of every level, and the single-bit
    # last digits that the run has (about two rows expected per bit)
    counts["N"] = {(48, 5): db + 1, (96, 5): db + 1, (200, 9): db + 1 + (k - 2) * db + db // 2,
                   (96, 3): (k - 1) * db + db // 2}[(n, k)]
    if material:
        counts.update(V=material, S=material * (2 * per_level + 1), X=material * 2 * per_level,
                      D=material * (2 * k + 18), G=counts["G"] + 1)
    if wagner:
        counts.update(F=64 + db // 2, T=64 + db // 2)  # each bit: two pairs expected at (96,5), more at (48,5)
        if (n, k) == (48, 5):
            counts["U"] = 8
    return counts


# ------------------------------------------------------------------ Wagner rounds in Python
def wagner_rounds(p, data, rounds, keep_shared=False):
    """`rounds` collision rounds of R.solve's table on integers: rows (remaining bit string, index
    tuple), paired within the groups of equal leading digit, the smaller index tuple in front.
    With keep_shared, pairs that share an index stay in (family U)."""
    bits = p.n
    rows = [(R.leaf_value(p.n, p.k, data, i), (i,)) for i in range(1 << p.index_bits)]
    for _ in range(rounds):
        bits -= p.db
        groups = collections.defaultdict(list)
        for row in rows:
            groups[row[0] >> bits].append(row)
        low = (1 << bits) - 1
        rows = []
        for g in groups.values():
            for a in range(len(g)):
                xa, ia = g[a]
                for b in range(a + 1, len(g)):
                    xb, ib = g[b]
                    if not keep_shared and not set(ia).isdisjoint(ib):
                        continue
                    rows.append(((xa ^ xb) & low, ia + ib if ia < ib else ib + ia))
    return rows


def near_solutions(p, data, keep_shared=False):
    """(finals, tops, full) from the rows after k-1 rounds, which keep digits k-1 and k: the pairs
    that collide on digit k-1 only and on digit k only, as (index tuple, the XOR of the digit that
    differs), and the index tuples of those that collide on both."""
    rows = wagner_rounds(p, data, p.k - 1, keep_shared)
    digit = (1 << p.db) - 1
    finals, tops, full = [], [], []

    def pairs(key):
        groups = collections.defaultdict(list)
        for row in rows:
            groups[key(row[0])].append(row)
        for g in groups.values():
            for a in range(len(g)):
                for b in range(a + 1, len(g)):
                    if keep_shared or set(g[a][1]).isdisjoint(g[b][1]):
                        yield g[a], g[b]

    def join(ra, rb):
        return ra[1] + rb[1] if ra[1] < rb[1] else rb[1] + ra[1]

    for ra, rb in pairs(lambda x: x >> p.db):
        diff = (ra[0] ^ rb[0]) & digit
        if diff:
            finals.append((join(ra, rb), diff))
        else:
            full.append(join(ra, rb))
    for ra, rb in pairs(lambda x: x & digit):
        diff = (ra[0] ^ rb[0]) >> p.db
        if diff:
            tops.append((join(ra, rb), diff))
    return finals, tops, full


def strictly_ordered(idx):
    """Every node's left first index is below its right first index."""
    w = 1
    while w < len(idx):
        if any(idx[a] >= idx[a + w] for a in range(0, len(idx), 2 * w)):
            return False
        w *= 2
    return True


# ------------------------------------------------------------------ the leading bits of an index range
HEAD_BITS = 48  # digits 0 and 1 of every set fit: 2 * 24 bits at (96,3)


def leaf_heads(p, data, lo, hi):
    """The leading HEAD_BITS bits of the leaf string of every index in [lo, hi), a numpy uint64
    array (lo a multiple of indices-per-hash): one BLAKE2b per hash, the slicing in numpy."""
    assert lo % p.iph == 0 and p.n >= HEAD_BITS
    base = R.base_hasher(p.n, p.k, data)
    out = []
    g0, g1 = lo // p.iph, (hi + p.iph - 1) // p.iph
    nbytes = p.n // 8
    for c0 in range(g0, g1, 1 << 16):
        c1 = min(g1, c0 + (1 << 16))
        raw = np.frombuffer(b"".join(R.generate_hash(base, g) for g in range(c0, c1)), dtype=np.uint8)
        lead = raw.reshape(-1, nbytes)[:, :HEAD_BITS // 8].astype(np.uint64)
        head = np.zeros(len(lead), dtype=np.uint64)
        for q in range(HEAD_BITS // 8):
            head = (head << np.uint64(8)) | lead[:, q]
        out.append(head)
    return np.concatenate(out)[:hi - lo]


# ------------------------------------------------------------------ the builder
class _Builder:
    def __init__(self, p):
        self.p = p
        self.rng = random.Random(SEED ^ (p.n << 8) ^ p.k)
        self.vectors = []
        self.labels = set()
        self.notes = []

    def add(self, label, data, soln, expect=None):
        """`expect`: the mask the construction promises (None: whatever the oracle gives)."""
        assert label not in self.labels, label
        self.labels.add(label)
        mask = R.check_mask(self.p.n, self.p.k, data, soln)
        if expect is not None:
            assert mask == expect, f"{label}: constructed for mask {expect}, the oracle says {mask}"
        self.vectors.append(Vector(label, data, soln, mask))
        return mask

    def add_idx(self, label, data, idx, expect=None):
        return self.add(label, data, self.p.pack(idx), expect)


def _spread(items):
    """First, middle and last of a list, without repeats."""
    if not items:
        return []
    out = []
    for x in (items[0], items[len(items) // 2], items[-1]):
        if x not in out:
            out.append(x)
    return out


def _swap_family(b, tag, data, idx):
    p = b.p
    for l in range(p.k):
        w = 1 << l
        nodes = list(range(p.leaves // (2 * w)))

        def swapped(j):
            s = j * 2 * w
            return idx[:s] + idx[s + w:s + 2 * w] + idx[s:s + w] + idx[s + 2 * w:]

        if l == p.k - 1:
            b.add_idx(f"S.root.l{l}.{tag}", data, swapped(0), ORDER)
            continue
        for j in _spread([j for j in nodes if j & 1]):
            b.add_idx(f"S.right.l{l}.j{j}.{tag}", data, swapped(j), ORDER)
        for j in _spread([j for j in nodes if not j & 1]):
            mask = b.add_idx(f"S.left.l{l}.j{j}.{tag}", data, swapped(j))
            assert mask & ORDER and not mask & ~ORDER, (l, j, mask)


def _cross_family(b, tag, data, idx):
    p = b.p
    for l in range(p.k - 1):
        w = 1 << l
        for j in _spread(list(range(p.leaves // (4 * w)))):
            s = j * 4 * w
            a, bb, c, d = (idx[s + q * w:s + (q + 1) * w] for q in range(4))
            for name, left, right in (("ac_bd", a + c, sorted([bb, d])), ("ad_bc", a + d, sorted([bb, c]))):
                lst = idx[:s] + left + right[0] + right[1] + idx[s + 4 * w:]
                mask = b.add_idx(f"X.{name}.l{l}.j{j}.{tag}", data, lst)
                assert mask in (0, COLLISION), (l, j, mask)  # 0: the wrong pair collides too


def _dup_family(b, tag, data, idx):
    p = b.p
    L = p.leaves
    pairs = [(0, 1), (0, L - 1), (L // 2 - 1, L // 2), (L - 2, L - 1)]
    for m in range(p.k):
        for pair in ((0, 1 << m), (L - 1 - (1 << m), L - 1)):
            if pair not in pairs:
                pairs.append(pair)
    assert len(pairs) == 2 * p.k + 2
    while len(pairs) < 2 * p.k + 18:
        pair = (b.rng.randrange(L), b.rng.randrange(L))
        if pair[0] != pair[1] and pair not in pairs:
            pairs.append(pair)
    for a, q in pairs:
        lst = list(idx)
        lst[q] = lst[a]
        mask = b.add_idx(f"D.p{a}.q{q}.{tag}", data, lst)
        assert mask & DUP, (a, q, mask)


def _pair_tiled(b, data):
    """P: for each edge index e a partner with the same digit 0 (one pass over the index space with
    numpy, capped at 2^22 indices), tiled (min, max, min, max, ...), and a twin whose partner does
    not collide; for each bit of digit 0 a pair (an edge index, a partner) whose digits 0 differ
    in that bit alone. Returns the scanned leaf heads."""
    p = b.p
    edges = sorted({0, 1, p.iph - 1, p.iph, (1 << p.db) - 1, 1 << p.db, (1 << (p.db + 1)) - 1})
    want = {e: R.leaf_value(p.n, p.k, data, e) >> (p.n - p.db) for e in edges}
    span = min(1 << p.index_bits, 1 << 22)
    heads = leaf_heads(p, data, 0, span)
    digits = heads >> np.uint64(HEAD_BITS - p.db)
    tile = p.leaves // 2
    for e in edges:
        hits = [int(i) for i in np.flatnonzero(digits == want[e]) if int(i) != e]
        if hits:
            partner = hits[0]
            assert R.leaf_value(p.n, p.k, data, partner) >> (p.n - p.db) == want[e]
            b.add_idx(f"P.collide.e{e}", data, sorted([e, partner]) * tile, ORDER | DUP)
        else:
            b.notes.append(f"P: no partner for index {e} among the first {span} indices")
        other = next(i for i in range(2, span) if i != e and int(digits[i]) != want[e])
        b.add_idx(f"P.twin.e{e}", data, sorted([e, other]) * tile, COLLISION | ORDER | DUP)
    for bit in range(p.db):
        for e in edges:
            hits = np.flatnonzero(digits == (want[e] ^ (1 << bit)))
            if len(hits):
                b.add_idx(f"P.near.bit{bit}.e{e}", data, sorted([e, int(hits[0])]) * tile, COLLISION | ORDER | DUP)
                break
        else:
            b.notes.append(f"P: no edge index has a partner one bit away in bit {bit} of digit 0")
    return heads


def _near_level1(b, data, heads):
    """N: two pairs that each collide on digit 0 and whose XORs differ in one bit of digit 1 alone,
    tiled (a, b, c, d, a, b, c, d, ...): level 0 collides, level 1 differs in that bit, every
    level above compares equal halves and the final digit is zero. One list per bit of digit 1 and
    one whose pairs collide on digit 1 as well. Needs the heads of the whole index space."""
    p = b.p
    assert len(heads) == 1 << p.index_bits
    mask = np.uint64((1 << p.db) - 1)
    d0 = heads >> np.uint64(HEAD_BITS - p.db)
    d1 = (heads >> np.uint64(HEAD_BITS - 2 * p.db)) & mask
    order = np.argsort(d0, kind="stable")
    sorted_d0 = d0[order]
    adjacent = np.flatnonzero(sorted_d0[:-1] == sorted_d0[1:])
    pa, pb = order[adjacent], order[adjacent + 1]  # pa < pb: the sort is stable
    pd = d1[pa] ^ d1[pb]
    by_pd = np.argsort(pd, kind="stable")
    spd = pd[by_pd]

    def quad(diff):
        """The first two pairs of four distinct indices whose digit-1 XORs differ by `diff`; the
        first of the two is looked for among the first 2^16 pairs, which is plenty."""
        target = pd[:1 << 16] ^ np.uint64(diff)
        pos = np.minimum(np.searchsorted(spd, target), len(spd) - 1)
        for h in np.flatnonzero(spd[pos] == target):
            q = by_pd[pos[h]]
            four = [int(pa[h]), int(pb[h]), int(pa[q]), int(pb[q])]
            if len(set(four)) == 4:
                return four if four[0] < four[2] else four[2:] + four[:2]
        return None

    tile = p.leaves // 4
    for bit in range(p.db):
        four = quad(1 << bit)
        if four is None:
            b.notes.append(f"N: no two pairs one bit apart in bit {bit} of digit 1")
        else:
            b.add_idx(f"N.l1.bit{bit}", data, four * tile, COLLISION | ORDER | DUP)
    four = quad(0)
    if four is not None:
        b.add_idx("N.l1.collide", data, four * tile, ORDER | DUP)


def near_file(n, k):
    return os.path.join(os.path.dirname(DATA_96_3), f"equihash_near_{n}_{k}.json")


def _near_committed(b):
    """N, the levels a test cannot build: the near-collisions of a whole Wagner run written by
    tools/eh_near_collisions.py, as index lists of two subtrees (tiled here to a whole list) or of a
    whole tree. Only the indices come from the file; every mask is the oracle's."""
    p = b.p
    with open(near_file(p.n, p.k)) as f:
        doc = json.load(f)
    data = bytes.fromhex(doc["input"])
    for e in doc["lists"]:
        idx = e["indices"] * (p.leaves // len(e["indices"]))
        if e["level"] == "final":
            mask = b.add_idx(f"N.final.bit{e['bit']}", data, idx)
            assert mask & FINAL and not mask & COLLISION, (e["bit"], mask)
        elif len(e["indices"]) < p.leaves:
            b.add_idx(f"N.l{e['level']}.bit{e['bit']}", data, idx, COLLISION | ORDER | DUP)
        else:
            mask = b.add_idx(f"N.l{e['level']}.bit{e['bit']}", data, idx)
            assert mask & COLLISION, (e["bit"], mask)


def _constants(b, data):
    p = b.p
    b.add("Z.zero_bytes", data, bytes(p.width), ORDER | DUP)
    b.add("Z.one_bytes", data, b"\xff" * p.width, ORDER | DUP)
    b.add_idx("Z.mid_index", data, [1 << p.db] * p.leaves, ORDER | DUP)


def _general(b, data, base_idx, second_idx):
    """G. base_idx: a valid solution's indices, or None (then a random list is the material)."""
    p = b.p
    L, top = p.leaves, 1 << p.db
    rnd = [[b.rng.randrange(1 << p.index_bits) for _ in range(L)] for _ in range(32)]
    for i, lst in enumerate(rnd):
        b.add_idx(f"G.random.{i}", data, lst)
    idx = list(base_idx) if base_idx is not None else rnd[0]
    if second_idx is not None:
        for l in range(p.k):
            w = 1 << l
            s = (b.rng.randrange(L // w)) * w
            b.add_idx(f"G.graft.l{l}.at{s}", data, idx[:s] + list(second_idx[s:s + w]) + idx[s + w:])
    if base_idx is not None:
        b.add_idx("G.left_half_twice", data, idx[:L // 2] * 2)
    # first indices of the two children of the level-(k-1)//2 node 0 one bit apart, both orders
    w = 1 << ((p.k - 1) // 2)
    for name, bit in (("top_bit", top), ("low_bit", 1)):
        v = idx[0] & ~bit
        for order, (x, y) in (("up", (v, v | bit)), ("down", (v | bit, v))):
            lst = list(idx)
            lst[0], lst[w] = x, y
            mask = b.add_idx(f"G.{name}.{order}", data, lst)
            assert mask & ORDER or order == "up", (name, order, mask)
    good = p.pack(idx)
    b.add("G.short_by_one", data, good[:-1], LENGTH)
    b.add("G.long_by_one", data, good + b"\0", LENGTH)


class VectorSet:
    def __init__(self, p, vectors, valid, material, wagner, notes, seconds):
        self.p, self.n, self.k = p, p.n, p.k
        self.vectors, self.valid, self.notes, self.seconds = vectors, valid, notes, seconds
        self.material, self.wagner = material, wagner  # solutions behind S, X and D; F and T built

    def family(self, f):
        return [v for v in self.vectors if v.label.split(".")[0] == f]

    def counts(self):
        return dict(collections.Counter(v.label.split(".")[0] for v in self.vectors))


def load_96_3():
    """The committed (96,3) solutions (tools/eh_solve_96_3.py): [(input140, solution)], each
    re-checked by the oracle."""
    with open(DATA_96_3) as f:
        entries = json.load(f)["solutions"]
    out = [(bytes.fromhex(e["input"]), bytes.fromhex(e["solution"])) for e in entries]
    for data, soln in out:
        assert R.is_valid_solution(96, 3, data, soln)
    return out


def solve_valid(native, n, k, gpu=False):
    """[(input140, solution)] of the accept side. (48,5): the oracle's solver on nonces 0..15;
    (96,5): the CPU solver on nonces 0..7; (200,9): one 8-nonce GPU solve (gpu=True) or nothing;
    (96,3): the committed file. Every solution is confirmed by R.is_valid_solution."""
    out = []
    if (n, k) == (48, 5):
        for nonce in range(16):
            out += [(header_input(nonce), s) for s in R.solve(n, k, header_input(nonce))]
    elif (n, k) == (96, 3):
        return load_96_3()
    elif (n, k) == (96, 5) or gpu:
        inputs = [header_input(nonce) for nonce in range(8)]
        states = []
        for data in inputs:
            st = native.EquihashState(n, k)
            st.update(data)
            states.append(st)
        found = native.EquihashGpuSolver(n, k, 8).solve(states) if (n, k) == (200, 9) else \
            [native.eh_solve_cpu(n, k, st)[0] for st in states]
        for data, sols in zip(inputs, found):
            out += [(data, bytes(s)) for s in sorted(sols)]
    for data, soln in out:
        assert R.is_valid_solution(n, k, data, soln)
    return out


def build(native, n, k, valid=None, gpu=False):
    """The vectors of one parameter set. `valid`: the accept side if the caller has it already,
    else solve_valid(native, n, k, gpu). Without an accept side ((200,9) with no GPU) only the
    families that need none are built: P, N, Z and G."""
    t0 = time.time()
    p = Params(n, k)
    b = _Builder(p)
    if valid is None:
        valid = solve_valid(native, n, k, gpu)
    for i, (data, soln) in enumerate(valid):
        b.add(f"V.{i}", data, soln, 0)
    if valid:
        seen = {i % p.iph for _, soln in valid for i in p.unpack(soln)}
        assert seen == set(range(p.iph)), f"hash slices never used by an accepted vector: {set(range(p.iph)) - seen}"
    # material of S, X and D: every solution of the small set, three of the others
    material = valid if (n, k) == (48, 5) else valid[:3]
    for i, (data, soln) in enumerate(material):
        idx = p.unpack(soln)
        _swap_family(b, f"v{i}", data, idx)
        _cross_family(b, f"v{i}", data, idx)
        _dup_family(b, f"v{i}", data, idx)
    wagner = (n, k) in ((48, 5), (96, 5))
    if wagner:
        finals, tops, dups = [], [], []
        for nonce in range(16 if n == 48 else 1):
            data = header_input(nonce)
            f, t, _ = near_solutions(p, data)
            finals += [(idx, nonce, diff) for idx, diff in f]
            tops += [(idx, nonce, diff) for idx, diff in t]
            if n == 48:
                _, _, full = near_solutions(p, data, keep_shared=True)
                dups += [(idx, nonce, 0) for idx in full if len(set(idx)) < len(idx) and strictly_ordered(idx)]
        for fam, found, mask in (("F", finals, FINAL), ("T", tops, COLLISION), ("U", dups, DUP)):
            found = sorted(set(found))
            for i, (idx, nonce, _) in enumerate(found[:64]):
                b.add_idx(f"{fam}.{i}.n{nonce}", header_input(nonce), list(idx), mask)
            # the first pair after those whose digit differs in one bit alone, for every bit
            for bit in range(p.db if fam != "U" else 0):
                one = next((x for x in found[64:] if x[2] == 1 << bit), None)
                if one is None:
                    b.notes.append(f"{fam}: no pair one bit apart in bit {bit}")
                else:
                    b.add_idx(f"{fam}.bit{bit}.n{one[1]}", header_input(one[1]), list(one[0]), mask)
    data0 = valid[0][0] if valid else header_input(0)
    heads = _pair_tiled(b, data0)
    if len(heads) == 1 << p.index_bits:
        _near_level1(b, data0, heads)
    if os.path.exists(near_file(n, k)):
        _near_committed(b)
    _constants(b, data0)
    # a nonce with two solutions for the grafts
    by_data = collections.defaultdict(list)
    for data, soln in valid:
        by_data[data].append(p.unpack(soln))
    twice = next((d for d, sols in by_data.items() if len(sols) >= 2), None)
    if twice is not None:
        _general(b, twice, by_data[twice][0], by_data[twice][1])
    elif valid:
        b.notes.append("G: no nonce with two solutions, no grafts")
        _general(b, valid[0][0], p.unpack(valid[0][1]), None)
    else:
        _general(b, data0, None, None)
    return VectorSet(p, b.vectors, valid, len(material), wagner, b.notes, time.time() - t0)
