"""Transaction lists and filters for the BIP37 scan tests (tests/test_bloom_scan.py on the CPU,
tests/test_bloom_gpu.py with the membership passes on the device): each case is built once per
session, and its expectation is either spelled out here or the reference loop's
(native.bloom_scan_reference, CBloomFilter::IsRelevantAndUpdate per transaction)."""
import functools
import random
import struct

from bitcoincashplus_amd import native
from bitcoincashplus_amd.testing.messages import COutPoint, CTransaction, CTxIn, CTxOut, hash256, ser_string

UPDATE_NONE, UPDATE_ALL, UPDATE_P2PUBKEY_ONLY = 0, 1, 2
M32 = 0xFFFFFFFF


def push(data: bytes) -> bytes:
    assert 0 < len(data) < 76
    return bytes([len(data)]) + data


def p2pkh(h20: bytes) -> bytes:
    return b"\x76\xa9" + push(h20) + b"\x88\xac"


def p2pk(pub: bytes) -> bytes:
    return push(pub) + b"\xac"


def multisig_1of2(a: bytes, b: bytes) -> bytes:
    return b"\x51" + push(a) + push(b) + b"\x52\xae"


def fake_pubkey(rng) -> bytes:
    return b"\x02" + rng.randbytes(32)


class Tx:
    """A serialized transaction with its txid (internal byte order) and outpoints."""

    def __init__(self, ins, outs):
        t = CTransaction()
        for (txid, n), script_sig in ins:
            t.vin.append(CTxIn(COutPoint(int.from_bytes(txid, "little"), n), script_sig))
        for i, spk in enumerate(outs):
            t.vout.append(CTxOut(1000 + i, spk))
        self.raw = t.serialize()
        self.txid = hash256(self.raw)

    def outpoint(self, n: int) -> bytes:
        return self.txid + struct.pack("<I", n)


class Filter:
    """CBloomFilter's data, insert and filterload payload."""

    def __init__(self, size: int, n_hash: int, tweak: int, flags: int, fill: int = 0):
        self.data = bytearray([fill]) * size
        self.n_hash, self.tweak, self.flags = n_hash, tweak, flags

    @classmethod
    def sized(cls, n_elements: int, fp: float, tweak: int, flags: int):
        import math
        size = int(min(-1 / (math.log(2) ** 2) * n_elements * math.log(fp), 36000 * 8) / 8)
        return cls(size, int(min(size * 8 / n_elements * math.log(2), 50)), tweak, flags)

    def bits(self, key: bytes):
        return [native.murmur3((i * 0xFBA4C795 + self.tweak) & M32, key) % (len(self.data) * 8) for i in range(self.n_hash)]

    def insert(self, key: bytes):
        for bit in self.bits(key):
            self.data[bit >> 3] |= 1 << (bit & 7)

    def contains(self, key: bytes) -> bool:
        return all(self.data[bit >> 3] >> (bit & 7) & 1 for bit in self.bits(key))

    def ser(self) -> bytes:
        return ser_string(bytes(self.data)) + struct.pack("<IIB", self.n_hash, self.tweak, self.flags)


def _spend(rng, tx, n):
    return Tx([((tx.txid, n), b"")], [p2pkh(rng.randbytes(20))])


def _fresh(rng, outs, script_sig=b""):
    return Tx([((rng.randbytes(32), rng.randrange(4)), script_sig)], outs)


def random_block(rng, ntx):
    txs, key_hashes = [], []
    for i in range(ntx):
        prev = (rng.randbytes(32), rng.randrange(4))
        if i and rng.randrange(3) == 0:  # a third spend an earlier transaction of the list
            prev = (txs[rng.randrange(i)].txid, rng.randrange(2))
        key_hashes.append(rng.randbytes(20))
        second = p2pkh(rng.randbytes(20)) if rng.randrange(8) else p2pk(fake_pubkey(rng))
        txs.append(Tx([(prev, push(rng.randbytes(71 + rng.randrange(2))) + push(fake_pubkey(rng)))],
                      [p2pkh(key_hashes[-1]), second]))
    return txs, key_hashes


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(txs=[raw], filter=payload, verdicts=[bool] or None, unchanged=bool)."""
    out = {}

    def add(name, txs, f, verdicts=None, unchanged=False):
        out[name] = dict(txs=[t.raw for t in txs], filter=f.ser(), verdicts=verdicts, unchanged=unchanged)

    # UPDATE_NONE: key hashes, a txid, an outpoint and a scriptSig public key; nothing is inserted
    rng = random.Random(101)
    sig_keys = [fake_pubkey(rng) for _ in range(40)]
    hashes = [rng.randbytes(20) for _ in range(40)]
    txs = [_fresh(rng, [p2pkh(hashes[i]), p2pkh(rng.randbytes(20))], push(rng.randbytes(71)) + push(sig_keys[i]))
           for i in range(40)]
    txs.append(_spend(rng, txs[3], 0))  # spends a matched output: no match without the insert
    f = Filter.sized(20, 0.0001, 77, UPDATE_NONE)
    for key in (hashes[3], hashes[17], txs[5].txid, txs[9].raw[5:41], sig_keys[21]):
        f.insert(key)
    add("update_none", txs, f, [i in (3, 5, 9, 17, 21) for i in range(41)], unchanged=True)

    # UPDATE_ALL: A pays a watched key hash, B spends A:0 to an unwatched script, C spends B:0
    rng = random.Random(102)
    watched = rng.randbytes(20)
    a = _fresh(rng, [p2pkh(watched)])
    b = _spend(rng, a, 0)
    c = _spend(rng, b, 0)
    f = Filter.sized(10, 0.000001, 5, UPDATE_ALL)
    f.insert(watched)
    add("update_all_chain", [a, b, c], f, [True, True, False])
    add("reversed_order", [b, a], f, [False, True])  # a fixed point over the list would match B

    # P2PUBKEY_ONLY: a P2PKH match inserts nothing, P2PK and bare multisig matches do
    rng = random.Random(103)
    h, pk, m1, m2 = rng.randbytes(20), fake_pubkey(rng), fake_pubkey(rng), fake_pubkey(rng)
    t_pkh, t_pk = _fresh(rng, [p2pkh(h)]), _fresh(rng, [p2pk(pk)])
    t_ms = _fresh(rng, [p2pkh(rng.randbytes(20)), multisig_1of2(m1, m2)])
    f = Filter.sized(10, 0.000001, 9, UPDATE_P2PUBKEY_ONLY)
    for key in (h, pk, m2):
        f.insert(key)
    add("p2pubkey_only", [t_pkh, _spend(rng, t_pkh, 0), t_pk, _spend(rng, t_pk, 0), t_ms, _spend(rng, t_ms, 1),
                          _spend(rng, t_ms, 0)], f, [True, False, True, True, True, True, False])

    # filter edge cases over one list
    rng = random.Random(104)
    txs = [_fresh(rng, [p2pkh(rng.randbytes(20))], push(rng.randbytes(72)) + push(fake_pubkey(rng))) for _ in range(20)]
    add("all_ones", txs, Filter(50, 5, 1, UPDATE_ALL, fill=0xFF), [True] * 20, unchanged=True)
    add("all_zero", txs, Filter(50, 5, 1, UPDATE_ALL), [False] * 20, unchanged=True)
    add("empty_vdata", txs, Filter(0, 5, 1, UPDATE_ALL), [True] * 20, unchanged=True)  # full and empty: full wins

    # a 3,000-transaction block with in-list spends, under each update mode
    rng = random.Random(105)
    txs, key_hashes = random_block(rng, 3000)
    for flags, name in ((UPDATE_NONE, "none"), (UPDATE_ALL, "all"), (UPDATE_P2PUBKEY_ONLY, "p2pubkey")):
        f = Filter.sized(200, 0.001, 4242, flags)
        for i in range(30):
            f.insert(key_hashes[(i * 97) % len(key_hashes)])
        add("random_block_" + name, txs, f)
    # few matches: every insert gets a pass of its own and the passes do not run out
    f = Filter.sized(200, 0.0001, 4243, UPDATE_ALL)
    for i in range(3):
        f.insert(key_hashes[1000 * i + 500])
    add("random_block_few", txs, f)
    return out


@functools.lru_cache(maxsize=None)
def same_transaction_case():
    """2 bytes, 2 hash functions: a transaction whose output 1 does not match the filter as loaded
    but does once the outpoint of its matching output 0 went in (so the loop inserts (tx, 1) too).
    Returns (tries, raw txs, filter payload); tries is None when 1,000 did not find one."""
    rng = random.Random(106)
    watched = rng.randbytes(20)
    for attempt in range(1000):
        f = Filter(2, 2, attempt, UPDATE_ALL)
        f.insert(watched)
        other = rng.randbytes(20)
        tx = _fresh(rng, [p2pkh(watched), p2pkh(other)])
        if f.contains(other) or f.contains(tx.txid):
            continue
        g = Filter(2, 2, attempt, UPDATE_ALL)
        g.data = bytearray(f.data)
        g.insert(tx.outpoint(0))
        if not g.contains(other):
            continue
        return attempt + 1, [tx.raw, _spend(rng, tx, 1).raw], f.ser()
    return None, None, None


def check_scan(raw_txs, filter_ser, use_gpu, verdicts=None, unchanged=False):
    """The scan against the reference loop: verdicts and the filter afterwards. Returns info."""
    want, want_filter = native.bloom_scan_reference(raw_txs, filter_ser)
    got, got_filter, info = native.bloom_scan(raw_txs, filter_ser, use_gpu)
    assert got == want
    assert got_filter == want_filter
    if verdicts is not None:
        assert got == verdicts
    if unchanged:
        assert got_filter == filter_ser
    return info
