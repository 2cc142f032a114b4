"""Transaction lists and wallets for the wallet scan tests (tests/test_wallet_scan.py on the CPU,
tests/test_wallet_scan_gpu.py with the match passes on the device): each case is built once per
session, and its expectation is either spelled out here or the reference loop's
(native.wallet_scan_reference, CWallet::AddToWalletIfInvolvingMe per transaction)."""
import functools
import random
import struct

from bitcoincashplus_amd import native
from bitcoincashplus_amd.testing.messages import COutPoint, CTransaction, CTxIn, CTxOut, hash256

OP_RETURN = b"\x6a"


def push(data: bytes, form: int = 0) -> bytes:
    """form 0: the shortest direct push; 1, 2, 4: OP_PUSHDATA1 / 2 / 4."""
    if form == 0:
        assert len(data) < 76
        return bytes([len(data)]) + data
    if form == 1:
        return b"\x4c" + bytes([len(data)]) + data
    if form == 2:
        return b"\x4d" + struct.pack("<H", len(data)) + data
    return b"\x4e" + struct.pack("<I", len(data)) + data


def p2pkh(h20: bytes, form: int = 0) -> bytes:
    return b"\x76\xa9" + push(h20, form) + b"\x88\xac"


def p2pk(pub: bytes, form: int = 0) -> bytes:
    return push(pub, form) + b"\xac"


def p2sh(h20: bytes, form: int = 0) -> bytes:
    return b"\xa9" + push(h20, form) + b"\x87"


def multisig_1of2(a: bytes, b: bytes, form: int = 0) -> bytes:
    return b"\x51" + push(a, form) + push(b, form) + b"\x52\xae"


def fake_pubkey(rng, compressed: bool = True) -> bytes:
    """IsMine hashes a public key and never checks the curve point."""
    return (b"\x02" + rng.randbytes(32)) if compressed else (b"\x04" + rng.randbytes(64))


class Tx:
    """A serialized transaction with its txid (internal byte order) and outpoints."""

    def __init__(self, ins, outs):
        t = CTransaction()
        for txid, n in ins:
            t.vin.append(CTxIn(COutPoint(int.from_bytes(txid, "little"), n), b""))
        for i, spk in enumerate(outs):
            t.vout.append(CTxOut(1000 + i, spk))
        self.raw = t.serialize()
        self.txid = hash256(self.raw)

    def outpoint(self, n: int) -> bytes:
        return self.txid + struct.pack("<I", n)


def fresh(rng, outs):
    return Tx([(rng.randbytes(32), rng.randrange(4))], outs)


class Wallet:
    """Three keys, a redeem script of ours, one that is known but pays someone else, and a
    nonstandard watch-only script."""

    def __init__(self, rng):
        self.p1 = fake_pubkey(rng)
        self.p2 = fake_pubkey(rng, compressed=False)
        self.p3 = fake_pubkey(rng)
        self.h1, self.h2, self.h3 = (native.hash160(p) for p in (self.p1, self.p2, self.p3))
        self.redeem_mine = p2pk(self.p3)
        self.redeem_other = p2pkh(rng.randbytes(20))
        self.watch = b"\x51\x75\x51\x75\x51"
        self.wallet_txs = []

    def desc(self):
        return dict(pubkeys=[self.p1, self.p2, self.p3], scripts=[self.redeem_mine, self.redeem_other],
                    watch=[self.watch], wallet_txs=[t.raw for t in self.wallet_txs])


def random_block(rng, ntx, ours, key_hashes):
    """2-in/2-out transactions, a third of them spending an earlier one of the list; those at the
    positions `ours` pay one of the wallet's keys."""
    txs = []
    for i in range(ntx):
        ins = []
        for _ in range(2):
            if i and rng.randrange(3) == 0:
                ins.append((txs[rng.randrange(i)].txid, rng.randrange(2)))
            else:
                ins.append((rng.randbytes(32), rng.randrange(4)))
        first = p2pkh(rng.choice(key_hashes) if i in ours else rng.randbytes(20))
        second = p2pkh(rng.randbytes(20)) if rng.randrange(8) else p2pk(fake_pubkey(rng))
        txs.append(Tx(ins, [first, second]))
    return txs


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(txs=[raw], wallet=desc, f_update=bool, verdicts=[bool] or None, true_hits=int).
    true_hits counts, by construction, the transactions that hold a real member of the wallet's
    sets and are still not added (a multisig with one key ours, a double spend): the match flags
    them rightly, so they are no false positives of the fingerprints."""
    out = {}

    def add(name, txs, wallet, verdicts=None, f_update=True, true_hits=0):
        out[name] = dict(txs=[t.raw for t in txs], wallet=wallet, f_update=f_update, verdicts=verdicts,
                         true_hits=true_hits)

    rng = random.Random(2101)
    w = Wallet(rng)
    other = fake_pubkey(rng)
    stranger = rng.randbytes(20)

    # one transaction per branch of IsMine
    branches = [
        (p2pkh(w.h1), True),
        (p2pk(w.p1), True),
        (p2pk(w.p2), True),  # uncompressed
        (p2sh(native.hash160(w.redeem_mine)), True),
        (p2sh(rng.randbytes(20)), False),  # unknown script
        (p2sh(native.hash160(w.redeem_other)), False),  # known script that pays someone else
        (multisig_1of2(w.p1, other), False),  # one key ours: not mine
        (multisig_1of2(w.p1, w.p3), True),
        (w.watch, True),
        (OP_RETURN + push(b"wallet scan"), False),
        (p2pkh(stranger), False),
        (p2pk(other), False),
    ]
    add("ismine_branches", [fresh(rng, [spk]) for spk, _ in branches], w.desc(), [mine for _, mine in branches],
        true_hits=2)  # the known script that pays someone else, the multisig with one key ours

    # the same templates with OP_PUSHDATA1 / 2 / 4 pushes; P2SH is a byte pattern, so a pushdata
    # form of it is nonstandard even for a known script
    forms = []
    for form in (1, 2, 4):
        forms += [
            (p2pkh(w.h1, form), True),
            (p2pk(w.p1, form), True),
            (p2pk(w.p2, form), True),
            (multisig_1of2(w.p1, w.p3, form), True),
            (multisig_1of2(w.p1, other, form), False),
            (p2sh(native.hash160(w.redeem_mine), form), False),
            (p2pkh(stranger, form), False),
        ]
    add("pushdata_forms", [fresh(rng, [spk]) for spk, _ in forms], w.desc(), [mine for _, mine in forms],
        true_hits=6)  # per form: the multisig with one key ours, the known script id

    # GetOp failures: Solver gives up, whatever came before the failure
    truncated = [
        b"\x21" + w.p1[:10],  # a push that runs past the end
        p2pkh(w.h1) + b"\x4c",  # OP_PUSHDATA1 without its length byte
        p2pkh(w.h1) + b"\x4d\x01",  # OP_PUSHDATA2 with half its length
        p2pk(w.p1) + b"\x4e\xff\xff\xff\xff",  # OP_PUSHDATA4 of 4 GiB
        b"\x4c",
    ]
    add("truncated_push", [fresh(rng, [spk]) for spk in truncated], w.desc(), [False] * len(truncated),
        true_hits=3)  # our key hash or key is pushed before the failure

    # CPubKey clears a key whose header byte does not announce its length
    bad = [p2pk(b"\x05" + w.p1[1:]), p2pk(b"\x02" + rng.randbytes(33)), p2pk(b"\x04" + rng.randbytes(32)),
           multisig_1of2(b"\x05" + w.p1[1:], w.p3)]
    add("bad_pubkey_header", [fresh(rng, [spk]) for spk in bad], w.desc(), [False] * len(bad),
        true_hits=1)  # the multisig's second key is ours

    add("empty_script", [fresh(rng, [b""]), fresh(rng, [b"", p2pkh(w.h2)])], w.desc(), [False, True])

    # growth inside the list: A pays us, B spends A and pays us, C spends B; D has nothing to do with it
    a = fresh(rng, [p2pkh(w.h1)])
    b = Tx([(a.txid, 0)], [p2pkh(w.h2)])
    c = Tx([(b.txid, 0)], [p2pkh(stranger)])
    d = fresh(rng, [p2pkh(stranger)])
    add("chain_abc", [d, a, d, b, c, d], w.desc(), [False, True, False, True, True, False])
    # B before A: when B is judged A is not in the wallet, and B's own output is a stranger's
    b2 = Tx([(a.txid, 0)], [p2pkh(stranger)])
    add("reversed_ba", [b2, a], w.desc(), [False, True])

    # a transaction the wallet already has, fUpdate both ways
    known = Wallet(rng)
    x = fresh(rng, [p2pkh(known.h1)])
    known.wallet_txs = [x]
    spends_x = Tx([(x.txid, 0)], [p2pkh(stranger)])
    add("existing_update", [d, x, spends_x], known.desc(), [False, True, True], f_update=True)
    add("existing_no_update", [d, x, spends_x], known.desc(), [False, False, True], f_update=False)

    # double spends: of an input of a wallet transaction, and of an input of one added by the list
    q = (rng.randbytes(32), 1)
    ours = Tx([q], [p2pkh(known.h2)])
    twice = Tx([q], [p2pkh(stranger)])
    x_in = CTransaction()
    x_in.deserialize(__import__("io").BytesIO(x.raw))
    first_in = (x_in.vin[0].prevout.hash.to_bytes(32, "little"), x_in.vin[0].prevout.n)
    conflicts_x = Tx([first_in], [p2pkh(stranger)])
    add("double_spend", [ours, d, twice, conflicts_x], known.desc(), [True, False, False, False],
        true_hits=2)  # both double spends hit a spent outpoint

    add("empty_wallet", random_block(random.Random(5), 50, set(), [stranger]), dict(), [False] * 50)
    add("empty_list", [], w.desc(), [])

    # a 3,000-transaction block with 30 of ours (and whatever spends them later in the list)
    rb = random.Random(3000)
    big = Wallet(rb)
    hashes = [big.h1, big.h2, big.h3]
    extra = [fake_pubkey(rb) for _ in range(37)]
    desc = big.desc()
    desc["pubkeys"] = desc["pubkeys"] + extra
    hashes += [native.hash160(p) for p in extra]
    positions = set(rb.sample(range(3000), 30))
    add("random_block", random_block(rb, 3000, positions, hashes), desc, None)
    return out


def check_scan(case, use_gpu):
    """The scan against the reference loop: verdicts, wallet transactions (with their block and
    position) and spent outpoints. Returns (info, verdicts)."""
    want = native.wallet_scan_reference(case["txs"], case["wallet"], case["f_update"])
    verdicts, wtxs, spent, info = native.wallet_scan(case["txs"], case["wallet"], use_gpu, case["f_update"])
    if case["verdicts"] is not None:
        assert list(want[0]) == case["verdicts"]
    assert list(verdicts) == list(want[0])
    assert list(wtxs) == list(want[1])
    assert list(spent) == list(want[2])
    return info, list(verdicts)


def rerun_cap(case, verdicts):
    """cpu_reruns may not pass: transactions the loop adds + already-known ones + 1% of the list,
    and the case's true hits that are not added."""
    known = len(case["wallet"].get("wallet_txs", []))
    return sum(verdicts) + known + len(case["txs"]) // 100 + case["true_hits"]
