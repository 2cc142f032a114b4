"""Wallet matching on the GPU (csrc/kernels/wallet_match.hip): hash160_kernel against the CPU's
CHash160, wallet_match_kernel against its host twin byte for byte, and the batched scan of
transaction lists (csrc/wallet/walletscan.cpp) with its passes on the device against the loop of
AddToWalletIfInvolvingMe: the cases of tests/test_wallet_scan.py with ``use_gpu=True``."""
import random
import struct

import pytest

import wallet_scan_cases
from wallet_scan_cases import check_scan, p2pk, p2pkh, p2sh, multisig_1of2, push, rerun_cap

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 32, 33, 55, 56, 63, 64, 65, 119, 120, 520]
COUNTS = [1, 63, 64, 65, 257]
SALT = bytes(range(100, 116))


def test_hash160_lengths_at_every_alignment(native):
    """Every padding shape of SHA-256 (one to nine blocks, the length alone in a last block) at
    every blob offset mod 4 (the host path packs the messages back to back: one-byte fillers move
    the next one along)."""
    rng = random.Random(160)
    msgs, placed, at = [], set(), 0
    for length in LENGTHS:
        for r in range(4):
            while at % 4 != r:
                msgs.append(rng.randbytes(1))
                at += 1
            msgs.append(rng.randbytes(length))
            placed.add((length, at % 4))
            at += length
    assert placed == {(length, r) for length in LENGTHS for r in range(4)}
    assert native.hash160_gpu(msgs) == [native.hash160(m) for m in msgs]


@pytest.mark.parametrize("count", COUNTS)
def test_hash160_counts(native, count):
    rng = random.Random(count)
    msgs = [rng.randbytes(rng.choice((0, 20, 33, 65, 100, 520))) for _ in range(count)]
    assert native.hash160_gpu(msgs) == [native.hash160(m) for m in msgs]


def test_hash160_rejects_and_cpu_vectors(native):
    with pytest.raises(ValueError):
        native.hash160_gpu([bytes(521)])
    assert native.hash160_gpu([]) == []
    # the oracle itself: RIPEMD-160's published vectors, and HASH160 of nothing
    assert native.ripemd160(b"abc").hex() == "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"
    assert native.ripemd160(b"").hex() == "9c1185a5c5e9fc54612808977ee8f548b2258d31"
    assert native.hash160_gpu([b""])[0].hex() == "b472a266d0bd89c13706a4132ccfb16f7c3b9fcb"


def mixed_items(native, rng, keys, txids, spent, watch, pubkeys):
    """Every item kind, members and strangers alike."""
    TXID, INPUT, OUTPUT = native.WM_ITEM_TXID, native.WM_ITEM_INPUT, native.WM_ITEM_OUTPUT
    items = [(TXID, x) for x in txids] + [(TXID, rng.randbytes(32)) for _ in range(20)]
    items += [(INPUT, x) for x in spent] + [(INPUT, x + struct.pack("<I", 1)) for x in txids]
    items += [(INPUT, rng.randbytes(36)) for _ in range(20)]
    items += [(OUTPUT, p2pkh(k)) for k in keys] + [(OUTPUT, p2sh(k)) for k in keys[:5]]
    items += [(OUTPUT, p2pk(p)) for p in pubkeys] + [(OUTPUT, s) for s in watch]
    items += [(OUTPUT, p2pkh(rng.randbytes(20))) for _ in range(20)]
    rng.shuffle(items)
    return items


@pytest.mark.parametrize("entries", [0, 1, 2, 1000, 200000])
def test_match_equals_twin_at_table_sizes(native, entries):
    """200,000 entries make 524,288 slots, 4 MiB: far past WM_LDS_MAX_BYTES (64 KiB), the largest
    table wallet_match_kernel stages to LDS; 1,000 entries (2,048 slots, 16 KiB) are staged."""
    rng = random.Random(entries)
    n = entries // 4
    pubkeys = [b"\x02" + rng.randbytes(32) for _ in range(max(1, min(n, 40)))] if entries > 2 else []
    keys = [rng.randbytes(20) for _ in range(max(0, entries - 2 * n - len(pubkeys) - (1 if entries > 2 else 0)))]
    txids = [rng.randbytes(32) for _ in range(n)]
    spent = [rng.randbytes(36) for _ in range(n)]
    watch = [b"\x51\x75\x51"] if entries > 2 else []
    if entries == 1:
        keys = [rng.randbytes(20)]
    if entries == 2:
        keys, txids = [rng.randbytes(20)], [rng.randbytes(32)]
    desc = dict(salt=SALT, keys=keys + [native.hash160(p) for p in pubkeys], txids=txids, spent=spent, watch=watch)
    t = native.wallet_match_table(desc)
    assert t["entries"] == entries
    assert (t["n_slots"] * 8 > native.WM_LDS_MAX_BYTES) == (entries == 200000)
    items = mixed_items(native, rng, keys[:200], txids[:200], spent[:200], watch, pubkeys)
    want = native.wallet_match_cpu(desc, items)
    if entries > 2:
        hit = {native.WM_HIT_K, native.WM_HIT_W, native.WM_HIT_T, native.WM_HIT_S, native.WM_HIT_T | native.WM_HIT_S}
        assert 0 in want and hit - {native.WM_HIT_T | native.WM_HIT_S} <= set(want)
    assert native.wallet_match_gpu(desc, items) == want


def keys_homed_at(native, rng, n_slots, homes):
    """20-byte keys whose home slots are `homes`, in that order."""
    out = []
    for home in homes:
        while True:
            k = rng.randbytes(20)
            if (native.wallet_fingerprint(SALT, k) >> 32) & (n_slots - 1) == home:
                out.append(k)
                break
    return out


def test_probe_chain_wraps_the_table_end(native):
    rng = random.Random(3)
    # 12 entries make 32 slots; six keys homed at slot 29 occupy 29, 30, 31, 0, 1, 2
    keys = keys_homed_at(native, rng, 32, [29] * 6) + [rng.randbytes(20) for _ in range(6)]
    desc = dict(salt=SALT, keys=keys)
    t = native.wallet_match_table(desc)
    assert t["n_slots"] == 32
    slots = struct.unpack("<32Q", t["slots"])
    assert all(slots[s] for s in (29, 30, 31, 0, 1, 2))
    strangers = keys_homed_at(native, rng, 32, [29, 30, 31, 0])
    items = [(native.WM_ITEM_OUTPUT, p2pkh(k)) for k in keys + strangers]
    want = native.wallet_match_cpu(desc, items)
    assert want == [native.WM_HIT_K] * 12 + [0] * 4
    assert native.wallet_match_gpu(desc, items) == want


def test_probe_chain_of_maximum_length(native):
    """WM_MAX_PROBE entries homed at one slot: the last sits at the end of the longest chain a
    lookup walks. One more would make the builder grow the table instead."""
    rng = random.Random(4)
    n = native.WM_MAX_PROBE
    keys = keys_homed_at(native, rng, 2 * n, [5] * n)
    desc = dict(salt=SALT, keys=keys)
    t = native.wallet_match_table(desc)
    assert t["n_slots"] == 2 * n and t["entries"] == n
    slots = struct.unpack(f"<{2 * n}Q", t["slots"])
    assert all(slots[5 + i] for i in range(n))
    strangers = keys_homed_at(native, rng, 2 * n, [5, 6, 5 + n - 1])
    items = [(native.WM_ITEM_OUTPUT, p2pkh(k)) for k in keys + strangers]
    want = native.wallet_match_cpu(desc, items)
    assert want == [native.WM_HIT_K] * n + [0] * 3
    assert native.wallet_match_gpu(desc, items) == want
    grown = native.wallet_match_table(dict(salt=SALT, keys=keys + keys_homed_at(native, rng, 2 * n, [5])))
    assert grown["n_slots"] > 2 * n


def test_scripts_of_every_size_and_push_form(native):
    rng = random.Random(5)
    pub, pub65 = b"\x03" + rng.randbytes(32), b"\x04" + rng.randbytes(64)
    h, h65, sid = native.hash160(pub), native.hash160(pub65), rng.randbytes(20)
    watch520, watch10k = rng.randbytes(520), b"\x6a" + rng.randbytes(9999)
    desc = dict(salt=SALT, keys=[h, h65, sid, rng.randbytes(20)], watch=[b"", b"\x51", watch520, watch10k])
    OUT = native.WM_ITEM_OUTPUT
    K, W = native.WM_HIT_K, native.WM_HIT_W
    scripts = [(b"", W), (b"\x51", W), (b"\x52", 0), (p2pkh(h), K), (p2pkh(rng.randbytes(20)), 0),  # 0, 1, 25 bytes
               (p2pk(pub65), K), (p2pk(b"\x04" + rng.randbytes(64)), 0),  # 67 bytes
               (watch520, W), (rng.randbytes(520), None), (watch10k, W), (b"\x6a" + rng.randbytes(9999), None),
               (b"\x00" * 9979 + push(h), K),  # a hit at the very end of 10,000 bytes
               (bytes(10001), native.WM_NOT_READ)]
    for form in (0, 1, 2, 4):
        scripts += [(p2pkh(h, form), K), (p2pk(pub, form), K), (p2pk(pub65, form), K), (p2sh(sid, form), K),
                    (multisig_1of2(b"\x02" + rng.randbytes(32), pub, form), K), (p2pkh(rng.randbytes(20), form), 0)]
    # GetOp failures: nothing after them is probed, what came before is
    scripts += [(b"\x14" + h[:19], 0), (b"\x4c", 0), (b"\x4c\x14" + h[:19], 0), (b"\x4d\x14", 0), (b"\x4d\x14\x00" + h[:19], 0),
                (b"\x4e\x14\x00\x00", 0), (b"\x4e\xff\xff\xff\xff" + h, 0), (b"\x4c\x15" + h, 0), (push(h) + b"\x4c", K),
                (b"\x4d\x01" + push(h), 0)]
    # CPubKey's view of a key: an ill-formed one hashes as no bytes, whose id is in no table here
    scripts += [(p2pk(b"\x05" + pub[1:]), 0), (p2pk(b"\x02" + rng.randbytes(33)), 0), (p2pk(b"\x04" + rng.randbytes(40)), 0)]
    items = [(OUT, s) for s, _ in scripts]
    want = native.wallet_match_cpu(desc, items)
    for (s, flag), got in zip(scripts, want):
        if flag is not None:  # None: a random script, whatever its pushes happen to be
            assert got == flag, (s[:40].hex(), len(s))
    assert native.wallet_match_gpu(desc, items) == want
    # a table that holds the id of the empty key flags every ill-formed key, as HaveKey would
    empty_id = dict(salt=SALT, keys=[native.hash160(b"")])
    bad = [(OUT, p2pk(b"\x05" + pub[1:])), (OUT, p2pk(pub))]
    assert native.wallet_match_cpu(empty_id, bad) == [K, 0]
    assert native.wallet_match_gpu(empty_id, bad) == [K, 0]


def test_host_form_rejects_bad_arguments(native):
    desc = dict(salt=SALT, keys=[bytes(20)])
    with pytest.raises(ValueError):
        native.wallet_match_gpu(desc, [(3, b"abc")])
    with pytest.raises(ValueError):
        native.wallet_match_gpu(dict(keys=[bytes(19)]), [])
    assert native.wallet_match_gpu(desc, []) == []
    # lengths a kind cannot have are not read
    assert native.wallet_match_gpu(desc, [(native.WM_ITEM_TXID, bytes(31)), (native.WM_ITEM_INPUT, bytes(37))]) == [2, 2]


def test_tensor_path_equals_host_path(native):
    import torch
    from bitcoincashplus_amd import ops
    rng = random.Random(77)
    keys = [rng.randbytes(20) for _ in range(300)]
    txids = [rng.randbytes(32) for _ in range(300)]
    spent = [rng.randbytes(36) for _ in range(300)]
    pubkeys = [b"\x02" + rng.randbytes(32) for _ in range(20)]
    watch = [b"\x51\x75\x51"]
    desc = dict(salt=SALT, keys=keys[:150] + [native.hash160(p) for p in pubkeys[:10]], txids=txids[:150],
                spent=spent[:150], watch=watch)
    items = mixed_items(native, rng, keys, txids, spent, watch, pubkeys)
    host = ops.wallet_match(desc, items)
    assert host == native.wallet_match_cpu(desc, items)
    offs, at = [], 0
    for _, b in items:
        offs.append(at)
        at += len(b)
    whole = torch.frombuffer(bytearray(b"\0" + b"".join(b for _, b in items)), dtype=torch.uint8).cuda()
    blob = whole[1:]  # the items start at an odd device address
    assert blob.data_ptr() % 2 == 1
    kinds_t = torch.frombuffer(bytearray(b"\0" + bytes(k for k, _ in items)), dtype=torch.uint8).cuda()[1:]
    offs_t = torch.tensor(offs, dtype=torch.int32, device="cuda")
    lens_t = torch.tensor([len(b) for _, b in items], dtype=torch.int32, device="cuda")
    got = ops.wallet_match(desc, (kinds_t, blob, offs_t, lens_t))
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (len(items),)
    assert got.cpu().tolist() == host
    # items the kernel must not read: past the end, offset past the end, an unknown kind; and a
    # good one after them
    bad_kinds = torch.tensor([2, 2, 0, 7, 2], dtype=torch.uint8, device="cuda")
    bad_offs = torch.tensor([at - 2, at + 5, at - 31, 0, 0], dtype=torch.int32, device="cuda")
    bad_lens = torch.tensor([3, 1, 32, 4, 0], dtype=torch.int32, device="cuda")
    got = ops.wallet_match(desc, (bad_kinds, blob, bad_offs, bad_lens)).cpu().tolist()
    assert got == [2, 2, 2, 2, 0]
    assert got == native.wallet_match_cpu_packed(desc, bytes([2, 2, 0, 7, 2]), b"".join(b for _, b in items),
                                                 [at - 2, at + 5, at - 31, 0, 0], [3, 1, 32, 4, 0])
    # hash160 on tensors at an odd address, with messages it must not read
    msgs = [rng.randbytes(n) for n in (0, 33, 65, 520, 7)]
    mo, mat = [], 0
    for m in msgs:
        mo.append(mat)
        mat += len(m)
    mblob = torch.frombuffer(bytearray(b"\0" + b"".join(msgs)), dtype=torch.uint8).cuda()[1:]
    mo_t = torch.tensor(mo + [mat - 1, 0], dtype=torch.int32, device="cuda")
    ml_t = torch.tensor([len(m) for m in msgs] + [2, 521], dtype=torch.int32, device="cuda")
    digests, status = ops.hash160((mblob, mo_t, ml_t))
    assert status.cpu().tolist() == [1] * 5 + [2, 2]
    assert [bytes(d) for d in digests.cpu().tolist()] == ops.hash160(msgs) + [bytes(20)] * 2
    assert ops.hash160(msgs) == [native.hash160(m) for m in msgs]


@pytest.mark.parametrize("name", sorted(wallet_scan_cases.cases()))
def test_scan_on_device_equals_reference_loop(native, name):
    case = wallet_scan_cases.cases()[name]
    native.wallet_scan_reset_failures()
    before = native.wallet_scan_stats()
    info, verdicts = check_scan(case, True)
    after = native.wallet_scan_stats()
    assert after["gpu_failures"] == before["gpu_failures"]
    print(name, info, "cap", rerun_cap(case, verdicts))
    if name == "empty_list":
        assert info["passes"] == 0 and not info["used_gpu"]  # nothing to match: no device call
        return
    assert info["used_gpu"] and after["wallet_scans"] == before["wallet_scans"] + 1
    assert info["cpu_reruns"] <= rerun_cap(case, verdicts)
    if name == "chain_abc":
        assert info["passes"] >= 2  # a single pass would miss B and C
    if name == "reversed_ba":
        assert verdicts == [False, True]


def test_superset_on_random_block(native):
    """Every transaction the reference loop adds is flagged by the device against the table of the
    wallet as it ends up: the members it gained are in T and S."""
    case = wallet_scan_cases.cases()["random_block"]
    want, wtxs, spent = native.wallet_scan_reference(case["txs"], case["wallet"], True)
    assert sum(want) >= 30
    desc = dict(keys=[native.hash160(p) for p in case["wallet"]["pubkeys"]] +
                [native.hash160(s) for s in case["wallet"]["scripts"]],
                watch=case["wallet"]["watch"], txids=[w[:32] for w in wtxs], spent=[s[:36] for s in spent], salt=SALT)
    from bitcoincashplus_amd.testing.messages import CTransaction
    import io
    items, owner = [], []
    for i, raw in enumerate(case["txs"]):
        t = CTransaction()
        t.deserialize(io.BytesIO(raw))
        mine = [(native.WM_ITEM_INPUT, v.prevout.hash.to_bytes(32, "little") + struct.pack("<I", v.prevout.n)) for v in t.vin]
        mine += [(native.WM_ITEM_OUTPUT, o.scriptPubKey) for o in t.vout]
        items += mine
        owner += [i] * len(mine)
    flags = native.wallet_match_gpu(desc, items)
    assert flags == native.wallet_match_cpu(desc, items)
    flagged = {o for o, f in zip(owner, flags) if f}
    assert {i for i, v in enumerate(want) if v} <= flagged


def test_ops_wallet_scan(native):
    from bitcoincashplus_amd import ops
    case = wallet_scan_cases.cases()["chain_abc"]
    verdicts, wtxs, spent, info = ops.wallet_scan(case["txs"], case["wallet"])
    assert list(verdicts) == case["verdicts"] and info["used_gpu"]
    assert (list(verdicts), list(wtxs), list(spent)) == tuple(map(list, native.wallet_scan_reference(case["txs"], case["wallet"])))
