"""The batched wallet scan (csrc/wallet/walletscan.cpp) with its match passes on the CPU
(``use_gpu=False``: the host twin of wallet_match_kernel) against the loop of
CWallet::AddToWalletIfInvolvingMe, on the cases of tests/wallet_scan_cases.py; and the match table
and twin themselves."""
import random
import struct

import pytest

import wallet_scan_cases
from wallet_scan_cases import check_scan, rerun_cap


@pytest.mark.parametrize("name", sorted(wallet_scan_cases.cases()))
def test_scan_equals_reference_loop(native, name):
    case = wallet_scan_cases.cases()[name]
    before = native.wallet_scan_stats()
    info, verdicts = check_scan(case, False)
    after = native.wallet_scan_stats()
    assert not info["used_gpu"] and after["gpu_failures"] == before["gpu_failures"]
    assert after["wallet_scans"] == before["wallet_scans"] and after["cpu_scans"] == before["cpu_scans"] + 1
    print(name, info, "cap", rerun_cap(case, verdicts))
    assert info["cpu_reruns"] <= rerun_cap(case, verdicts)
    if name == "chain_abc":
        assert info["passes"] >= 2  # a single pass would miss B and C
    if name == "empty_list":
        assert info["passes"] == 0 and info["items"] == 0
    if name == "random_block":
        assert sum(verdicts) >= 30 and info["passes"] >= 16  # past the device passes: the host's exact sets


def test_published_ripemd160_vectors(native):
    """The CPU oracle of hash160_kernel, from the RIPEMD-160 paper's test vectors."""
    for msg, digest in ((b"", "9c1185a5c5e9fc54612808977ee8f548b2258d31"),
                        (b"a", "0bdc9d2d256b3ee9daae347be6f4dc835a467ffe"),
                        (b"abc", "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"),
                        (b"message digest", "5d0689ef49d2fae572b881b123a85ffa21595f36"),
                        (b"abcdefghijklmnopqrstuvwxyz", "f71c27109c692c1b56bbdceb5b9d2865b3708dbc")):
        assert native.ripemd160(msg).hex() == digest
    rng = random.Random(160)
    for _ in range(50):  # the one-block compression the device runs, compiled for the host
        d = rng.randbytes(32)
        assert native.wallet_match_ripemd160_32(d) == native.ripemd160(d)


def test_table_and_twin(native):
    rng = random.Random(9)
    keys = [rng.randbytes(20) for _ in range(300)]
    txids = [rng.randbytes(32) for _ in range(300)]
    spent = [rng.randbytes(36) for _ in range(300)]
    watch = [b"\x51" * 3, rng.randbytes(700)]
    desc = dict(salt=bytes(range(16)), keys=keys[:150], txids=txids[:150], spent=spent[:150], watch=watch[:1])
    t = native.wallet_match_table(desc)
    assert t["entries"] == 451 and t["n_slots"] == 1024 and t["has_watch"]
    K, W, T, S = native.WM_HIT_K, native.WM_HIT_W, native.WM_HIT_T, native.WM_HIT_S
    TXID, INPUT, OUTPUT = native.WM_ITEM_TXID, native.WM_ITEM_INPUT, native.WM_ITEM_OUTPUT
    items = [(TXID, x) for x in txids] + [(INPUT, x) for x in spent] + [(INPUT, x + struct.pack("<I", 7)) for x in txids]
    items += [(OUTPUT, wallet_scan_cases.p2pkh(k)) for k in keys] + [(OUTPUT, s) for s in watch]
    flags = native.wallet_match_cpu(desc, items)
    want = [T] * 150 + [0] * 150 + [S] * 150 + [0] * 150 + [T] * 150 + [0] * 150 + [K] * 150 + [0] * 150 + [W, 0]
    assert flags == want
    # the same members under another salt land elsewhere, and only coins are matched under their mask
    other = native.wallet_match_table(dict(desc, salt=bytes(16)))
    assert other["slots"] != t["slots"]
    coins = native.wallet_match_cpu(desc, items, 3)
    assert coins == want[:900] + [0] * 302
    # kinds and lengths the twin does not read
    assert native.wallet_match_cpu(desc, [(3, b"x"), (TXID, bytes(31)), (INPUT, bytes(35)), (OUTPUT, bytes(10001))]) == [2] * 4
    assert native.wallet_match_cpu(desc, [(OUTPUT, bytes(10000))]) == [0]
