"""Rescans and block connects of a wallet that matches whole blocks on the GPU against a CPU twin
(pattern: tests/test_functional_gpu_bloom.py).

Node A runs `-gpu=1 -gpuwalletscanthreshold=1`: every block of a rescan and every connected block
goes through the batched scan (wallet/walletscan.cpp) with its match passes on the device. Node B
runs `-gpu=0`: the per-transaction loop of CWallet::AddToWalletIfInvolvingMe. A third node, the
miner, owns the funds and makes the chain: payments to a key, to a P2SH script and to a bare
script, spends of some of them, and two in one block where the second spends the first.

A and B then import the same things, `importprivkey` (the key), `importaddress` (the P2SH redeem
script), `importmulti` (the bare script, watch-only), each with a rescan, and are restarted with
`-rescan`. What the two wallets then say must be equal, and A's counters must show the scans ran
on the device without a failure.
"""
import os
import time
from decimal import Decimal

import pytest

from bitcoincashplus_amd.node.process import BIN_DIR, BcpdProcess

pytestmark = [pytest.mark.gpu, pytest.mark.functional]


def _ensure_binaries():
    if not os.path.exists(os.path.join(BIN_DIR, "bcpd")):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.dirname(BIN_DIR), "-j8", "tools"])


def wait_until(pred, timeout=120, step=0.05, what="condition"):
    deadline = time.time() + timeout
    while time.time() < deadline:
        if pred():
            return
        time.sleep(step)
    raise AssertionError(f"timed out waiting for {what}")


def without_clock(entries):
    """Wallet entries without the fields that hold the node's own clock."""
    return [{k: v for k, v in e.items() if k != "timereceived"} for e in entries]


def wallet_view(rpc, since):
    lsb = rpc.listsinceblock(since, 1, True)
    return dict(
        transactions=without_clock(rpc.listtransactions("*", 1000, 0, True)),
        unspent=sorted(((u["txid"], u["vout"], str(u["amount"]), u["confirmations"], u["spendable"]) for u in rpc.listunspent(0)),
                       key=lambda u: u[:2]),
        balance=str(rpc.getbalance()),
        balance_watch=str(rpc.getbalance("*", 0, True)),
        txcount=rpc.getwalletinfo()["txcount"],
        since=sorted(without_clock(lsb["transactions"]), key=lambda e: (e["txid"], e.get("vout", -1), e["category"])),
        lastblock=lsb["lastblock"],
    )


def output_of(m, txid, value):
    return next(o["n"] for o in m.getrawtransaction(txid, True)["vout"] if abs(float(o["value"]) - float(value)) < 1e-9)


def spend(m, txid, value, to, amount):
    """The miner spends exactly the output of `txid` worth `value`."""
    vout = output_of(m, txid, value)
    raw = m.createrawtransaction([{"txid": txid, "vout": vout}], {to: amount})
    signed = m.signrawtransaction(raw)
    assert signed["complete"], signed
    return m.sendrawtransaction(signed["hex"])


def run_scenario(tmpdir, log=print):
    _ensure_binaries()
    common = ["-whitelist=127.0.0.1"]
    miner = BcpdProcess(os.path.join(tmpdir, "m"), extra_args=["-gpu=0", *common])
    a = BcpdProcess(os.path.join(tmpdir, "a"), extra_args=["-gpu=1", "-gpuwalletscanthreshold=1", *common])
    b = BcpdProcess(os.path.join(tmpdir, "b"), extra_args=["-gpu=0", *common])
    nodes = (miner, a, b)
    for n in nodes:
        n.start()
    try:
        m = miner.rpc
        m.generate(110)
        for n in (a, b):
            n.rpc.addnode(f"127.0.0.1:{miner.p2p_port}", "add")
        key_addr = m.getnewaddress()
        priv = m.dumpprivkey(key_addr)
        ms = m.createmultisig(1, [m.validateaddress(m.getnewaddress())["pubkey"] for _ in range(2)])
        script_addr, redeem = ms["address"], ms["redeemScript"]
        bare_spk = m.validateaddress(m.getnewaddress())["scriptPubKey"]  # watched by its script alone
        bare_addr = m.decodescript(bare_spk)["addresses"][0]
        first_block = m.getbestblockhash()
        # three blocks: payments among unrelated ones, spends of earlier payments, and a payment spent
        # in the block that confirms it
        paid = []
        for k in range(3):
            for i in range(12):
                m.sendtoaddress(m.getnewaddress(), Decimal("0.01") + Decimal(i) / 100000)
            paid.append(m.sendtoaddress(key_addr, Decimal("1.5") + k))
            # kept out of the miner's coin selection: spent only where the scenario says so
            assert m.lockunspent(False, [{"txid": paid[-1], "vout": output_of(m, paid[-1], Decimal("1.5") + k)}])
            m.sendtoaddress(script_addr, Decimal("0.25") + k)
            m.sendtoaddress(bare_addr, Decimal("0.125") + k)
            if k == 1:
                spend(m, paid[0], Decimal("1.5"), m.getnewaddress(), Decimal("1.499"))
            if k == 2:
                spend(m, paid[2], Decimal("3.5"), key_addr, Decimal("3.499"))  # A then B inside one block
            m.generate(1)
        for n in (a, b):
            wait_until(lambda: n.rpc.getbestblockhash() == m.getbestblockhash(), 120, what="syncing the miner's chain")

        ga0 = a.rpc.getgpuinfo()["walletscan"]
        assert ga0["threshold"] == 1
        for n in (a, b):
            r = n.rpc
            r.importprivkey(priv, "key", True)
            r.importaddress(redeem, "script", True, True)
            res = r.importmulti([{"scriptPubKey": bare_spk, "timestamp": 0, "watchonly": True, "internal": True}], {"rescan": True})
            assert res[0]["success"], res
        va, vb = wallet_view(a.rpc, first_block), wallet_view(b.rpc, first_block)
        assert va == vb
        assert va["txcount"] >= 3 * 3 + 2 and va["unspent"]
        ga1 = a.rpc.getgpuinfo()["walletscan"]
        log(f"A after the imports: {ga1}")
        assert ga1["wallet_scans"] > ga0["wallet_scans"] and ga1["gpu_failures"] == 0 and ga1["items"] > 0
        assert ga1["passes"] > ga1["wallet_scans"] - ga0["wallet_scans"]  # the in-block spend took a second pass

        # the same from scratch: -rescan at startup
        for n in (a, b):
            n.stop()
            n.extra_args = n.extra_args + ["-rescan"]
            n.start()
        va2, vb2 = wallet_view(a.rpc, first_block), wallet_view(b.rpc, first_block)
        assert va2 == vb2
        assert va2["txcount"] == va["txcount"] and va2["balance"] == va["balance"]
        ga2 = a.rpc.getgpuinfo()["walletscan"]
        log(f"A after -rescan: {ga2}")
        assert ga2["wallet_scans"] >= 110 and ga2["gpu_failures"] == 0  # a silent fallback would count cpu_scans instead

        # a block mined to A's own wallet: BlockConnected on the device path
        before = a.rpc.getgpuinfo()["walletscan"]["wallet_scans"]
        count = a.rpc.getwalletinfo()["txcount"]
        a.rpc.generate(1)
        ga3 = a.rpc.getgpuinfo()["walletscan"]
        assert ga3["wallet_scans"] > before and ga3["gpu_failures"] == 0
        assert a.rpc.getwalletinfo()["txcount"] == count + 1  # the coinbase
        gb = b.rpc.getgpuinfo()["walletscan"]
        assert gb["wallet_scans"] == 0 and gb["cpu_scans"] == 0  # the twin never left the loop
        return ga3
    finally:
        for n in nodes:
            n.stop()


def test_gpu_wallet_scan_node_matches_cpu_node(tmp_path):
    run_scenario(str(tmp_path))
