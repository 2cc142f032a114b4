"""Payments of a wallet that searches its coin subsets on the GPU (pattern:
tests/test_functional_gpu_wallet_scan.py).

Node A runs `-gpu=1 -gpucoinselectthreshold=1`: every subset search of SelectCoinsMinConf goes
through the batched search (wallet/coinselect.cpp) with its trials on the device. It mines past
maturity, fans a few hundred small outputs to itself with `sendmany`, and then pays node B with
`sendtoaddress` and with `fundrawtransaction`. The payments must be accepted and mined, their
inputs must cover amount plus fee, A's counters must show the searches ran on the device without
a fallback, and B (`-gpu=0`) must accept the same blocks and see the money.
"""
import os
import time
from decimal import Decimal

import pytest

from bitcoincashplus_amd.node.process import BIN_DIR, BcpdProcess

pytestmark = [pytest.mark.gpu, pytest.mark.functional]

FAN = 300


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


def inputs_and_outputs(rpc, txid):
    tx = rpc.getrawtransaction(txid, True)
    ins = [Decimal(str(rpc.getrawtransaction(i["txid"], True)["vout"][i["vout"]]["value"])) for i in tx["vin"]]
    outs = [Decimal(str(o["value"])) for o in tx["vout"]]
    return ins, outs


def run_scenario(tmpdir, log=print):
    _ensure_binaries()
    common = ["-whitelist=127.0.0.1", "-txindex=1"]
    a = BcpdProcess(os.path.join(tmpdir, "a"), extra_args=["-gpu=1", "-gpucoinselectthreshold=1", *common])
    b = BcpdProcess(os.path.join(tmpdir, "b"), extra_args=["-gpu=0", *common])
    nodes = (a, b)
    for n in nodes:
        n.start()
    try:
        ra, rb = a.rpc, b.rpc
        g0 = ra.getgpuinfo()["coinselect"]
        assert g0["threshold"] == 1 and g0["gpu_selections"] == 0
        assert rb.getgpuinfo()["coinselect"]["threshold"] >= 2048 or rb.getgpuinfo()["coinselect"]["threshold"] == 0
        ra.generate(110)
        rb.addnode(f"127.0.0.1:{a.p2p_port}", "add")
        # a few hundred small coins, no two alike
        fan = {ra.getnewaddress(): Decimal("0.01") + Decimal(i) / 100000 for i in range(FAN)}
        fan_txid = ra.sendmany("", fan)
        ra.generate(1)
        assert ra.gettransaction(fan_txid)["confirmations"] == 1
        g1 = ra.getgpuinfo()["coinselect"]
        log(f"A after the fan-out: {g1}")

        # more than any small coin and less than their sum: the subset search decides
        pay1, pay2 = Decimal("1.2345"), Decimal("0.777")
        addr1, addr2 = rb.getnewaddress(), rb.getnewaddress()
        txid1 = ra.sendtoaddress(addr1, pay1)
        g2 = ra.getgpuinfo()["coinselect"]
        assert g2["gpu_selections"] > g1["gpu_selections"] and g2["gpu_failures"] == 0 and g2["cpu_selections"] == 0
        funded = ra.fundrawtransaction(ra.createrawtransaction([], {addr2: pay2}))
        signed = ra.signrawtransaction(funded["hex"])
        assert signed["complete"], signed
        txid2 = ra.sendrawtransaction(signed["hex"])
        g3 = ra.getgpuinfo()["coinselect"]
        log(f"A after the payments: {g3}")
        assert g3["gpu_selections"] > g2["gpu_selections"] and g3["gpu_failures"] == 0 and g3["cpu_selections"] == 0
        assert set(ra.getrawmempool()) >= {txid1, txid2}
        ra.generate(1)
        for txid, amount, fee in ((txid1, pay1, -Decimal(str(ra.gettransaction(txid1)["fee"]))),
                                  (txid2, pay2, Decimal(str(funded["fee"])))):
            assert ra.gettransaction(txid)["confirmations"] == 1
            ins, outs = inputs_and_outputs(ra, txid)
            assert fee > 0 and sum(ins) == sum(outs) + fee
            assert sum(ins) >= amount + fee and amount in outs
            # many small coins, not one coinbase: the subset won
            assert len(ins) > 1 and max(ins) < 1
        wait_until(lambda: rb.getbestblockhash() == ra.getbestblockhash(), 120, what="B syncing A's chain")
        assert Decimal(str(rb.getreceivedbyaddress(addr1))) == pay1
        assert Decimal(str(rb.getreceivedbyaddress(addr2))) == pay2
        gb = rb.getgpuinfo()["coinselect"]
        assert gb["gpu_selections"] == 0 and gb["cpu_selections"] == 0 and gb["gpu_failures"] == 0
        return g3
    finally:
        for n in nodes:
            n.stop()


def test_gpu_coin_selection_node_pays_and_cpu_node_accepts(tmp_path):
    run_scenario(str(tmp_path))
