"""Filtered blocks and the mempool reply from a node that matches peers' BIP37 filters on the GPU
against a CPU twin (pattern: tests/test_functional_gpu_node.py).

Node A runs `-gpu=1 -gpubloomthreshold=1`: every `getdata MSG_FILTERED_BLOCK` and every `mempool`
request under a filter goes through the batched scan (net/bloomscan.cpp) with its membership
passes on the device. Node B runs `-gpu=0`: the per-transaction loop of
CBloomFilter::IsRelevantAndUpdate (reference src/net_processing.cpp:1241-1270, :3600-3625).

Both share a regtest chain whose last four blocks hold about 50 wallet transactions each; one of
them pays a watched address and another, in the same block, spends that output (it matches only
through the outpoint the first one inserted under BLOOM_UPDATE_ALL). A test peer loads the same
filter into both nodes, asks for the four blocks in turn (the filter carries over from block to
block) and then for the mempool. The `merkleblock` payloads, the `tx` messages that follow them
and the `inv` sets must be identical, and A's counters must show the scans ran on the device.
"""
import os
import time
from decimal import Decimal

import pytest

from bitcoincashplus_amd.node.process import BIN_DIR, BcpdProcess
from bitcoincashplus_amd.testing.messages import MSG_FILTERED_BLOCK, MSG_TX, CBloomFilter, CInv, msg_filterload, msg_getdata, msg_mempool
from bitcoincashplus_amd.testing.p2p import P2PPeer

pytestmark = [pytest.mark.gpu, pytest.mark.functional]

N_BLOCKS = 4
TX_PER_BLOCK = 50
N_MEMPOOL = 30


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


class RecordingPeer(P2PPeer):
    """Keeps the raw payload of every merkleblock, tx and inv message, in arrival order."""

    def __init__(self):
        super().__init__()
        self.raw = []

    def _dispatch(self, cmd, payload):
        if cmd in (b"merkleblock", b"tx", b"inv"):
            with self.cv:
                self.raw.append((cmd, payload))
        super()._dispatch(cmd, payload)


def key_hash(rpc, addr):
    spk = bytes.fromhex(rpc.validateaddress(addr)["scriptPubKey"])
    assert len(spk) == 25 and spk[:3] == b"\x76\xa9\x14"
    return spk[3:23]


def ask(node, flt, block_hashes, log):
    """One peer's session: filterload, the filtered blocks one by one, then the mempool."""
    peer = RecordingPeer().connect("127.0.0.1", node.p2p_port)
    try:
        peer.send(msg_filterload(flt))
        peer.sync_with_ping()
        blocks = []
        for h in block_hashes:
            start = len(peer.raw)
            peer.send(msg_getdata([CInv(MSG_FILTERED_BLOCK, int(h, 16))]))
            peer.sync_with_ping()
            got = [m for m in peer.raw[start:] if m[0] != b"inv"]
            assert got and got[0][0] == b"merkleblock" and all(c == b"tx" for c, _ in got[1:]), [c for c, _ in got]
            blocks.append(got)
        start = len(peer.raw)
        peer.send(msg_mempool())
        peer.wait_for(lambda: any(c == b"inv" for c, _ in peer.raw[start:]), 30, "the mempool reply")
        peer.sync_with_ping()
        invs = set()
        for m in peer.log:
            if m.command == b"inv":
                invs |= {i.hash for i in m.inv if i.type == MSG_TX}
        log(f"port {node.p2p_port}: {[len(b) - 1 for b in blocks]} matched transactions per block, {len(invs)} in the mempool reply")
        return blocks, invs
    finally:
        peer.close()


def run_scenario(tmpdir, expect_gpu=True, extra_a=(), log=print):
    _ensure_binaries()
    common = ["-whitelist=127.0.0.1", "-debug=net"]
    a = BcpdProcess(os.path.join(tmpdir, "a"), extra_args=["-gpu=1", "-gpubloomthreshold=1", *extra_a, *common])
    b = BcpdProcess(os.path.join(tmpdir, "b"), extra_args=["-gpu=0", *common])
    a.start()
    b.start()
    try:
        r = a.rpc
        r.generate(110)
        # B follows from here on, so that the wallet's transactions reach its pool as they are made
        b.rpc.addnode(f"127.0.0.1:{a.p2p_port}", "add")
        wait_until(lambda: a.rpc.getbestblockhash() == b.rpc.getbestblockhash(), 120, what="B syncing A's chain")
        # many confirmed coins, so that 50 sends a block do not chain through unconfirmed change
        for _ in range(3):
            r.sendmany("", {r.getnewaddress(): Decimal("2") for _ in range(40)})
        r.generate(1)
        watched = [r.getnewaddress() for _ in range(N_BLOCKS + 2)]
        flt = CBloomFilter(50, 0.0001, 0x1234ABCD, 1)  # BLOOM_UPDATE_ALL
        for w in watched:
            flt.insert(key_hash(r, w))
        block_hashes = []
        for k in range(N_BLOCKS + 1):  # the last round stays in the mempool
            last = k == N_BLOCKS
            for i in range(N_MEMPOOL if last else TX_PER_BLOCK - 2):
                r.sendtoaddress(watched[k] if i % 17 == 5 else r.getnewaddress(), Decimal("0.01") + Decimal(i) / 100000)
            # A pays a watched address; B spends exactly that output to an unwatched one
            txid = r.sendtoaddress(watched[k], Decimal("0.5"))
            vout = next(o["n"] for o in r.getrawtransaction(txid, True)["vout"] if abs(float(o["value"]) - 0.5) < 1e-9)
            raw = r.createrawtransaction([{"txid": txid, "vout": vout}], {r.getnewaddress(): Decimal("0.499")})
            signed = r.signrawtransaction(raw)
            assert signed["complete"], signed
            r.sendrawtransaction(signed["hex"])
            if not last:
                block_hashes += r.generate(1)
                assert len(r.getblock(block_hashes[-1])["tx"]) == TX_PER_BLOCK + 1
        wait_until(lambda: a.rpc.getbestblockhash() == b.rpc.getbestblockhash(), 120, what="B following A's chain")
        wait_until(lambda: sorted(a.rpc.getrawmempool()) == sorted(b.rpc.getrawmempool()), 120, what="B's mempool")
        assert len(a.rpc.getrawmempool()) == N_MEMPOOL + 2

        gi0 = a.rpc.getgpuinfo()["bloom"]
        assert gi0["threshold"] == 1 and b.rpc.getgpuinfo()["bloom"]["threshold"] == 0
        blocks_a, invs_a = ask(a, flt, block_hashes, log)
        blocks_b, invs_b = ask(b, flt, block_hashes, log)
        assert blocks_a == blocks_b  # merkleblock payloads and the tx messages after them, byte for byte
        assert invs_a == invs_b and invs_a
        # the pair of each block matched: at least A, B and the sends to the watched address
        assert all(len(blk) - 1 >= 4 for blk in blocks_a), [len(blk) for blk in blocks_a]
        gi1 = a.rpc.getgpuinfo()["bloom"]
        log(f"A bloom counters: {gi1}")
        if expect_gpu:
            assert gi1["gpu_scans"] - gi0["gpu_scans"] >= N_BLOCKS + 1, (gi0, gi1)
            assert gi1["gpu_failures"] == 0 and gi1["gpu_elements"] > 0 and gi1["rounds"] >= gi1["gpu_scans"]
        gb = b.rpc.getgpuinfo()["bloom"]
        assert gb["gpu_scans"] == 0 and gb["cpu_scans"] == 0  # the twin never left the loop
        return gi1
    finally:
        a.stop()
        b.stop()


def test_gpu_bloom_node_matches_cpu_node(tmp_path):
    run_scenario(str(tmp_path), expect_gpu=True)
