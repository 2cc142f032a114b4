"""The node's batched CheckBlockHeader (CheckBlockHeaders, csrc/consensus/pow.cpp) without a GPU.

1. The batch function on the CPU (`allow_gpu=False`, and the GPU path failing over with
   `set_gpu_fault_injection`) against the per-header consensus functions: CheckEquihashSolution,
   GetHash and CheckProofOfWork.
2. A node whose headers messages take the batch path (AcceptBlockHeader is handed the hash and the
   proof-of-work verdict) against a node on the per-header path: the same index entries, and the
   same reject reason and misbehaviour score for a message that holds a `high-hash` header.
"""
import glob
import os
import re
import time

import pytest

from bitcoincashplus_amd.testing.blocktools import create_block, create_coinbase, solve
from bitcoincashplus_amd.testing.messages import REGTEST_BCP_HEIGHT, CBlockHeader, msg_headers, uint256_from_compact

FORK_MARGIN = 6


def solve_high_hash(block, max_tries=1 << 16):
    """A valid Equihash(48,5) solution whose block hash is above the target of nBits."""
    from bitcoincashplus_amd import native
    target = uint256_from_compact(block.nBits)
    inp = block.equihash_input()
    for _ in range(max_tries):
        st = native.EquihashState(48, 5)
        st.update(inp + block.nNonce.to_bytes(32, "little"))
        for sol in native.eh_solve_cpu(48, 5, st)[0]:
            block.nSolution = bytes(sol)
            if block.rehash() > target:
                return block
        block.nNonce += 1
    raise RuntimeError("no high-hash solution found")


def build_headers(prev, height, ntime, count, high_at=None):
    """`count` post-fork regtest headers on top of (prev, height); header `high_at` has a valid
    solution and a hash above its target, and the ones after it build on it."""
    out = []
    for i in range(count):
        height += 1
        ntime += 1
        blk = create_block(prev, create_coinbase(height), ntime, height)
        if i == high_at:
            solve_high_hash(blk)
        else:
            solve(blk)
        out.append(CBlockHeader(blk))
        prev = blk.sha256
    return out


# ------------------------------------------------------------------ 1. the batch function
def test_batch_function_matches_per_header(native):
    headers = build_headers(0x1234, REGTEST_BCP_HEIGHT + 10, 1_600_000_000, 6, high_at=2)
    raw = [h.serialize() for h in headers]
    bad = bytearray(raw[4])
    bad[-1] ^= 0x01  # last solution byte
    raw[4] = bytes(bad)
    raw.append(raw[0][:140] + bytes([35]) + raw[0][141:176])  # a solution one byte short
    want = []
    for r in raw:
        hx = native.header_hash(r, False, "regtest")
        bits = int.from_bytes(r[104:108], "little")
        want.append((native.check_equihash_header(r, "regtest"), native.check_proof_of_work(hx, bits, True, "regtest"),
                     bytes.fromhex(hx)[::-1]))
    assert [w[0] for w in want] == [True, True, True, True, False, True, False]
    assert [w[1] for w in want][:4] == [True, True, False, True]  # header 2: valid solution, high hash
    got = native.check_block_headers(raw, "regtest", False)
    assert [g[:3] for g in got] == want
    assert not any(g[3] for g in got)  # nothing came from a device
    # the GPU path throwing: the same batch redone on the CPU
    native.set_gpu_fault_injection(True)
    try:
        again = native.check_block_headers(raw, "regtest", True)
    finally:
        native.set_gpu_fault_injection(False)
    assert again == got
    assert native.check_block_headers([], "regtest", False) == []


# ------------------------------------------------------------------ 2. nodes
def wait_until(pred, timeout=120, step=0.05, what="condition"):
    deadline = time.time() + timeout
    while time.time() < deadline:
        if pred():
            return
        time.sleep(step)
    raise AssertionError(f"timed out waiting for {what}")


def log_lines(node):
    for path in glob.glob(os.path.join(node.datadir, "**", "debug.log"), recursive=True):
        with open(path, errors="replace") as f:
            yield from f


def misbehaviour(node):
    """[(score added, reason)] of every Misbehaving line of the node's log."""
    out = []
    for line in log_lines(node):
        m = re.search(r"Misbehaving.*\((\d+) -> (\d+)\) reason: (\S+)", line)
        if m:
            out.append((int(m.group(2)) - int(m.group(1)), m.group(3)))
    return out


def header_scenario(tmpdir, others):
    """Node A (`-gpu=0`, the per-header path) mines through the fork; every node of `others`
    ({name: extra args}) syncs A's chain over P2P. Then each node gets the same HEADERS message
    of six headers whose fourth has a valid solution and a hash above its target. Returns
    {name: (ban scores, misbehaviour, chain tips, getgpuinfo after the sync, header batches that
    failed over to the CPU)} with A under "a"."""
    import subprocess
    from bitcoincashplus_amd.node.embedded import RPCError
    from bitcoincashplus_amd.node.process import BIN_DIR, BcpdProcess
    from bitcoincashplus_amd.testing.p2p import P2PPeer
    if not os.path.exists(os.path.join(BIN_DIR, "bcpd")):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN_DIR), "-j8", "tools"])
    common = ["-whitelist=127.0.0.1"]
    nodes = {"a": BcpdProcess(os.path.join(tmpdir, "a"), extra_args=["-gpu=0", *common])}
    for name, args in others.items():
        nodes[name] = BcpdProcess(os.path.join(tmpdir, name), extra_args=[*args, *common])
    peers, started = [], []
    try:
        for n in nodes.values():
            n.start()
            started.append(n)
        a = nodes["a"]
        a.rpc.generate(REGTEST_BCP_HEIGHT - 1)
        a.rpc.generate(FORK_MARGIN)
        tip = a.rpc.getbestblockhash()
        for name, n in nodes.items():
            if name != "a":
                n.rpc.addnode(f"127.0.0.1:{a.p2p_port}", "onetry")
        for name, n in nodes.items():
            wait_until(lambda: n.rpc.getbestblockhash() == tip, 300, what=f"node {name} syncing A's chain")
        info_synced = {name: n.rpc.getgpuinfo() for name, n in nodes.items()}
        hdr = a.rpc.getblockheader(tip)
        assert hdr["height"] == REGTEST_BCP_HEIGHT - 1 + FORK_MARGIN
        headers = build_headers(int(tip, 16), hdr["height"], hdr["time"], 6, high_at=3)
        last_good = f"{headers[2].sha256:064x}"
        out = {}
        for name, n in nodes.items():
            for p in n.rpc.getpeerinfo():  # keep the nodes' own link out of the exchange
                try:
                    n.rpc.disconnectnode(p["addr"])
                except RPCError as e:  # the other end of the link dropped it first: it is gone, as wanted
                    if e.code != -29:
                        raise
        for name, n in nodes.items():
            wait_until(lambda: not n.rpc.getpeerinfo(), 60, what=f"node {name} dropping its peers")
            peer = P2PPeer().connect("127.0.0.1", n.p2p_port)
            peers.append(peer)
            peer.send(msg_headers(headers))
            peer.sync_with_ping(timeout=120)
            scores = [p["banscore"] for p in n.rpc.getpeerinfo()]
            tips = sorted((t["hash"], t["height"], t["status"]) for t in n.rpc.getchaintips())
            assert (last_good, hdr["height"] + 3, "headers-only") in tips, tips
            assert n.rpc.getbestblockhash() == tip
            failed_over = sum("GPU header check failed" in line for line in log_lines(n))
            out[name] = (scores, misbehaviour(n), tips, info_synced[name], failed_over)
        return out
    finally:
        for p in peers:
            try:
                p.close()
            except Exception:
                pass
        for n in started:
            n.stop()


@pytest.mark.functional
def test_node_batch_path_matches_per_header_path(tmp_path):
    # B: the GPU way with every device batch failing, so the batch function's CPU results reach
    # AcceptBlockHeader as supplied hash and proof-of-work verdict
    res = header_scenario(str(tmp_path), {"b": ["-gpufaultinjection"]})
    (sa, ma, ta, _, fa), (sb, mb, tb, gib, fb) = res["a"], res["b"]
    # the sync's post-fork headers and the message above went through the batch function on B
    assert fa == 0 and fb >= 2, (fa, fb)
    assert ma == [(50, "high-hash")], ma
    assert mb == ma and sb == sa == [50]
    assert ta == tb
    assert sum(L["header_hashes"] for L in gib["validation_lanes"]) == 0
