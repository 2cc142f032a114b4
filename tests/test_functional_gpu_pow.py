"""The built-in miner's device-side target filter in a running node.

Node A (`-gpu=1`) mines across the regtest fork: every post-fork block goes through
SolveEquihash -> EquihashSearchGpu(target) -> LaunchPow / CollectPow, so the device builds the
nonce states, solves, encodes each solution, hashes the header and compares it with the target,
and the node re-checks only the chosen hit on the CPU. Node B (`-gpu=0`) validates A's chain on
the CPU consensus path. `equihash_pow_hits` counts the solutions the device filter passed: it
stays 0 if the miner falls back to the host-side `accept` path.
"""
import os
import time

import pytest

from bitcoincashplus_amd.node.process import BIN_DIR, BcpdProcess
from bitcoincashplus_amd.testing.messages import REGTEST_BCP_HEIGHT

pytestmark = [pytest.mark.gpu, pytest.mark.functional]

POST_FORK = 5  # blocks mined past the fork height


def wait_until(pred, timeout, what, step=0.05):
    deadline = time.time() + timeout
    while time.time() < deadline:
        if pred():
            return
        time.sleep(step)
    raise AssertionError(f"timed out waiting for {what}")


def test_gpu_node_mines_with_device_filter(tmp_path):
    if not os.path.exists(os.path.join(BIN_DIR, "bcpd")):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.dirname(BIN_DIR), "-j8", "tools"])
    a = BcpdProcess(os.path.join(str(tmp_path), "a"), extra_args=["-gpu=1", "-whitelist=127.0.0.1"])
    b = BcpdProcess(os.path.join(str(tmp_path), "b"), extra_args=["-gpu=0", "-whitelist=127.0.0.1"])
    a.start()
    b.start()
    try:
        a.rpc.generate(REGTEST_BCP_HEIGHT - 1)
        before = a.rpc.getmininginfo()["miner"]
        assert before["equihash_pow_hits"] == 0 and before["equihash_solutions"] == 0, before
        hashes = a.rpc.generate(POST_FORK)
        assert len(hashes) == POST_FORK
        assert a.rpc.getblockcount() == REGTEST_BCP_HEIGHT - 1 + POST_FORK
        mi = a.rpc.getmininginfo()["miner"]
        print(f"miner after {POST_FORK} post-fork blocks: {mi}")
        assert mi["enabled"] and mi["gpu_ms"] > 0, mi
        # every block came from a device hit, and the filter saw no fewer solutions than it passed
        assert mi["equihash_pow_hits"] >= POST_FORK, mi
        assert mi["equihash_solutions"] >= mi["equihash_pow_hits"], mi
        b.rpc.addnode(f"127.0.0.1:{a.p2p_port}", "add")
        wait_until(lambda: a.rpc.getbestblockhash() == b.rpc.getbestblockhash(), 300, "B syncing A's chain")
        tip = b.rpc.getblockheader(b.rpc.getbestblockhash())
        assert tip["hash"] == hashes[-1] and tip["height"] == REGTEST_BCP_HEIGHT - 1 + POST_FORK
        assert b.rpc.getmininginfo()["miner"]["equihash_pow_hits"] == 0
    finally:
        a.stop()
        b.stop()
