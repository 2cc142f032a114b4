#!/usr/bin/env python3
"""Cost of the device-side target filter: the mining loop with launch_pow / collect_pow next to
the same loop with launch / collect, over the same nonces, alternated on one GPU.

python tools/eh_pow_loop.py [--reps 5] [--steps 10] [--batch 96] [--once pow|plain|host]
Each rep runs three loops (two solvers in flight, as bench.py). "plain" is launch / collect alone:
a BLAKE2b state per nonce before the launch, the minimal encoding of every solution after it.
"host" adds what the miner's accept path does per solution: a SHA-256d of the 1,487-byte header
compared with the target. "pow" passes header, first nonce, count and target and reads back the
hits.
The target is the mainnet powLimitStart, so almost nothing passes. Prints one JSON line per run
and a summary (median, min, max Sol/s per loop). --once runs one loop once (for a kernel trace).
"""
import argparse
import collections
import hashlib
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADER = bytes((i * 37 + 11) & 0xFF for i in range(108))
TARGET = bytes.fromhex("00000fffffffffffffffffffffffffffffffffffffffffffffffffffffffffff")[::-1]  # mainnet powLimitStart
TINT = int.from_bytes(TARGET, "little")


def nonce_of(i):
    return struct.pack("<QQQQ", i, 0, 0, 0)


def loop(native, solvers, steps, batch, mode):
    pow_mode, host_check = mode == "pow", mode == "host"
    pending = collections.deque()
    nsol = nhit = 0
    t0 = time.perf_counter()

    def collect():
        nonlocal nsol, nhit
        s, sv = pending.popleft()
        if pow_mode:
            r = sv.collect_pow()
            nsol += r["solutions"]
            nhit += len(r["hits"])
        else:
            for b, sols in enumerate(sv.collect()):
                nsol += len(sols)
                inp = HEADER + nonce_of(s * batch + b)
                for x in sols if host_check else ():
                    h = hashlib.sha256(hashlib.sha256(inp + b"\xfd\x40\x05" + x).digest()).digest()
                    nhit += int.from_bytes(h, "little") <= TINT

    for s in range(steps):
        if len(pending) == len(solvers):
            collect()
        sv = solvers[s % len(solvers)]
        if pow_mode:
            sv.launch_pow(HEADER, nonce_of(s * batch), batch, TARGET)
        else:
            sts = []
            for b in range(batch):
                st = native.EquihashState(200, 9)
                st.update(HEADER + nonce_of(s * batch + b))
                sts.append(st)
            sv.launch(sts)
        pending.append((s, sv))
    while pending:
        collect()
    dt = time.perf_counter() - t0
    return {"loop": mode, "sol_per_s": round(nsol / dt, 1), "ms_per_step": round(1e3 * dt / steps, 3),
            "solutions": nsol, "hits": nhit}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--once", choices=["pow", "plain", "host"], default=None)
    a = ap.parse_args()
    from bitcoincashplus_amd import native, require_gpu
    require_gpu("eh_pow_loop")
    solvers = [native.EquihashGpuSolver(200, 9, a.batch, 0) for _ in range(2)]
    if a.once:
        print(json.dumps(loop(native, solvers, a.steps, a.batch, a.once)), flush=True)
        return
    loop(native, solvers, 2, a.batch, "pow")  # warm-up of both paths
    loop(native, solvers, 2, a.batch, "plain")
    res = {"plain": [], "host": [], "pow": []}
    for _ in range(a.reps):
        for mode in res:
            r = loop(native, solvers, a.steps, a.batch, mode)
            res[r["loop"]].append(r["sol_per_s"])
            print(json.dumps(r), flush=True)
    print(json.dumps({k: {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
                      for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
