#!/usr/bin/env python3
"""Overflow rows of the slot rounds (EhCfg::ks) over the bench's inputs: rows that found the 8
slots of their key taken and went through the round's overflow list (BCP_EH_OVL entries).

python tools/eh_overflow.py [--steps 20] [--batch 96]   (BCP_NATIVE_PATH selects a build)
Solves the nonces of bench.py's timed steps and prints, per round, the overflow rows per nonce and
per bucket and the most seen in one bucket: the number the list is sized from (four times it or
more), next to the pair and row drops of the same run.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=96)
    a = ap.parse_args()
    import bench
    from bitcoincashplus_amd import native
    sv = native.EquihashGpuSolver(200, 9, a.batch, 0)
    nsol = 0
    for step in range(a.steps):
        nsol += sum(len(x) for x in sv.solve(bench.step_states(native, a.batch, step, 0)))
    st = sv.stats()
    nonces = a.steps * a.batch
    rows, most = st["overflow_rows_all"], st["overflow_bucket_max"]
    for rnd in range(1, len(rows)):
        if rows[rnd]:
            print(json.dumps({"round": rnd, "overflow_rows": rows[rnd], "per_nonce": round(rows[rnd] / nonces, 1),
                              "per_bucket": round(rows[rnd] / nonces / 512, 3), "most_in_a_bucket": most[rnd]}), flush=True)
    print(json.dumps({"nonces": nonces, "solutions": nsol, "most_in_a_bucket": max(most or [0]),
                      "carry_launches": st["carry_launches"], "pair_dropped_all": st["pair_dropped_all"],
                      "stage_dropped_all": st["stage_dropped_all"], "cand_dropped": st["cand_dropped"]}))


if __name__ == "__main__":
    main()
