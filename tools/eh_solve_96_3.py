#!/usr/bin/env python3
"""Solves Equihash(96,3) once on the CPU for a few headers and writes the header inputs and the
solutions, as hex, to tests/data/equihash_96_3.json: the accept side of the (96,3) vectors
(tests/equihash_vectors.py re-checks every entry with the Python oracle before use).

(96,3) has 2^25 leaves of 25-bit indices, so one solve takes about half a minute; the tests never
solve it themselves.

    python tools/eh_solve_96_3.py [--headers 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import equihash_vectors as V  # noqa: E402
from bitcoincashplus_amd import native  # noqa: E402
from bitcoincashplus_amd.utils import equihash_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--headers", type=int, default=3)
    ap.add_argument("--out", default=V.DATA_96_3)
    args = ap.parse_args()
    entries = []
    for nonce in range(args.headers):
        data = V.header_input(nonce)
        st = native.EquihashState(96, 3)
        st.update(data)
        t0 = time.time()
        sols, _ = native.eh_solve_cpu(96, 3, st)
        print(f"nonce {nonce}: {len(sols)} solutions in {time.time() - t0:.0f} s", flush=True)
        for s in sorted(bytes(x) for x in sols):
            assert R.is_valid_solution(96, 3, data, s)
            entries.append({"nonce": nonce, "input": data.hex(), "solution": s.hex()})
    with open(args.out, "w") as f:
        json.dump({"n": 96, "k": 3, "solutions": entries}, f, indent=1)
        f.write("\n")
    print(f"{len(entries)} solutions -> {args.out}")


if __name__ == "__main__":
    main()
