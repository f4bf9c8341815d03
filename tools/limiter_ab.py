#!/usr/bin/env python3
"""ms per tracer step with and without the limiter (limiter_option 8 / 0), interleaved on one GPU.

One context at a time (two ne120/q35 contexts do not fit side by side): for each round and each option, a fresh PrimRun of DCMIP 1-1
runs --warmup whole rsplit cycles, then --cycles timed cycles of the device-resident loop (prim_run_subcycle; tracer steps, device
winds and the fused remap); ms/step = wall time / tracer steps.  Prints one JSON line per measurement and a summary line.

    python tools/limiter_ab.py --ne 120 --qsize 35 [--rounds 2] [--cycles 3] [--warmup 1] [--options 8,0]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(ne, qsize, limiter_option, warmup, cycles):
    from transport_se_amd.driver import PrimRun
    run = PrimRun(ne, qsize, test_case=1, limiter_option=limiter_option)
    try:
        r = run.rsplit
        run.run(warmup * r)
        run.hip.synchronize()
        t0 = time.perf_counter()
        run.run(cycles * r)
        run.hip.synchronize()
        return 1e3 * (time.perf_counter() - t0) / (cycles * r)
    finally:
        run.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=120); ap.add_argument("--qsize", type=int, default=35)
    ap.add_argument("--rounds", type=int, default=2); ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--options", default="8,0", help="limiter options to alternate (e.g. 0: the unlimited route alone, for a profile)")
    a = ap.parse_args()
    opts = [int(x) for x in a.options.split(",")]
    got = {8: [], 0: []}
    for rnd in range(a.rounds):
        for opt in (opts if rnd % 2 == 0 else opts[::-1]):
            ms = measure(a.ne, a.qsize, opt, a.warmup, a.cycles)
            got[opt].append(ms)
            print(json.dumps({"round": rnd, "limiter_option": opt, "ne": a.ne, "qsize": a.qsize, "ms_per_step": round(ms, 3)}), flush=True)
    print(json.dumps({"ne": a.ne, "qsize": a.qsize, "ms_per_step_limiter8": [round(x, 3) for x in got[8]],
                      "ms_per_step_unlimited": [round(x, 3) for x in got[0]]}), flush=True)


if __name__ == "__main__":
    main()
