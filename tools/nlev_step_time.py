"""ms per tracer step of the DCMIP 1-1 case at ne/qsize on one GPU for a given vertical grid (default the 12k_top-64 fixtures),
timed as bench.py times the flagship (warm-up, then whole rsplit cycles through the device-resident loop), with the per-kernel
HIP-event times: python tools/nlev_step_time.py [--ne 120 --qsize 35 --steps 12 --warmup 3 --vfile-mid M --vfile-int I
--limiter-option 8|9|0]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    vc = os.path.join(ROOT, "tests", "golden", "vcoord")
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=120)
    ap.add_argument("--qsize", type=int, default=35)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vfile-mid", default=os.path.join(vc, "12k_top-64m.ascii"))
    ap.add_argument("--vfile-int", default=os.path.join(vc, "12k_top-64i.ascii"))
    ap.add_argument("--limiter-option", type=int, default=8, help="control_mod's limiter_option: 8, 9 (clip-and-sum) or 0 (none)")
    a = ap.parse_args()
    import torch
    from transport_se_amd.driver import PrimRun
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord(a.vfile_mid, a.vfile_int)
    run = PrimRun(a.ne, a.qsize, test_case=1, hvcoord=hv, limiter_option=a.limiter_option)
    run.run(a.warmup)
    run.hip.synchronize(); torch.cuda.synchronize()
    run.hip.timing(True)
    t0 = time.perf_counter()
    run.run(a.steps)
    run.hip.synchronize(); torch.cuda.synchronize()
    el = time.perf_counter() - t0
    kt = {k: run.hip.kernel_time(k) for k in ("advance0", "advance1", "advance2", "lap", "dss", "minmax", "remap", "level", "dcmip", "avg")}
    print(json.dumps(dict(ne=a.ne, qsize=a.qsize, nlev=run.nlev, limiter_option=a.limiter_option, steps=a.steps, warmup=a.warmup, ms_per_step=1e3 * el / a.steps,
                          kernel_ms_per_step={k: v[0] / a.steps for k, v in kt.items()},
                          launches_per_step={k: v[1] / a.steps for k, v in kt.items()})))
    run.close()


if __name__ == "__main__":
    main()
