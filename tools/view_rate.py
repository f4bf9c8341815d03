#!/usr/bin/env python3
"""Rate of the strided device views (tse_view_put / tse_view_get of "qdp") against a plain device-to-device copy of the same bytes.

  python tools/view_rate.py [--ne 30] [--qsize 35] [--seconds 1.0] [--out FILE]

For a dense level-fastest ([ie][q][j][i][k], path 1: the transposing kernel) and a dense point-fastest ([ie][q][k][j][i], path 0) device
tensor it times put and get with device events on a side stream, after warm-up, alternating every view call with a plain
`dst.copy_(src)` of a tensor of the same size inside the same loop, until every kind has at least --seconds of device time.  Both a
view call and the plain copy read and write every byte exactly once, so the yardstick is the plain copy: path 1 is accepted at no more
than 1.25 x its time.  tse_copy_qdp_h2d / _d2h from a numpy array are timed once for scale.  The table goes to stdout and, with --out, is appended to FILE
(profiles/device_views_rate.txt holds a record).  Needs the GPU; there is no CPU fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def context(ne, qsize):
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.driver import partition
    from transport_se_amd.hip_mod import HipMod
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord()
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    d = cm.edge_descriptors(topo, partition(ne, 1), 0)
    elem = dict(Dinv=geo["Dinv"], metdet=geo["metdet"], rmetdet=geo["rmetdet"], spheremp=geo["spheremp"], rspheremp=geo["rspheremp"],
                putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    return HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, 0.0, device=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=30)
    ap.add_argument("--qsize", type=int, default=35)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("view_rate: no GPU (rates are measured on the device only)")
    hip = context(args.ne, args.qsize)
    n, qs, K = hip.nelemd, hip.qsize, hip.nlev
    nbytes = n * qs * K * 16 * 8
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    lf = torch.rand((n, qs, 4, 4, K), dtype=torch.float64, device="cuda", generator=gen)    # level-fastest
    pf = torch.zeros((n, qs, K, 4, 4), dtype=torch.float64, device="cuda")                  # point-fastest
    dst = torch.empty_like(lf)
    plans = dict(lf=hip.view_plan("qdp", lf, "eqjik")["path"], pf=hip.view_plan("qdp", pf, "eqkji")["path"])
    assert plans == dict(lf=1, pf=0), plans
    s = torch.cuda.Stream()
    kinds = {
        "put level-fastest": lambda: hip.put("qdp", lf, "eqjik", nt=1, stream=s),
        "get level-fastest": lambda: hip.get("qdp", lf, "eqjik", nt=1, stream=s),
        "put point-fastest": lambda: hip.put("qdp", pf, "eqkji", nt=1, stream=s),
        "get point-fastest": lambda: hip.get("qdp", pf, "eqkji", nt=1, stream=s),
    }
    copy = lambda: dst.copy_(lf)   # noqa: E731
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        # the bits first: what went in level-fastest comes out point-fastest
        kinds["put level-fastest"](); kinds["get point-fastest"]()
        s.synchronize()
        assert torch.equal(pf, lf.permute(0, 1, 4, 2, 3)), "view round trip changed the data"
        for _ in range(3):   # warm-up of every shape timed below
            for f in kinds.values():
                f()
            copy()
        s.synchronize()
        times = {k: [] for k in kinds}; times["plain copy"] = []
        total = {k: 0.0 for k in times}
        while min(total.values()) < args.seconds * 1e3:
            evs = []
            for k, f in kinds.items():   # view call, plain copy, view call, plain copy, ...
                for name, g in ((k, f), ("plain copy", copy)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(s); g(); b.record(s)
                    evs.append((name, a, b))
            s.synchronize()
            for name, a, b in evs:
                ms = a.elapsed_time(b); times[name].append(ms); total[name] += ms
    # the host route, once, for scale
    host = np.zeros((n, 2, qs, K, 4, 4))
    t0 = time.perf_counter(); hip.copy_qdp_h2d(dict(Qdp=host), 1); t_h2d = time.perf_counter() - t0
    t0 = time.perf_counter(); hip.copy_qdp_d2h(dict(Qdp=host), 1); t_d2h = time.perf_counter() - t0
    ref = float(np.mean(times["plain copy"]))
    lines = ["device views vs a plain device-to-device copy: qdp, ne%d (%d elements), %d tracers, %d levels, %.3f GB per time level"
             % (args.ne, n, qs, K, nbytes / 1e9),
             "%s, torch %s; device events on a side stream, %d warm-up rounds, window >= %.1f s of device time per kind"
             % (torch.cuda.get_device_name(0), torch.__version__, 3, args.seconds),
             "%-20s %6s %10s %10s %10s %10s %8s" % ("kind", "calls", "mean ms", "min ms", "max ms", "GB/s r+w", "x copy")]
    for k, v in times.items():
        m = float(np.mean(v))
        lines.append("%-20s %6d %10.4f %10.4f %10.4f %10.1f %8.3f" % (k, len(v), m, min(v), max(v), 2 * nbytes / m / 1e6, m / ref))
    worst = max(float(np.mean(times[k])) / ref for k in ("put level-fastest", "get level-fastest"))
    lines.append("path 1 (level-fastest) at %.3f x the plain copy: %s the 1.25 x bound" % (worst, "inside" if worst <= 1.25 else "OUTSIDE"))
    lines.append("host route for scale, one call each from a numpy array: tse_copy_qdp_h2d %.1f ms (%.2f GB/s), tse_copy_qdp_d2h %.1f ms (%.2f GB/s)"
                 % (t_h2d * 1e3, nbytes / t_h2d / 1e9, t_d2h * 1e3, nbytes / t_d2h / 1e9))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n\n")
    hip.close()


if __name__ == "__main__":
    main()
