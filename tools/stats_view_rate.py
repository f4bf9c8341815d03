#!/usr/bin/env python3
"""Rate of tse_stats_view against tse_dss_view of the same view and a plain device-to-device copy of the same bytes.

  python tools/stats_view_rate.py [--ne 30] [--nf 1,2,35] [--calls 20] [--out FILE]

nf fields of nlev levels of a one-rank context, laid out three ways: dense point-fastest ([ie][q][k][j][i], path 0), dense level-fastest
([ie][q][j][i][k], path 1) and [ie][q][k][i][j] (path 2); the field alone, with a reference of the same layout, and with a reference and
a weight (one point-fastest field of nlev levels).  After warm-up every kind is called --calls times (at least 20), alternating in the
same loop and the same process with tse_dss_view of the same view and a plain `dst.copy_(src)` of the field's bytes; the medians are
reported.  A stats call is complete on return, so its time is the host's wall clock around the call; the time of its one kernel is the
"fieldstats" timer group of a second loop, the difference is the host-side share of a call (the stream hand-over, the copy of the shares
to the host and the wait for it).  GB/s is the bytes of all inputs read once over the kernel's time.  tse_dss_view and the copy are timed
with device events on the stream.  The table goes to stdout and, with --out, is appended to FILE (profiles/stats_view_rate.txt holds a
record).  Needs the GPU; there is no CPU fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=30)
    ap.add_argument("--nf", default="1,2,35")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    calls = max(20, args.calls)
    import torch
    if not torch.cuda.is_available():
        sys.exit("stats_view_rate: no GPU (rates are measured on the device only)")
    from view_rate import context
    from transport_se_amd.hip_mod import build_dss_view, dss_view_plan
    hip = context(args.ne, 4)
    n, K = hip.nelemd, hip.nlev
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    s = torch.cuda.Stream()
    lines = ["tse_stats_view vs tse_dss_view of the same view and a plain copy of the field: ne%d (%d elements), one rank, %d levels; %s, torch %s"
             % (args.ne, n, K, torch.cuda.get_device_name(0), torch.__version__),
             "3 warm-up rounds, median of %d calls per kind, the kinds alternating in one loop; stats ms: wall clock of a call (complete on return); "
             "kernel ms: the fieldstats group; host ms: their difference; GB/s: bytes of all inputs over the kernel's time; dss ms, copy ms: device events" % calls,
             "%3s %-18s %-12s %9s %10s %9s %9s %9s %9s %10s %10s" % ("nf", "layout", "inputs", "stats ms", "kernel ms", "host ms", "GB/s", "dss ms", "copy ms", "stats/dss", "kernel/dss")]
    for nf in [int(x) for x in args.nf.split(",")]:
        src = torch.rand((n, nf, K, 4, 4), dtype=torch.float64, device="cuda", generator=gen) + 0.5
        dst = torch.empty_like(src)
        wgt = torch.rand((n, K, 4, 4), dtype=torch.float64, device="cuda", generator=gen) + 1.0
        layouts = {"point-fastest": ("eqkji", 0, lambda t: t.contiguous()), "level-fastest": ("eqjik", 1, lambda t: t.permute(0, 1, 3, 4, 2).contiguous()),
                   "generic [k][i][j]": ("eqkij", 2, lambda t: t.permute(0, 1, 2, 4, 3).contiguous())}
        want = None
        for name, (axes, path, lay) in layouts.items():
            f, r = lay(src), lay(src * 1.001)
            v, f_, k_ = build_dss_view(f, axes, n)
            assert (f_, k_, dss_view_plan(n, f_, k_, v)["path"]) == (nf, K, path), name
            kinds = {"field": {}, "field+ref": dict(ref=r), "field+ref+w": dict(ref=r, weight=wgt, weight_axes="ekji")}
            nin = {"field": 1.0, "field+ref": 2.0, "field+ref+w": 2.0 + 1.0 / nf}
            got = hip.stats_view(f, axes, **kinds["field+ref+w"])
            if want is None:
                want = got
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "the paths disagree"
            work = f.clone()                                   # tse_dss_view works in place: on a copy (a summed field is a fixed point up to rounding)
            for _ in range(3):
                for kw in kinds.values():
                    hip.stats_view(f, axes, stream=s, **kw)
                with torch.cuda.stream(s):
                    hip.dss_view(work, axes, stream=s); dst.copy_(src)
            s.synchronize()
            wall = {k: [] for k in kinds}; ev = {"dss": [], "copy": []}
            for _ in range(calls):
                for k, kw in kinds.items():
                    s.synchronize()                          # (the call waits for the stream: nothing of the loop may be left on it)
                    t0 = time.perf_counter(); hip.stats_view(f, axes, stream=s, **kw); wall[k].append((time.perf_counter() - t0) * 1e3)
                    with torch.cuda.stream(s):
                        for what, g in (("dss", lambda: hip.dss_view(work, axes, stream=s)), ("copy", lambda: dst.copy_(src))):
                            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            a.record(s); g(); b.record(s)
                            ev[what].append((a, b))
                s.synchronize()
            dss, copy = (float(np.median([a.elapsed_time(b) for a, b in ev[w]])) for w in ("dss", "copy"))
            for k, kw in kinds.items():
                hip.timing(True)
                for _ in range(calls):
                    hip.stats_view(f, axes, stream=s, **kw)
                ms, launches = hip.kernel_time("fieldstats")
                assert launches == calls, launches
                hip.timing(False)
                kern, w = ms / calls, float(np.median(wall[k]))
                gbs = nin[k] * src.numel() * 8 / (kern * 1e-3) / 1e9
                lines.append("%3d %-18s %-12s %9.4f %10.4f %9.4f %9.0f %9.4f %9.4f %10.3f %10.3f" % (nf, name, k, w, kern, w - kern, gbs, dss, copy, w / dss, kern / dss))
            del f, r, work
        del src, dst
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n\n")
    hip.close()


if __name__ == "__main__":
    main()
