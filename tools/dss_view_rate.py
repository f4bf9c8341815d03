#!/usr/bin/env python3
"""Rate of tse_dss_view against a plain device-to-device copy of the same bytes.

  python tools/dss_view_rate.py [--ne 30] [--nf 4] [--seconds 0.5] [--out FILE]

nf fields of nlev levels (nf * nlev layers: u, v, T, dp3d of one Runge-Kutta stage) of a one-rank context, laid out four ways: dense
point-fastest ([ie][q][k][j][i], path 0), dense level-fastest ([ie][q][j][i][k], path 1), level-fastest rows padded to the odd pitch
nlev + 3 (path 1, 8 bytes per lane) and [ie][q][k][i][j] (path 2).  Every call is timed with device events on a side stream, after
warm-up, alternated with a plain `dst.copy_(src)` of nf * nlev * 16 doubles per element inside the same loop, until every kind has at
least --seconds of device time.  The call crosses the field twice (view -> staging field, staging field -> view: the field is read twice
and written twice), the plain copy once, so the yardstick is not a bound.  The time of the "fielddss" timer group (the two kernels, without
the stream hand-over) is printed beside it, from a second loop with tse_timing on.  The table goes to stdout and, with --out, is
appended to FILE (profiles/dss_view_rate.txt holds a record).  Needs the GPU; there is no CPU fallback."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=30)
    ap.add_argument("--nf", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("dss_view_rate: no GPU (rates are measured on the device only)")
    from view_rate import context
    from transport_se_amd.hip_mod import dss_view_plan
    hip = context(args.ne, 4)
    n, nf, K = hip.nelemd, args.nf, hip.nlev
    nbytes = n * nf * K * 16 * 8
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    S = K + 3
    src = torch.rand((n, nf, K, 4, 4), dtype=torch.float64, device="cuda", generator=gen) + 0.5
    dst = torch.empty_like(src)
    pad = torch.zeros((n, nf, 4, 4, S), dtype=torch.float64, device="cuda")
    fields = {
        "point-fastest": (torch.empty((n, nf, K, 4, 4), dtype=torch.float64, device="cuda"), "eqkji", 0),
        "level-fastest": (torch.empty((n, nf, 4, 4, K), dtype=torch.float64, device="cuda"), "eqjik", 1),
        "level-fastest, pitch %d" % S: (pad[..., :K], "eqjik", 1),
        "generic [k][i][j]": (torch.empty((n, nf, K, 4, 4), dtype=torch.float64, device="cuda"), "eqkij", 2),
    }
    from transport_se_amd.hip_mod import build_dss_view
    for name, (t, axes, path) in fields.items():
        v, f_, k_ = build_dss_view(t, axes, n)
        got = dss_view_plan(n, f_, k_, v)["path"]
        assert (f_, k_, got) == (nf, K, path), (name, f_, k_, got)
    s = torch.cuda.Stream()
    copy = lambda: dst.copy_(src)   # noqa: E731

    def fill():
        for t, axes, _ in fields.values():
            t.copy_(src if axes == "eqkji" else src.permute(0, 1, 3, 4, 2) if axes == "eqjik" else src.permute(0, 1, 2, 4, 3))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        # the bits first: the four layouts hold the same field and must get the same result
        fill()
        for t, axes, _ in fields.values():
            hip.dss_view(t, axes, stream=s)
        s.synchronize()
        ref = fields["point-fastest"][0]
        assert not torch.equal(ref, src)
        assert torch.equal(fields["level-fastest"][0].permute(0, 1, 4, 2, 3), ref) and torch.equal(pad[..., :K].permute(0, 1, 4, 2, 3), ref)
        assert torch.equal(fields["generic [k][i][j]"][0].permute(0, 1, 2, 4, 3), ref), "the paths disagree"
        for _ in range(3):   # warm-up of every shape timed below (a DSS'd field is a fixed point up to rounding: no growth)
            for t, axes, _ in fields.values():
                hip.dss_view(t, axes, stream=s)
            copy()
        s.synchronize()
        times = {k: [] for k in fields}; times["plain copy"] = []
        total = {k: 0.0 for k in times}
        while min(total.values()) < args.seconds * 1e3:
            evs = []
            for k, (t, axes, _) in fields.items():   # call, plain copy, call, plain copy, ...
                for name, g in ((k, lambda: hip.dss_view(t, axes, stream=s)), ("plain copy", copy)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(s); g(); b.record(s)
                    evs.append((name, a, b))
            s.synchronize()
            for name, a, b in evs:
                ms = a.elapsed_time(b); times[name].append(ms); total[name] += ms
        # the kernels alone: the "fielddss" group, 20 calls per layout
        group = {}
        for k, (t, axes, _) in fields.items():
            hip.timing(True)
            for _ in range(20):
                hip.dss_view(t, axes, stream=s)
            s.synchronize()
            ms, launches = hip.kernel_time("fielddss")
            assert launches == 40, launches
            group[k] = ms / 20
        hip.timing(False)
    base = float(np.mean(times["plain copy"]))
    lines = ["tse_dss_view vs a plain device-to-device copy of the same bytes: ne%d (%d elements), one rank, %d fields x %d levels = %d layers, %.3f GB"
             % (args.ne, n, nf, K, nf * K, nbytes / 1e9),
             "%s, torch %s; device events on a side stream, 3 warm-up rounds, window >= %.1f s of device time per kind; fielddss: the two kernels "
             "of a call, mean of 20 calls" % (torch.cuda.get_device_name(0), torch.__version__, args.seconds),
             "%-28s %6s %10s %10s %10s %8s %12s" % ("kind", "calls", "mean ms", "min ms", "max ms", "x copy", "fielddss ms")]
    for k, v in times.items():
        m = float(np.mean(v))
        lines.append("%-28s %6d %10.4f %10.4f %10.4f %8.3f %12s" % (k, len(v), m, min(v), max(v), m / base, "%.4f" % group[k] if k in group else "-"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n\n")
    hip.close()


if __name__ == "__main__":
    main()
