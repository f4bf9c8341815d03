#!/usr/bin/env python3
"""Device time of tse_column_view against tse_view_get of one level field on the same path.

  python tools/column_view_rate.py [--ne 30] [--calls 20] [--out FILE]

Every op of a one-rank context on dense point-fastest arrays ([ie][k][j][i], path 0) and dense level-fastest ones ([ie][j][i][k], path 1;
the nlev + 1 levels of PINT's out then take path 2): PINT, PMID, PHI and OMEGA with the pressure formed on the fly, PHI and OMEGA with p
given, and the two-call sequence PMID then PHI(p) that PHI without p fuses.  After warm-up the kinds are called in --calls rounds (at
least 20), alternating in one loop on one stream with tse_view_get("omega_p") into an array of the same layout; a round's device time per
kind is the difference of the "fieldcol" (or "view") timer group around it, the medians and the quartile spread are reported.  A field
pass is one field of nlev levels read or written once: tse_view_get makes two (the library's field read, the view written), PMID two,
PHI three (dp, T_v, out; four with p; phis is a sixteenth of a level field and is not counted), OMEGA four (dp or p, vgrad_p, divdp, out).  `per pass` is the kind's time per
pass over tse_view_get's time per pass on the same layout in the same run; GB/s is the bytes of all passes over the time.  The table
goes to stdout and, with --out, is appended to FILE (profiles/column_view_rate.txt holds a record).  Needs the GPU; there is no CPU
fallback."""
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    calls = max(20, args.calls)
    import torch
    if not torch.cuda.is_available():
        sys.exit("column_view_rate: no GPU (rates are measured on the device only)")
    from view_rate import context
    hip = context(args.ne, 4)
    n, K = hip.nelemd, hip.nlev
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    s = torch.cuda.Stream()
    rnd = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)
    ptop, rgas = 219.4, 287.04
    lines = ["tse_column_view vs tse_view_get of one level field: ne%d (%d elements), one rank, %d levels; %s, torch %s"
             % (args.ne, n, K, torch.cuda.get_device_name(0), torch.__version__),
             "3 warm-up rounds, %d rounds, the kinds alternating in one loop on one stream; ms: median device time of a call (fieldcol / view "
             "timer group), spread: (q3 - q1) / median; passes: fields of nlev levels read or written; per pass: against view_get of the same layout" % calls,
             "%-14s %-14s %7s %9s %8s %8s %9s" % ("layout", "kind", "passes", "ms", "spread", "GB/s", "per pass")]
    for name, axes, lay in (("point-fastest", "ekji", lambda t: t.contiguous()), ("level-fastest", "ejik", lambda t: t.permute(0, 2, 3, 1).contiguous())):
        dp = lay(100.0 + 50.0 * rnd(n, K, 4, 4)); tv = lay(180.0 + 140.0 * rnd(n, K, 4, 4))
        vg = lay(rnd(n, K, 4, 4) - 0.5); dv = lay(1e-3 * (rnd(n, K, 4, 4) - 0.5))
        phis = 1e4 * rnd(n, 4, 4)
        out, p = torch.empty_like(dp), torch.empty_like(dp)
        pi = lay(torch.empty((n, K + 1, 4, 4), dtype=torch.float64, device="cuda"))
        col = lambda op, **kw: hip.column_view(op, dp_axes=axes, ptop=ptop, rgas=rgas, stream=s, **kw)
        kinds = {
            "view_get": (2, "view", lambda: hip.get("omega_p", out, axes, stream=s)),
            "pint": (2, "fieldcol", lambda: col("pint", dp=dp, out=pi)),
            "pmid": (2, "fieldcol", lambda: col("pmid", dp=dp, out=p)),
            "phi": (3, "fieldcol", lambda: col("phi", dp=dp, a=tv, b=phis, b_axes="eji", out=out)),
            "phi(p)": (4, "fieldcol", lambda: col("phi", dp=dp, p=p, a=tv, b=phis, b_axes="eji", out=out)),
            "pmid+phi(p)": (6, "fieldcol", lambda: (col("pmid", dp=dp, out=p), col("phi", dp=dp, p=p, a=tv, b=phis, b_axes="eji", out=out))),
            "omega": (4, "fieldcol", lambda: col("omega", dp=dp, a=vg, b=dv, out=out)),
            "omega(p)": (4, "fieldcol", lambda: col("omega", p=p, a=vg, b=dv, out=out)),
        }
        for _ in range(3):
            for _, _, call in kinds.values():
                call()
        s.synchronize()
        ms = {k: [] for k in kinds}
        hip.timing(True)
        for _ in range(calls):
            for k, (_, group, call) in kinds.items():
                t0 = hip.kernel_time(group)[0]
                call()
                s.synchronize()
                ms[k].append(hip.kernel_time(group)[0] - t0)
        hip.timing(False)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k, (passes, _, _) in kinds.items():
            q1, q3 = np.percentile(ms[k], [25, 75])
            gbs = passes * dp.numel() * 8 / (med[k] * 1e-3) / 1e9
            lines.append("%-14s %-14s %7d %9.4f %8.3f %8.0f %9.3f" % (name, k, passes, med[k], (q3 - q1) / med[k], gbs, (med[k] / passes) / (med["view_get"] / 2)))
        lines.append("%-14s fused phi / (pmid + phi(p)) = %.3f" % (name, med["phi"] / med["pmid+phi(p)"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n\n")
    hip.close()


if __name__ == "__main__":
    main()
