#!/usr/bin/env python3
"""Rate of tse_sphere_op_view -- gradient, divergence and vorticity, LOCAL and C0 -- against tse_dss_view(AVERAGE) on an array of the
output's shape and layout, a plain device-to-device copy of the input's plus the output's bytes, and tse_vlaplace_view order 1 on the
same wind.

  python tools/sphere_op_rate.py [--ne 30] [--seconds 0.5] [--out FILE]

A wind of nlev levels (2 * nlev layers) and a scalar of nlev levels of a one-rank context, laid out four ways: dense point-fastest
([ie][c][k][j][i] and [ie][k][j][i], path 0), E3SM's state%v order ([ie][k][c][j][i]: component stride 16, level stride 32; the scalar
dense; path 0), dense level-fastest ([ie][c][j][i][k], path 1) and [ie][c][k][i][j] (path 2).  Every call is timed with device events on a
side stream, after warm-up, the kinds alternated inside one loop with a plain copy of three fields of nlev levels (what an operator reads
plus what it writes), until every kind has at least --seconds of device time.  tse_dss_view(AVERAGE) runs in place on a scratch array of
the output's shape that is refilled before every call, outside the timed interval.  The expectation to read the table against: C0 costs
about one tse_dss_view of the output plus one read of the input; the column "x (local + dss)" is C0 over the sum of the LOCAL call and
tse_dss_view run separately.  The time of the "fieldop" timer group (the two kernels, without the stream hand-over) is printed beside,
from a second loop with tse_timing on.  The table goes to stdout and, with --out, is appended to FILE (profiles/sphere_op_rate.txt holds
a record).  Needs the GPU; there is no CPU fallback."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

OPS = ("gradient", "divergence", "vorticity")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=30)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sphere_op_rate: no GPU (rates are measured on the device only)")
    from view_rate import context
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.hip_mod import build_dss_view, sphere_op_view_plan
    hip = context(args.ne, 4)
    geo = cm.geometry(args.ne)
    hip.vector_setup(geo["D"], cm.metinv(geo["D"]), geo["mp"])
    n, K = hip.nelemd, hip.nlev
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    wind0 = 30.0 * (torch.rand((n, 2, K, 4, 4), dtype=torch.float64, device="cuda", generator=gen) - 0.5)
    scal0 = 30.0 * (torch.rand((n, 1, K, 4, 4), dtype=torch.float64, device="cuda", generator=gen) - 0.5)
    csrc = torch.empty((n, 3, K, 4, 4), dtype=torch.float64, device="cuda").copy_(torch.cat([wind0, scal0], dim=1))
    cdst = torch.empty_like(csrc)
    nbytes = 2 * csrc.numel() * 8
    wshape = {"eqkji": (n, 2, K, 4, 4), "ekqji": (n, K, 2, 4, 4), "eqjik": (n, 2, 4, 4, K), "eqkij": (n, 2, K, 4, 4)}
    sshape = {"ekji": (n, K, 4, 4), "ejik": (n, 4, 4, K), "ekij": (n, K, 4, 4)}
    new = lambda shape: torch.empty(shape, dtype=torch.float64, device="cuda")   # noqa: E731
    # name -> (wind axes, scalar axes, path)
    layouts = {"point-fastest": ("eqkji", "ekji", 0), "state%v [k][c][j][i]": ("ekqji", "ekji", 0), "level-fastest": ("eqjik", "ejik", 1),
               "generic [k][i][j]": ("eqkij", "ekij", 2)}
    wdense = lambda t, axes: {"eqkji": t, "ekqji": t.permute(0, 2, 1, 3, 4), "eqjik": t.permute(0, 1, 4, 2, 3), "eqkij": t.permute(0, 1, 2, 4, 3)}[axes]   # noqa: E731
    sdense = lambda t, axes: {"ekji": t, "ejik": t.permute(0, 3, 1, 2), "ekij": t.permute(0, 1, 3, 2)}[axes].unsqueeze(1)   # noqa: E731
    F = {}
    for name, (wa, sa, path) in layouts.items():
        # the two inputs, an output and a dss scratch of either shape, and a wind-shaped output for tse_vlaplace_view
        F[name] = dict(w=new(wshape[wa]), s=new(sshape[sa]), ow=new(wshape[wa]), os=new(sshape[sa]), dw=new(wshape[wa]), ds=new(sshape[sa]), wa=wa, sa=sa)
        vw, vs = build_dss_view(F[name]["w"], wa, n)[0], build_dss_view(F[name]["s"], sa, n)[0]
        vow, vos = build_dss_view(F[name]["ow"], wa, n)[0], build_dss_view(F[name]["os"], sa, n)[0]
        assert [p["path"] for p in sphere_op_view_plan(n, K, "gradient", vs, vow)] == [path, path], name
        assert [p["path"] for p in sphere_op_view_plan(n, K, "vorticity", vw, vos)] == [path, path], name

    def call(f, op, c0, s):
        if op == "gradient":
            hip.sphere_op_view(f["s"], f["sa"], f["ow"], f["wa"], op=op, c0=c0, stream=s)
        else:
            hip.sphere_op_view(f["w"], f["wa"], f["os"], f["sa"], op=op, c0=c0, stream=s)

    s = torch.cuda.Stream()
    copy = lambda: cdst.copy_(csrc)   # noqa: E731
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for f in F.values():
            wdense(f["w"], f["wa"]).copy_(wind0)
            sdense(f["s"], f["sa"]).copy_(scal0)
        # the bits first: the four layouts hold the same fields and must get the same result, for every operator and mode
        for op in OPS:
            for c0 in (False, True):
                for f in F.values():
                    call(f, op, c0, s)
                s.synchronize()
                out = lambda f: wdense(f["ow"], f["wa"]) if op == "gradient" else sdense(f["os"], f["sa"])   # noqa: E731
                ref = out(F["point-fastest"]).clone()
                for name, f in F.items():
                    assert torch.equal(out(f), ref), "the paths disagree: %s %s c0=%d" % (name, op, c0)
                    assert torch.equal(wdense(f["w"], f["wa"]), wind0) and torch.equal(sdense(f["s"], f["sa"]), scal0), "in changed: " + name
        kinds = {}
        for k, f in F.items():
            for op in OPS:
                for c0 in (False, True):
                    kinds[(k, "%s %s" % (op, "C0" if c0 else "local"))] = (None, lambda f=f, op=op, c0=c0: call(f, op, c0, s))
            kinds[(k, "dss_view nf=1")] = (lambda f=f: f["ds"].copy_(f["s"]), lambda f=f: hip.dss_view(f["ds"], f["sa"], mode="average", stream=s))
            kinds[(k, "dss_view nf=2")] = (lambda f=f: f["dw"].copy_(f["w"]), lambda f=f: hip.dss_view(f["dw"], f["wa"], mode="average", stream=s))
            kinds[(k, "vlaplace 1")] = (None, lambda f=f: hip.vlaplace_view(f["w"], f["wa"], out=f["ow"], order=1, stream=s))
        for _ in range(3):   # warm-up of every shape timed below
            for pre, g in kinds.values():
                if pre:
                    pre()
                g()
            copy()
        s.synchronize()
        times = {k: [] for k in kinds}; times[("plain copy", "")] = []
        total = {k: 0.0 for k in times}
        while min(total.values()) < args.seconds * 1e3:
            evs = []
            for k, (pre, g) in kinds.items():   # call, plain copy, call, plain copy, ...
                if pre:
                    pre()
                for name, fn in ((k, g), (("plain copy", ""), copy)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(s); fn(); b.record(s)
                    evs.append((name, a, b))
            s.synchronize()
            for name, a, b in evs:
                ms = a.elapsed_time(b); times[name].append(ms); total[name] += ms
        # the kernels alone: the "fieldop" group, 20 calls per layout, operator and mode
        group = {}
        for k, f in F.items():
            for op in OPS:
                for c0 in (False, True):
                    hip.timing(True)
                    for _ in range(20):
                        call(f, op, c0, s)
                    s.synchronize()
                    ms, launches = hip.kernel_time("fieldop")
                    assert launches == 40, launches
                    group[(k, "%s %s" % (op, "C0" if c0 else "local"))] = ms / 20
        hip.timing(False)
    med = {k: float(np.median(v)) for k, v in times.items()}
    base = med[("plain copy", "")]
    lines = ["tse_sphere_op_view vs tse_dss_view(AVERAGE) on the output's shape, tse_vlaplace_view order 1 and a plain device-to-device copy of input "
             "plus output bytes: ne%d (%d elements), one rank, %d levels, copy of %.3f GB read + written%s" % (args.ne, n, K, nbytes / 1e9, ("; " + args.note) if args.note else ""),
             "%s, torch %s; device events on a side stream, 3 warm-up rounds, window >= %.1f s of device time per kind; fieldop: the two kernels "
             "of a call, mean of 20 calls" % (torch.cuda.get_device_name(0), torch.__version__, args.seconds),
             "%-22s %-18s %6s %9s %9s %9s %9s %7s %7s %15s %10s" % ("layout", "kind", "calls", "median ms", "mean ms", "min ms", "max ms", "x copy", "x dss",
                                                                 "x (local + dss)", "fieldop ms")]
    for k, v in times.items():
        op = k[1].split(" ")[0]
        dss = med.get((k[0], "dss_view nf=2" if op == "gradient" else "dss_view nf=1")) if op in OPS + ("vlaplace",) else None
        if op == "vlaplace":
            dss = med.get((k[0], "dss_view nf=2"))
        both = "-"
        if k[1].endswith(" C0"):
            both = "%.3f" % (med[k] / (med[(k[0], op + " local")] + dss))
        lines.append("%-22s %-18s %6d %9.4f %9.4f %9.4f %9.4f %7.3f %7s %15s %10s" % (
            k[0], k[1], len(v), med[k], float(np.mean(v)), min(v), max(v), med[k] / base, "%.3f" % (med[k] / dss) if dss else "-", both,
            "%.4f" % group[k] if k in group else "-"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n\n")
    hip.close()


if __name__ == "__main__":
    main()
