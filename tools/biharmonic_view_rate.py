#!/usr/bin/env python3
"""Rate of tse_biharmonic_view (order 1 and order 2) against tse_dss_view(WEAK) on the same array and a plain device-to-device copy.

  python tools/biharmonic_view_rate.py [--ne 30] [--nf 4] [--seconds 0.5] [--out FILE]

nf fields of nlev levels (nf * nlev layers: T, dp3d and two tracers of one hyperviscosity sub-step) of a one-rank context, laid out the
four ways of tools/dss_view_rate.py: dense point-fastest ([ie][q][k][j][i], path 0), dense level-fastest ([ie][q][j][i][k], path 1),
level-fastest rows padded to the odd pitch nlev + 3 (path 1, 8 bytes per lane) and [ie][q][k][i][j] (path 2).  Every call is timed with
device events on a side stream, after warm-up, the kinds alternated inside one loop with a plain `dst.copy_(src)` of the same bytes,
until every kind has at least --seconds of device time.  tse_biharmonic_view writes a second array of the same layout, so that its input
keeps its values over the whole window (in place the field would shrink by the square of the grid spacing over the earth's radius with
every call; the traffic is the same: view -> staging field -> view).  tse_dss_view(WEAK) runs in place on a scratch array of the same
layout that is refilled before every call, outside the timed interval.  Both entries cross the field four times, the plain copy twice.
The time of the "fieldlap" timer group (the two kernels, without the stream hand-over) is printed beside, from a second loop with
tse_timing on.  The table goes to stdout and, with --out, is appended to FILE (profiles/biharmonic_view_rate.txt holds a record).
Needs the GPU; there is no CPU fallback."""
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
        sys.exit("biharmonic_view_rate: no GPU (rates are measured on the device only)")
    from view_rate import context
    from transport_se_amd.hip_mod import biharmonic_view_plan, build_dss_view
    hip = context(args.ne, 4)
    n, nf, K = hip.nelemd, args.nf, hip.nlev
    nbytes = n * nf * K * 16 * 8
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    S = K + 3
    src = 300.0 * (torch.rand((n, nf, K, 4, 4), dtype=torch.float64, device="cuda", generator=gen) + 0.5)
    dst = torch.empty_like(src)

    def alloc(kind):
        if kind == "pad":
            return torch.zeros((n, nf, 4, 4, S), dtype=torch.float64, device="cuda")[..., :K]
        return torch.empty({"eqkji": (n, nf, K, 4, 4), "eqjik": (n, nf, 4, 4, K), "eqkij": (n, nf, K, 4, 4)}[kind], dtype=torch.float64, device="cuda")
    # name -> (in, out, scratch, axes, path)
    fields = {
        "point-fastest": tuple(alloc("eqkji") for _ in range(3)) + ("eqkji", 0),
        "level-fastest": tuple(alloc("eqjik") for _ in range(3)) + ("eqjik", 1),
        "level-fastest, pitch %d" % S: tuple(alloc("pad") for _ in range(3)) + ("eqjik", 1),
        "generic [k][i][j]": tuple(alloc("eqkij") for _ in range(3)) + ("eqkij", 2),
    }
    for name, (t, o, _, axes, path) in fields.items():
        vi, f_, k_ = build_dss_view(t, axes, n)
        vo, _, _ = build_dss_view(o, axes, n)
        got = [p["path"] for p in biharmonic_view_plan(n, f_, k_, vi, vo)]
        assert (f_, k_, got) == (nf, K, [path, path]), (name, f_, k_, got)
    dense = lambda t, axes: t if axes == "eqkji" else t.permute(0, 1, 4, 2, 3) if axes == "eqjik" else t.permute(0, 1, 2, 4, 3)   # noqa: E731
    s = torch.cuda.Stream()
    copy = lambda: dst.copy_(src)   # noqa: E731
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for t, _, _, axes, _ in fields.values():
            dense(t, axes).copy_(src)
        # the bits first: the four layouts hold the same field and must get the same result, for either order
        for order in (1, 2):
            for t, o, _, axes, _ in fields.values():
                hip.biharmonic_view(t, axes, out=o, order=order, stream=s)
            s.synchronize()
            ref = fields["point-fastest"][1]
            assert not torch.equal(ref, src)
            for name, (t, o, _, axes, _) in fields.items():
                assert torch.equal(dense(o, axes), ref), "the paths disagree: " + name
                assert torch.equal(dense(t, axes), src), "in changed: " + name
        kinds = {}
        for k, (t, o, w, axes, _) in fields.items():
            kinds[(k, "order 1")] = (None, lambda t=t, o=o, axes=axes: hip.biharmonic_view(t, axes, out=o, order=1, stream=s))
            kinds[(k, "order 2")] = (None, lambda t=t, o=o, axes=axes: hip.biharmonic_view(t, axes, out=o, order=2, stream=s))
            kinds[(k, "dss_view weak")] = (lambda t=t, w=w: w.copy_(t), lambda w=w, axes=axes: hip.dss_view(w, axes, mode="weak", stream=s))
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
        # the kernels alone: the "fieldlap" group, 20 calls per layout and order
        group = {}
        for k, (t, o, _, axes, _) in fields.items():
            for order in (1, 2):
                hip.timing(True)
                for _ in range(20):
                    hip.biharmonic_view(t, axes, out=o, order=order, stream=s)
                s.synchronize()
                ms, launches = hip.kernel_time("fieldlap")
                assert launches == 40, launches
                group[(k, "order %d" % order)] = ms / 20
        hip.timing(False)
    base = float(np.mean(times[("plain copy", "")]))
    mean = {k: float(np.mean(v)) for k, v in times.items()}
    lines = ["tse_biharmonic_view vs tse_dss_view(WEAK) and a plain device-to-device copy of the same bytes: ne%d (%d elements), one rank, %d fields x %d "
             "levels = %d layers, %.3f GB" % (args.ne, n, nf, K, nf * K, nbytes / 1e9),
             "%s, torch %s; device events on a side stream, 3 warm-up rounds, window >= %.1f s of device time per kind; fieldlap: the two kernels "
             "of a call, mean of 20 calls" % (torch.cuda.get_device_name(0), torch.__version__, args.seconds),
             "%-28s %-14s %6s %10s %10s %10s %10s %8s %8s %12s" % ("layout", "kind", "calls", "median ms", "mean ms", "min ms", "max ms", "x copy", "x dss", "fieldlap ms")]
    for k, v in times.items():
        dss = mean.get((k[0], "dss_view weak"))
        lines.append("%-28s %-14s %6d %10.4f %10.4f %10.4f %10.4f %8.3f %8s %12s" % (k[0], k[1], len(v), float(np.median(v)), mean[k], min(v), max(v), mean[k] / base,
                                                                             "%.3f" % (mean[k] / dss) if dss else "-", "%.4f" % group[k] if k in group else "-"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n\n")
    hip.close()


if __name__ == "__main__":
    main()
