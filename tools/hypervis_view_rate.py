#!/usr/bin/env python3
"""Rate of tse_hypervis_view against the loop it replaces: tse_biharmonic_view, tse_vlaplace_view, the product, two tse_dss_view(WEAK)
and the addition, with torch doing the product and the addition.

  python tools/hypervis_view_rate.py [--ne 30] [--seconds 0.5] [--out FILE]     (needs the GPU)
  python tools/hypervis_view_rate.py --kres FILE                                (needs hipcc only)

T, dp3d, one more scalar and the wind at nlev levels of a one-rank context -- (3 + 2) * nlev layers -- in the four layouts of
INTEGRATION.md section 2h: dense point-fastest ([ie][q][k][j][i], path 0), dense level-fastest ([ie][q][j][i][k], path 1: 16 bytes per
lane), level-fastest with rows padded to the odd pitch nlev + 3 (path 1: 8 bytes per lane) and [ie][q][k][i][j] (path 2).  Both kinds
update the state in place, with factors of the size a host forms (-nu * dt / hypervis_subcycle, about -1e15), so the values stay
what they are over the whole window.  Every call is
timed with device events on a side stream, after warm-up, the two kinds alternated inside one loop, until each has at least --seconds
of device time; the medians, their ratio and the pass count go to the table.  Before the timing the fused call is held to the loop's
bits in every layout.  The table goes to stdout and, with --out, is appended to FILE (profiles/hypervis_view_rate.txt holds a
record).  --kres: registers, LDS and spills of the call's kernels through tools/kres.sh into FILE (profiles/hypervis_view_kres.txt).

Passes over the fields, in units of one read or one write of the (nf + 2) * nk layers: the loop makes 13 -- biharmonic_view and
vlaplace_view 4 (in, stage, stage, out), the product 2, dss_view 4, the addition 3 -- the fused call 7: x -> stage, stage -> stage2,
stage2 and x -> x, with the neighbours' lines of the two staging fields read from the L2."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
KERNELS = ("k_lap_view_stage", "k_vlap_view_stage", "k_lap_view_mid", "k_vlap_view_mid", "k_dss_view_final")
PASSES = (7, 13)


def kres(path):
    lines = ["tools/kres.sh  (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; nlev = 72): the kernels of tse_hypervis_view --",
             "the two stage kernels it shares with tse_biharmonic_view / tse_vlaplace_view, k_lap_view_mid, k_vlap_view_mid, k_dss_view_final<ADD>"]
    out = subprocess.run([os.path.join(ROOT, "tools", "kres.sh"), "k_"], stdout=subprocess.PIPE, check=True).stdout.decode()
    lines += [l for l in out.splitlines() if l.startswith(KERNELS)]
    text = "\n".join(lines)
    print(text)
    with open(path, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=30)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kres", default=None)
    args = ap.parse_args()
    if args.kres:
        return kres(args.kres)
    import torch
    if not torch.cuda.is_available():
        sys.exit("hypervis_view_rate: no GPU (rates are measured on the device only)")
    from view_rate import context
    from transport_se_amd import cube_mesh as cm
    hip = context(args.ne, 4)
    geo = cm.geometry(args.ne)
    hip.vector_setup(geo["D"], cm.metinv(geo["D"]), geo["mp"])
    n, K, nf, nu = hip.nelemd, hip.nlev, 3, 2.5
    coef = (-1.1e15, -0.7e15, -0.9e15, -1.3e15)
    nbytes = n * (nf + 2) * K * 16 * 8
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    src_s = 300.0 * (torch.rand((n, nf, K, 4, 4), dtype=torch.float64, device="cuda", generator=gen) + 0.5)
    src_v = 30.0 * (torch.rand((n, 2, K, 4, 4), dtype=torch.float64, device="cuda", generator=gen) - 0.5)
    shape = lambda axes, q, pad: {"eqkji": (n, q, K, 4, 4), "eqjik": (n, q, 4, 4, K + pad), "eqkij": (n, q, K, 4, 4)}[axes]   # noqa: E731
    alloc = lambda axes, q, pad: torch.empty(shape(axes, q, pad), dtype=torch.float64, device="cuda")[..., :K if axes == "eqjik" else None]   # noqa: E731
    dense = lambda t, axes: {"eqkji": t, "eqjik": t.permute(0, 1, 4, 2, 3), "eqkij": t.permute(0, 1, 2, 4, 3)}[axes]   # noqa: E731
    # name -> (axes of s and v, padding of a row of levels)
    layouts = {"point-fastest": ("eqkji", 0), "level-fastest": ("eqjik", 0), "level-fastest, pitch %d" % (K + 3): ("eqjik", 3), "generic [k][i][j]": ("eqkij", 0)}
    st = torch.cuda.Stream()
    fields, kinds = {}, {}
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for name, (sa, pad) in layouts.items():
            f = dict(sa=sa, va=sa)
            for tag in ("fused", "loop"):
                f[tag] = (alloc(sa, nf, pad), alloc(sa, 2, pad))
            f["ten"], f["vten"] = alloc(sa, nf, pad), alloc(sa, 2, pad)
            f["cs"] = torch.tensor(coef[:nf], dtype=torch.float64, device="cuda").reshape(1, nf, 1, 1, 1)   # (q is the second axis of every layout)
            fields[name] = f

            def fused(f=f):
                hip.hypervis_view(f["fused"][0], f["sa"], f["fused"][1], f["va"], coef=coef, nu_ratio=nu, stream=st)

            def loop(f=f):
                s, v = f["loop"]
                hip.biharmonic_view(s, f["sa"], out=f["ten"], order=2, stream=st)
                hip.vlaplace_view(v, f["va"], out=f["vten"], order=2, nu_ratio=nu, stream=st)
                f["ten"].mul_(f["cs"]); f["vten"].mul_(coef[nf])                       # host_scale
                hip.dss_view(f["ten"], f["sa"], mode="weak", stream=st)
                hip.dss_view(f["vten"], f["va"], mode="weak", stream=st)
                s.add_(f["ten"]); v.add_(f["vten"])                                    # host_add
            kinds[(name, "fused")], kinds[(name, "loop")] = fused, loop
        # the bits first: one sub-step of either kind from the same state, in every layout
        ref = None
        for name, f in fields.items():
            for tag in ("fused", "loop"):
                dense(f[tag][0], f["sa"]).copy_(src_s); dense(f[tag][1], f["va"]).copy_(src_v)
                kinds[(name, tag)]()
            st.synchronize()
            got = [dense(f["fused"][0], f["sa"]), dense(f["fused"][1], f["va"])]
            assert not torch.equal(got[0], src_s) and not torch.equal(got[1], src_v)
            assert torch.equal(got[0], dense(f["loop"][0], f["sa"])) and torch.equal(got[1], dense(f["loop"][1], f["va"])), "fused and loop disagree: " + name
            ref = ref or [g.clone() for g in got]
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), "the paths disagree: " + name
        for _ in range(3):   # warm-up of every shape timed below
            for g in kinds.values():
                g()
        st.synchronize()
        times = {k: [] for k in kinds}
        total = {k: 0.0 for k in kinds}
        while min(total.values()) < args.seconds * 1e3:
            evs = []
            for k, g in kinds.items():   # fused, loop, fused, loop, ...
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st); g(); b.record(st)
                evs.append((k, a, b))
            st.synchronize()
            for k, a, b in evs:
                ms = a.elapsed_time(b); times[k].append(ms); total[k] += ms
        # the kernels alone: the "fieldhv" group, 20 calls per layout
        group = {}
        for name in fields:
            hip.timing(True)
            for _ in range(20):
                kinds[(name, "fused")]()
            st.synchronize()
            ms, launches = hip.kernel_time("fieldhv")
            assert launches == 100, launches
            group[name] = ms / 20
        hip.timing(False)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = ["tse_hypervis_view vs the loop it replaces (biharmonic_view, vlaplace_view, product, 2 x dss_view(WEAK), addition; torch does the product "
             "and the addition): ne%d (%d elements), one rank, (%d + 2) x %d levels = %d layers, %.3f GB" % (args.ne, n, nf, K, (nf + 2) * K, nbytes / 1e9),
             "%s, torch %s; device events on a side stream, 3 warm-up rounds, window >= %.1f s of device time per kind; fieldhv: the five kernels "
             "of a call, mean of 20 calls; passes over the fields: fused %d, loop %d" % (torch.cuda.get_device_name(0), torch.__version__, args.seconds, PASSES[0], PASSES[1]),
             "%-24s %-6s %6s %10s %10s %10s %10s %12s %11s" % ("layout", "kind", "calls", "median ms", "mean ms", "min ms", "max ms", "fused / loop", "fieldhv ms")]
    worst = 0.0
    for (name, tag), v in times.items():
        ratio = med[(name, "fused")] / med[(name, "loop")]
        worst = max(worst, ratio)
        lines.append("%-24s %-6s %6d %10.4f %10.4f %10.4f %10.4f %12s %11s" % (
            name, tag, len(v), med[(name, tag)], float(np.mean(v)), min(v), max(v), "%.3f" % ratio if tag == "fused" else "-",
            "%.4f" % group[name] if tag == "fused" else "-"))
    lines.append("condition (the fused call is not slower than the loop on any layout): worst fused / loop = %.3f -> %s" % (worst, "met" if worst <= 1.0 else "NOT MET"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n\n")
    hip.close()


if __name__ == "__main__":
    main()
