#!/usr/bin/env python3
"""Time of tse_remap_view on each path of its field view against the library's own remap kernel on the same shape.

  python tools/remap_view_rate.py [--ne 30] [--qsize 35] [--seconds 1.0] [--out FILE]

The state is the prescribed case after one tracer step.  The field is a copy of Qdp in the host's layout; dp_src is the library's dp3d of
that step (dp - dt * divdp_proj, the floating levels), dp_tgt the reference levels at its surface pressure -- the two grids
tse_vertical_remap forms for itself, so both remaps move every interface by the same fraction of a layer.  Timed, interleaved in one loop
after warm-up:
  view <layout>   hip.remap_view(field, ..., stream=s): the check kernel and k_remap_view, between two device events on the side stream s;
  k_remap         hip.vertical_remap(dt, 2): the same arithmetic on the library's dense layout with its lockstep column loop and the
                  bounds emission, by the library's own timer group "remap" (events on the compute stream around the launch).
The "fieldremap" timer group (the two launches alone, without the stream hand-over) is printed as well.  GB/s counts two field passes.
The table goes to stdout and, with --out, is appended to FILE (profiles/remap_view_rate.txt holds a record).  Needs the GPU."""
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
    ap.add_argument("--qsize", type=int, default=35)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("remap_view_rate: no GPU (times are measured on the device only)")
    from forcing_rate import context
    from transport_se_amd.driver import TSTEP
    from transport_se_amd.hybvcoord import HvCoord
    hip = context(args.ne, args.qsize)
    n, qs, K = hip.nelemd, hip.qsize, hip.nlev
    nbytes = n * qs * K * 16 * 8
    tstep = TSTEP.get(args.ne, 300.0 * 30.0 / args.ne)
    dt = 3 * tstep
    hip.dcmip_step_inputs(0, tstep); hip.advec_tracers_remap_rk2(tstep, 1, 2)
    hip.vertical_remap(dt, 2)                                       # leaves dp3d = dp - dt * divdp_proj
    hv = HvCoord()
    f64 = dict(dtype=torch.float64, device="cuda")
    src = torch.empty((n, K, 4, 4), **f64)
    hip.get("dp3d", src, "ekji")
    dA = torch.tensor(np.diff(hv.hyai), **f64)[None, :, None, None]
    dB = torch.tensor(np.diff(hv.hybi), **f64)[None, :, None, None]
    ps = hv.hyai[0] * hv.ps0 + src.sum(dim=1, keepdim=True)
    tgt = dA * hv.ps0 + dB * ps
    q0 = torch.empty((n, qs, K, 4, 4), **f64)
    hip.get("qdp", q0, "eqkji", nt=2)
    pad = torch.empty((n, qs, 4, 4, K + 3), **f64)
    fields = {   # name: (array, axes, path)
        "point-fastest": (q0.clone(), "eqkji", 0),
        "level-fastest": (q0.permute(0, 1, 3, 4, 2).contiguous(), "eqjik", 1),
        "level-fastest, rows + 3": (pad[..., :K], "eqjik", 1),
        "j/i swapped": (q0.permute(0, 1, 2, 4, 3).contiguous(), "eqkij", 2),
    }
    pad[..., :K] = q0.permute(0, 1, 3, 4, 2)
    grids = {"point-fastest": (src, tgt, "ekji"), "level-fastest": (src.permute(0, 2, 3, 1).contiguous(), tgt.permute(0, 2, 3, 1).contiguous(), "ejik")}
    s = torch.cuda.Stream()

    def view(name, mode="mass", grid="point-fastest"):
        f, axes, _ = fields[name]
        a, b, gaxes = grids[grid]
        return lambda: hip.remap_view(f, axes, a, gaxes, b, gaxes, mode=mode, stream=s)
    kinds = {"view " + name: view(name) for name in fields}
    kinds["view level-fastest, grids too"] = view("level-fastest", grid="level-fastest")
    mean = q0 / src[:, None]
    fields["mean"] = (mean, "eqkji", 0)
    kinds["view point-fastest, mean"] = view("mean", mode="mean")
    torch.cuda.synchronize()
    # the bits first: every layout leaves what the point-fastest one leaves
    outs = {}
    for name in ("point-fastest", "level-fastest", "level-fastest, rows + 3", "j/i swapped"):
        f, axes, _ = fields[name]
        keep = f.clone()
        torch.cuda.synchronize()   # (without a stream the call is not ordered behind torch's work)
        assert hip.remap_view(f, axes, src, "ekji", tgt, "ekji") == 0, hip.last_error()
        outs[name] = f.permute(*[axes.index(c) for c in "eqkji"]).clone(memory_format=torch.contiguous_format).view(torch.int64)
        assert torch.equal(outs[name], outs["point-fastest"]), name
        f.copy_(keep)
    del outs, keep
    hip.timing(True)
    with torch.cuda.stream(s):
        for _ in range(3):
            for f in kinds.values():
                f()
            hip.vertical_remap(dt, 2)
        s.synchronize(); hip.synchronize()
        hip.timing(True)   # (reset)
        times = {k: [] for k in kinds}
        total = {k: 0.0 for k in kinds}
        while min(total.values()) < args.seconds * 1e3:
            evs = []
            for k, f in kinds.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s); f(); b.record(s)
                evs.append((k, a, b))
            hip.vertical_remap(dt, 2)
            s.synchronize(); hip.synchronize()
            for k, a, b in evs:
                ms = a.elapsed_time(b); times[k].append(ms); total[k] += ms
    assert hip.remap_view_status() == (0, None)
    rm_ms, rm_n = hip.kernel_time("remap")
    fr_ms, fr_n = hip.kernel_time("fieldremap")
    hip.timing(False)
    dense = rm_ms / rm_n
    lines = ["tse_remap_view vs k_remap (tse_vertical_remap): ne%d (%d elements), %d fields / tracers, %d levels, %.3f GB per field set"
             % (args.ne, n, qs, K, nbytes / 1e9),
             "%s, torch %s; device events on a side stream, 3 warm-up rounds, window >= %.1f s of device time per kind"
             % (torch.cuda.get_device_name(0), torch.__version__, args.seconds),
             "%-34s %6s %10s %10s %10s %12s %10s" % ("kind", "calls", "mean ms", "min ms", "max ms", "GB/s (2 x)", "x k_remap")]
    for k, v in times.items():
        m = float(np.mean(v))
        lines.append("%-34s %6d %10.4f %10.4f %10.4f %12.1f %10.3f" % (k, len(v), m, min(v), max(v), 2 * nbytes / m / 1e6, m / dense))
    lines.append("%-34s %6d %10.4f %10s %10s %12.1f %10.3f" % ("k_remap (timer group \"remap\")", rm_n, dense, "", "", 2 * nbytes / dense / 1e6, 1.0))
    lines.append("timer group \"fieldremap\": %.4f ms per call over %d calls of all kinds (check kernel + remap kernel, no stream hand-over)" % (fr_ms / fr_n, fr_n))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n\n")
    hip.close()


if __name__ == "__main__":
    main()
