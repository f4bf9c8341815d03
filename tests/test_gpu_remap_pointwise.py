"""-m gpu: the PPM vertical remap (k_remap through tse_remap_q_ppm) held output by output to the forward-error bound of
tests/remap_ld.py against longdouble: |got - v| <= (gamma_m + gamma_m(2^-64)) * A * (1 + 2^-40) at every SAFE output (every sign test
that feeds it decided beyond its own rounding error; derivation, counts and the definition of safe: remap_ld.py; the model and the
bound are shown right and sharp on the CPU in test_remap_bound_cpu.py, on these very arrays).

Inputs (remap_ld.inputs): ne 2, 24 elements x 16 columns, a grid family per block of elements (gentle: lockstep loop; squeeze: generic
loop; random; identity: every interface a pio == pin tie; thin: a layer at 1e-3 of its neighbours), a tracer family per slot (sine,
bell, noise, spikes over exact zeros, ramp, sign-changing noise) at slot scalings 2^-200 .. 2^200.
Routes: TSE_REMAP_GENERIC 0 and 1, vert_remap_q_alg 0 and 2, the 72-level library and the 64-level one (each in a child process of its
own), qsize 1, 3, 16, 19, 20, 35 (remap_ld.QSIZES: whole rounds, 1-3 segment-task tracers with the 2^+-200 slots among them, a fourth
leftover in a partly idle round).
* safe outputs: the bound, every one;
* unsafe outputs: at most 1 % per (grid family, tracer family), held to the single-call tolerance of test_gpu_ops_golden.py, 1e-13 of
  the tracer's field maximum;
* column mass, every column: remap_ld.column_mass_ratio (rigorous: the last running mass takes no decision);
* the uniform mixing ratio Q = c*dp1 (c = 0.75, 1, 2^-200) is outside the pointwise claim -- fl(c*dp)/dp differs from cell to cell
  by an ulp, so every decision on it is rounding noise: out/dp2 against c per level at Q_TOL_CYCLES = 5e-13 of
  test_gpu_tracer_invariance.py, the per-level maxima recorded;
* a target grid the bracket search cannot end on comes back as TseError with no kernel launched.
NT = 2, the fused route and vertical_remap's own target grid cannot be reached through the operator call; they are pinned to these
bits by test_gpu_parity.py (test_remap_column_loop_variants, the fused-remap test) and test_gpu_tracer_invariance.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
UNSAFE_TOL = 1e-13       # test_gpu_ops_golden.py: one remap_Q_ppm call, of the field maximum
Q_TOL_CYCLES = 5e-13     # test_gpu_tracer_invariance.py
CAP = 0.01
GENERIC = (0, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# worker side (a child process): one library
def _hip(nlev, qsize, alg):
    import remap_ld as rl
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.driver import partition
    from transport_se_amd.hip_mod import HipMod
    hv = rl.hvcoord(nlev)
    topo = cm.topology(2); geo = cm.geometry(2, topo)
    d = cm.edge_descriptors(topo, partition(2, 1), 0)
    mine = d["elems"]
    elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, 0.0, device=0, vert_remap_q_alg=alg)
    assert h.nlev == nlev and h.nelemd == rl.NELEM
    return h


def _worker(spec):
    import remap_ld as rl
    from transport_se_amd.hip_mod import TseError
    nlev, alg, out = spec["nlev"], spec["alg"], {}
    if spec["kind"] == "pointwise":
        for qsize in rl.QSIZES:
            Q, dp1, dp2 = rl.inputs(nlev, qsize)          # (asserts the precondition)
            h = _hip(nlev, qsize, alg)
            for generic in GENERIC:
                os.environ["TSE_REMAP_GENERIC"] = str(generic)
                out["%d/%d" % (qsize, generic)] = h.remap_q_ppm(Q, dp1, dp2)
            h.close()
    elif spec["kind"] == "uniform":
        Q, dp1, dp2, c = rl.uniform_inputs(nlev)
        h = _hip(nlev, Q.shape[1], alg)
        for generic in GENERIC:
            os.environ["TSE_REMAP_GENERIC"] = str(generic)
            out["%d" % generic] = h.remap_q_ppm(Q, dp1, dp2)
        h.close()
    elif spec["kind"] == "guard":
        Q, dp1, dp2 = rl.inputs(nlev, 3)
        h = _hip(nlev, 3, alg)
        h.timing(True)
        good = h.remap_q_ppm(Q, dp1, dp2)
        n0 = h.kernel_time("remap")[1]
        e, k, j, i = 7, nlev - 2, 2, 3
        bad = dp2.copy(); bad[e, k, j, i] += dp2[e, k + 1, j, i] + 2.0      # the partial sum above the last level passes sum(dp1) + 1
        # the harmless one first: a NaN in dp2 from level 5 on ends every bracket search at once, guard or no guard.  The grids a search
        # cannot end on (negative dp1, the over-long dp2) go only to a library that has just shown, by raising, that it checks its grids
        msgs = []
        for x1, x2 in ((dp1, np.where(np.arange(nlev)[None, :, None, None] == 5, np.nan, dp2)), (-dp1, dp2), (dp1, bad)):
            try:
                h.remap_q_ppm(Q, x1, x2)
                msgs.append("")
                break
            except TseError as ex:
                msgs.append(str(ex))
        msgs += [""] * (3 - len(msgs))
        n1 = h.kernel_time("remap")[1]
        again = h.remap_q_ppm(Q, dp1, dp2)               # the context is still good
        n2 = h.kernel_time("remap")[1]
        h.close()
        out = dict(msgs=np.array(msgs), counts=np.array([n0, n1, n2]), same=np.array(np.array_equal(good, again)),
                   where=np.array([e, 4 * j + i, k]))
    np.savez(spec["out"], **out)


# ---------------------------------------------------------------------------------------------------------------------------
# test side
def _child(spec, tmp_path, timeout=300):
    out = str(tmp_path / ("%s_%d_%d.npz" % (spec["kind"], spec["nlev"], spec["alg"])))
    spec = dict(spec, out=out)
    env = dict(os.environ)
    env.pop("TSE_REMAP_GENERIC", None); env.pop("TSE_REMAP_NT", None); env.pop("TSE_LIB", None)   # the product library of this tree
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(spec)], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    return dict(np.load(out))


def _check(route, qsize, got, Q, t, safe, kid, worst):
    """every safe output within the bound (on failure: where, got, v, A, m, kid there, the number over); unsafe ones at most 1 % per
    family pair and within 1e-13 of the tracer's field maximum; every column's mass.  worst[(kind, family)] = (ratio, qsize, level)"""
    import remap_ld as rl
    from step_ld import ratio
    _, r = ratio(got, t)
    rs = np.where(safe, r, 0.0)
    for kind, fams, ax in (("grid", rl.GRIDS, 0), ("tracer", rl.TRACERS, 1)):
        for f in fams:
            ix = [n for n in range(rs.shape[ax]) if (rl.grid_family(n) if ax == 0 else rl.tracer_family(n)) == f]
            if ix:
                sub = np.take(rs, ix, axis=ax)
                w = float(sub.max())
                lev = int(np.unravel_index(int(np.argmax(sub)), sub.shape)[2])
                if w >= worst.get((kind, f), (-1.0,))[0]:
                    worst[(kind, f)] = (w, qsize, lev)
    if rs.max() > 1.0:
        ix = np.unravel_index(int(np.argmax(rs)), rs.shape)
        e, q, k, j, i = map(int, ix)
        pytest.fail("%s qsize %d: |got - v| / bound = %.3g (m = %d) at element %d (%s), tracer %d (%s), level %d, column %d; got %r, v %r, "
                    "A %r; kid(k) = %d, kid(k-1) = %d; %d safe outputs over, levels %s"
                    % (route, qsize, float(rs.max()), t.m, e, rl.grid_family(e), q, rl.tracer_family(q), k, 4 * j + i, float(got[ix]),
                       float(t.v[ix]), float(t.A[ix]), int(kid[e, k, j, i]), int(kid[e, max(k - 1, 0), j, i]), int((rs > 1).sum()),
                       sorted(set(np.argwhere(rs > 1)[:, 2].tolist()))[:24]))
    for g in rl.GRIDS:
        es = [e for e in range(rl.NELEM) if rl.grid_family(e) == g]
        for f in rl.TRACERS:
            qs = [q for q in range(qsize) if rl.tracer_family(q) == f]
            if qs:
                frac = 1.0 - safe[es][:, qs].mean()
                assert frac <= CAP, (route, qsize, g, f, frac)
    fmax = np.abs(t.v).max(axis=(0, 2, 3, 4)).astype(np.float64)[None, :, None, None, None]
    err = np.where(safe, 0.0, np.abs(got.astype(np.longdouble) - t.v).astype(np.float64))
    assert (err <= UNSAFE_TOL * fmax).all(), (route, qsize, float((err / fmax).max()))
    wm, rm = rl.column_mass_ratio(got, Q, t)
    worst["mass"] = max(worst.get("mass", (0.0,)), (wm, qsize))
    assert wm <= 1.0, (route, qsize, "column mass", wm, np.unravel_index(int(np.argmax(rm)), rm.shape))


@pytest.mark.parametrize("alg", [0, 2])
@pytest.mark.parametrize("nlev", [72, 64])
def test_remap_pointwise(tmp_path, nlev, alg):
    import remap_ld as rl
    from conftest import record_margin
    from step_ld import has_extended_precision
    assert has_extended_precision(), np.finfo(np.longdouble)
    res = _child(dict(kind="pointwise", nlev=nlev, alg=alg), tmp_path)
    worst = {g: {} for g in GENERIC}
    for qsize in rl.QSIZES:
        Q, dp1, dp2 = rl.inputs(nlev, qsize)
        t, safe, kid = rl.remap_q_ppm(Q, dp1, dp2, alg)
        for generic in GENERIC:
            got = res["%d/%d" % (qsize, generic)]
            assert got.shape == Q.shape and np.isfinite(got).all()
            _check("L%d alg%d generic%d" % (nlev, alg, generic), qsize, got, Q, t, safe, kid, worst[generic])
    for generic in GENERIC:
        for key, val in sorted(worst[generic].items(), key=str):
            name = "column mass" if key == "mass" else "%s %s" % key
            record_margin("pointwise remap L%d alg%d generic%d %s" % (nlev, alg, generic, name), val[0], 1.0)
            if key != "mass":   # where the worst output sits (a record of its own, so that the names stay the same from run to run)
                record_margin("pointwise remap L%d alg%d generic%d %s: level of the worst output" % (nlev, alg, generic, name), val[2], nlev - 1)
            print("pointwise remap L%d alg%d generic%d %s: %.4g %s" % (nlev, alg, generic, name, val[0], val[1:]))


@pytest.mark.parametrize("alg", [0, 2])
@pytest.mark.parametrize("nlev", [72, 64])
def test_uniform_mixing_ratio_per_level(tmp_path, nlev, alg):
    """Q = c*dp1 -> out/dp2 against c per level (outside the pointwise claim; Q_TOL_CYCLES), the per-level maxima recorded"""
    import remap_ld as rl
    from conftest import record_margin
    res = _child(dict(kind="uniform", nlev=nlev, alg=alg), tmp_path)
    Q, dp1, dp2, c = rl.uniform_inputs(nlev)
    for generic in GENERIC:
        got = res["%d" % generic]
        rel = np.abs(got / dp2[:, None] / c[None, :, None, None, None] - 1.0)
        per_level = rel.max(axis=(0, 1, 3, 4))
        for k in sorted(set(range(0, nlev, 8)) | set(range(nlev - 8, nlev))):   # the table of DESIGN.md section 5: a record per level
            record_margin("uniform mixing ratio through the remap L%d alg%d generic%d level %d" % (nlev, alg, generic, k), per_level[k],
                          Q_TOL_CYCLES)
        record_margin("uniform mixing ratio through the remap L%d alg%d generic%d worst level" % (nlev, alg, generic), per_level.max(), Q_TOL_CYCLES)
        assert per_level.max() <= Q_TOL_CYCLES, (generic, int(np.argmax(per_level)), float(per_level.max()))


@pytest.mark.parametrize("nlev", [72, 64])
def test_a_bad_target_grid_is_refused_before_any_launch(tmp_path, nlev):
    """dp2 whose partial sum passes sum(dp1) + 1 above the last level, a negative dp1, a NaN in dp2: TseError naming element, column and
    level (the harmless two first), the launch count of kernel_time("remap") unchanged (a good call raises it by one), and the context still works"""
    res = _child(dict(kind="guard", nlev=nlev, alg=0), tmp_path)
    msgs, (n0, n1, n2) = [str(m) for m in res["msgs"]], res["counts"]
    e, p, k = res["where"]
    assert all(m.startswith("tse_remap_q_ppm: ") for m in msgs), msgs
    assert "dp2" in msgs[0] and "element 0, column 0, level 5" in msgs[0], msgs[0]
    assert "dp1" in msgs[1] and "element 0, column 0, level 0" in msgs[1], msgs[1]
    assert "element %d, column %d, level %d" % (e, p, k) in msgs[2] and "partial sum of dp2" in msgs[2], msgs[2]
    assert n0 == 1 and n1 == n0 and n2 == n0 + 1, (n0, n1, n2)
    assert bool(res["same"])


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    _worker(json.loads(sys.argv[2]))
