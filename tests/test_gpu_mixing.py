"""-m gpu: the mixing and filament diagnostics formed on the device (tse_mix_partials, PrimRun.mixing_reference / mixing, bin/preqx --mixing).
Every entry of an element's share is held to tests/mixing_model.py -- the device's algorithm and order of addition in numpy -- bit for bit, on
synthetic (chi, xi) fields that cover every class boundary and every path of the distance, on the 72-, 64- and 80-level libraries; the rows do
not change in a bit with the element order or the partition; a DCMIP 1-1 run meets the host route on the fetched fields at the summation bound;
misuse is refused before anything is launched; bin/preqx prints the same digits on 1 and 2 ranks."""
import ctypes as C
import os

import numpy as np
import pytest

import mixing_model as mm
from transport_se_amd import cube_mesh as cm
from transport_se_amd import diagnostics as dg
from transport_se_amd.driver import PrimRun, partition
from transport_se_amd.hip_mod import HipMod, TseError
from transport_se_amd.hybvcoord import HvCoord

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VC = os.path.join(ROOT, "tests", "golden", "vcoord")
NE, QSIZE, NU_Q, TSTEP = 2, 4, 1e19, 1800.0
QA, QB = 2, 1                                   # (not the defaults 0, 1: the tracer arguments are used)
TAU = np.array(dg.MIX_TAU)
TAU24 = np.linspace(-0.5, 0.95, 24)             # the most thresholds a call takes, some of them below xmin
PARS = {"dcmip": ((0.0, 1.0, 0.9, -0.8), TAU), "negative xmin": ((-0.6, 1.0, 0.9, -0.8), TAU24)}


def _hv(nlev):
    return HvCoord() if nlev == 72 else HvCoord(os.path.join(VC, "12k_top-%dm.ascii" % nlev), os.path.join(VC, "12k_top-%di.ascii" % nlev))


def _same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _weights(ne, hv):
    geo = cm.geometry(ne)
    return dg.column_weights(ne, geo["lat"], geo["lon"], dg.level_heights(hv.hyam, hv.hybm))


def _write(ptr, arr):
    arr = np.ascontiguousarray(arr, np.float64)
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(ptr), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), C.c_int(1)) == 0


def realize(x, dp):
    """Qdp with fl(Qdp / dp) == x wherever one exists within three ulps of x*dp (the device forms Q = Qdp/dp: a family that needs an exact
    value -- on the chord, on an edge, on a threshold -- keeps it at such points), x*dp elsewhere"""
    q = x * dp
    best, ok = q.copy(), q / dp == x
    for step in (1, -1, 2, -2, 3, -3):
        c = q.copy()
        for _ in range(abs(step)):
            c = np.nextafter(c, np.inf if step > 0 else -np.inf)
        hit = ~ok & (c / dp == x)
        best[hit] = c[hit]; ok |= hit
    return best


def synthetic_qdp(hv, par, tau, nelem, seed, ps0):
    """(qdp_a, qdp_b, chi, xi): the two tracer fields to upload and the mixing ratios the device will form from them (ps_v = ps0)"""
    m = mm.constants(*par)
    chi, xi = mm.synthetic_fields(m, tau, nelem, hv.nlev, np.random.default_rng(seed))
    dp = dg.hybrid_dp(hv.hyai, hv.hybi, np.full((nelem, 4, 4), ps0))
    qa, qb = realize(chi, dp), realize(xi, dp)
    return qa, qb, qa / dp, qb / dp


def _upload(hip, qa, qb, tl=1):
    n = hip.nelemd
    qdp = hip.fetch("qdp%d" % tl, (n, hip.qsize, hip.nlev, 4, 4)).copy()
    qdp[:, QA] = qa; qdp[:, QB] = qb
    _write(hip.device_ptr("qdp%d" % tl)[0], qdp)
    hip.invalidate_cache()


def _families_survive_the_division(m, tau, chi, xi, owner):
    """the exact families are still exact in what the device forms, at owned points"""
    own = np.broadcast_to(owner[:, None] != 0, chi.shape)
    x, y = chi[own], xi[own]
    chord = m["yhi"] + (x - m["xmin"]) * m["sl"]
    curve = m["c0"] + m["c2"] * (x * x)
    inx = (x > m["xmin"]) & (x < m["xmax"])
    assert (inx & (y == chord)).sum() >= 20 and (inx & (y == curve)).sum() >= 20
    for edge in (x == m["xmin"], x == m["xmax"], y == m["ylo"], y == m["yhi"]):
        assert edge.sum() >= 20
    for cx in (m["xmin"], m["xmax"]):
        for cy in (m["ylo"], m["yhi"]):
            assert ((x == cx) & (y == cy)).any(), (cx, cy)
    assert (x < m["xmin"]).any() and (x > m["xmax"]).any() and (y < m["ylo"]).any() and (y > np.maximum(curve, m["yhi"])).any()
    assert all((x == t).any() for t in tau)
    P = mm.cubic(m, x, y)[0]
    sc = mm.sign_changes(m, x, y)
    assert (P >= 0).any() and ((P < 0) & (sc == 1)).any()
    A, B, Cc = mm.classes(m, x, y)
    assert min(A.sum(), B.sum(), Cc.sum()) >= 100
    return sc


@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_synthetic_fields_equal_the_model_bit_for_bit(nlev):
    hv = _hv(nlev)
    run = PrimRun(NE, QSIZE, test_case=1, nu_q=NU_Q, tstep=TSTEP, hvcoord=hv)
    try:
        hip, n = run.hip, run.nelem
        assert run.nlev == nlev and hip.L.tse_nlev() == nlev
        ps = hip.fetch("ps_v", (n, 4, 4))
        assert _same_bits(ps, np.full_like(ps, hv.ps0))
        owner, colw, dh = _weights(NE, hv)
        hip.norm_setup(owner, colw, dh)
        for name, (par, tau) in PARS.items():
            m = mm.constants(*par)
            qa, qb, chi, xi = synthetic_qdp(hv, par, tau, n, 100 + nlev, hv.ps0)
            sc = _families_survive_the_division(m, tau, chi, xi, owner)
            if name == "negative xmin":
                assert (sc == 3).sum() >= 100               # three sign changes: only a range with xmin < 0 has them
            _upload(hip, qa, qb)
            Q = run.fetch_q(1)[0]
            assert _same_bits(Q[:, QA], chi) and _same_bits(Q[:, QB], xi)    # the device forms the fields the model is given
            got = hip.mix_partials(1, QA, QB, *par, tau)
            want = mm.element_partials(chi, xi, owner, colw, dh, *par, tau)
            d = np.abs(got - want)
            print("nlev %d, %s: %d of %d entries differ, largest difference %.3e, d_max %.17g" % (nlev, name, (d != 0).sum(), d.size, d.max(), got[:, 7].max()))
            assert got.shape == (n, 32) and _same_bits(got, want), name
            assert (got[:, :8] > 0).all() and not got[:, 8 + tau.size:].any()
            assert got[:, 4:7].sum() == nlev * owner.sum()
    finally:
        run.close()


def test_rows_follow_the_elements_and_do_not_depend_on_the_partition():
    """the elements in another order (fields, owner mask and weights permuted alike) give the same rows in that order; the mesh cut into two
    contexts over partition(ne, 2) gives each context the rows of its elements"""
    hv = _hv(72)
    par, tau = PARS["negative xmin"]
    owner, colw, dh = _weights(NE, hv)
    run = PrimRun(NE, QSIZE, test_case=1, nu_q=NU_Q, tstep=TSTEP)
    try:
        hip, n = run.hip, run.nelem
        qa, qb, chi, xi = synthetic_qdp(hv, par, tau, n, 11, hv.ps0)
        hip.norm_setup(owner, colw, dh)
        _upload(hip, qa, qb)
        base = hip.mix_partials(1, QA, QB, *par, tau)
        assert _same_bits(base, mm.element_partials(chi, xi, owner, colw, dh, *par, tau))
        perm = np.random.default_rng(5).permutation(n)
        hip.norm_setup(owner[perm], colw[perm], dh)
        _upload(hip, qa[perm], qb[perm])
        assert _same_bits(hip.mix_partials(1, QA, QB, *par, tau), base[perm])
        assert (base[perm] != base).any()
    finally:
        run.close()
    topo = cm.topology(NE); geo = cm.geometry(NE, topo)
    own_rank = partition(NE, 2)
    seen = np.zeros(n, bool)
    for r in range(2):
        d = cm.edge_descriptors(topo, own_rank, r)
        mine = d["elems"]
        elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                    rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
        h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), QSIZE, NU_Q, device=0, schedule=dict(send=d["send"], recv=d["recv"]),
                   exchange=lambda *a: 1)      # (never entered: nothing here steps)
        try:
            assert 0 < mine.size < n
            _write(h.device_ptr("ps_v")[0], np.full((mine.size, 4, 4), hv.ps0))
            qdp = np.zeros((mine.size, QSIZE, hv.nlev, 4, 4)); qdp[:, QA] = qa[mine]; qdp[:, QB] = qb[mine]
            _write(h.device_ptr("qdp2")[0], qdp)
            h.invalidate_cache()
            h.norm_setup(owner[mine], colw[mine], dh)
            assert _same_bits(h.mix_partials(2, QA, QB, *par, tau), base[mine]), r
            seen[mine] = True
        finally:
            h.close()
    assert seen.all()


@pytest.mark.parametrize("limiter", [8, 0])
def test_a_dcmip11_run_meets_the_host_route_at_the_summation_bound(limiter):
    run = PrimRun(NE, QSIZE, test_case=1, nu_q=NU_Q, tstep=TSTEP, limiter_option=limiter)
    try:
        hv = run.hv
        owner, colw, dh = _weights(NE, hv)
        lat, lon = run._mesh_latlon
        zm = dg.level_heights(hv.hyam, hv.hybm)
        Q0 = run.fetch_q(1)[0]
        xmin, xmax = run.mixing_reference()
        assert (xmin, xmax) == (float(Q0[:, 0].min()), float(Q0[:, 0].max())) and xmin == 0.0 and 0.5 < xmax <= 1.0
        t0 = run.mixing(1)
        print("limiter %d, t0: %s" % (limiter, t0))
        assert 0 <= t0["l_r"] + t0["l_u"] + t0["l_o"] <= 1e-14 and t0["d_max"] <= 1e-14
        reached = TAU <= xmax
        assert reached.sum() >= 10 and t0["l_f"] == [100.0 if r else 0.0 for r in reached]
        np1 = run.run(6)
        Q = run.fetch_q(np1)[0]
        got = run.mixing(np1)
        host = dg.mixing_diagnostics(NE, lat, lon, Q[:, 0], Q[:, 1], zm, xmin, xmax, 0.9, -0.8, TAU, chi0=Q0[:, 0])
        print("limiter %d, nstep 6: device %s\n  host %s" % (limiter, got, host))
        sb = mm.summation_bounds(owner, run.nlev)
        for k in ("l_r", "l_u", "l_o"):
            assert abs(got[k] - host[k]) <= sb["l"] * host[k], (k, got[k], host[k])
        assert got["l_r"] + got["l_u"] + got["l_o"] > 1e-8            # six steps of deformation and diffusion do mix
        for a, b in zip(got["l_f"], host["l_f"]):
            assert abs(a - b) <= sb["l_f"] * b
        assert got["counts"] == host["counts"] and got["d_max"] == host["d_max"]
        # ... and the element shares behind it are the model's, bit for bit
        P = run.hip.mix_partials(np1, 0, 1, xmin, xmax, 0.9, -0.8, TAU)
        assert _same_bits(P, mm.element_partials(Q[:, 0], Q[:, 1], owner, colw, dh, xmin, xmax, 0.9, -0.8, TAU))
    finally:
        run.close()


def test_misuse_is_refused_with_a_message_and_launches_nothing():
    run = PrimRun(NE, QSIZE, test_case=1, nu_q=NU_Q, tstep=TSTEP)
    try:
        hip = run.hip
        hip.timing(True)
        owner, colw, dh = _weights(NE, run.hv)
        good = (1, 0, 1, 0.0, 1.0, 0.9, -0.8)

        def refused(call, *words):
            with pytest.raises(TseError) as ex:
                call()
            assert all(w in str(ex.value) for w in ("tse_mix_partials",) + words), str(ex.value)

        def raw(*args):
            rc = hip.L.tse_mix_partials(hip.h, *args)
            return rc, hip.L.tse_last_error().decode()

        refused(lambda: hip.mix_partials(*good, TAU), "tse_norm_setup first")
        with pytest.raises(RuntimeError, match="mixing_reference first"):
            run.mixing(1)
        hip.norm_setup(owner, colw, dh)
        for nt in (0, 3):
            refused(lambda: hip.mix_partials(nt, *good[1:], TAU), "nt=%d" % nt)
        for q in (-1, QSIZE):
            refused(lambda: hip.mix_partials(1, q, 1, *good[3:], TAU), "tracer q=%d" % q)
            refused(lambda: hip.mix_partials(1, 0, q, *good[3:], TAU), "tracer q=%d" % q)
        refused(lambda: hip.mix_partials(1, 0, 1, 0.5, 0.5, 0.9, -0.8, TAU), "xmax=", "<= xmin=")
        refused(lambda: hip.mix_partials(1, 0, 1, 0.5, 0.25, 0.9, -0.8, TAU), "xmax=", "<= xmin=")
        for c2 in (0.0, 0.8):
            refused(lambda: hip.mix_partials(1, 0, 1, 0.0, 1.0, 0.9, c2, TAU), "c2=", "c2 < 0")
        refused(lambda: hip.mix_partials(*good, np.linspace(0.0, 1.0, 25)), "ntau=25")
        out = np.empty((hip.nelemd, 32))
        vp = out.ctypes.data_as(C.c_void_p)
        rc, msg = raw(*good, None, -1, vp)
        assert rc != 0 and "ntau=-1" in msg
        rc, msg = raw(*good, None, 3, vp)
        assert rc != 0 and "null argument" in msg
        rc, msg = raw(*good, TAU.ctypes.data_as(C.c_void_p), TAU.size, None)
        assert rc != 0 and "tse_mix_partials" in msg and "null argument" in msg
        assert hip.kernel_time("mixing") == (0.0, 0)        # none of the refused calls launched anything
        P = hip.mix_partials(*good)                         # (no thresholds is a valid call)
        ms, launches = hip.kernel_time("mixing")
        assert launches == 1 and ms > 0 and np.isfinite(P).all() and not P[:, 8:].any() and (P[:, 3] > 0).all()
    finally:
        run.close()


def test_preqx_mixing_prints_the_same_digits_on_1_and_2_ranks(tmp_path):
    """the namelist of tests/test_prim_main.py at ne2, six tracer steps: the mixing and filament lines (after the cycle nearest to the middle
    of the run and at its end) are the same strings on 1 rank and on 2 staged ranks; without --mixing there is no such line and every other
    line is what it is with it"""
    from test_prim_main import NL, _run_preqx
    nl = NL.replace("ne = 8", "ne = 2")
    assert "ne = 2" in nl

    def pick(out):
        return [l for l in out.splitlines() if l.startswith(("mixing", "filament"))]

    def rest(out):
        return [l for l in out.splitlines() if not l.startswith(("mixing", "filament", "prim_run wall"))]
    one = _run_preqx(["--mixing"], nl, tmp_path)
    lines = pick(one)
    assert [l.split(":")[0] for l in lines] == ["mixing   nstep=3", "filament nstep=3", "mixing   nstep=6", "filament nstep=6"], one[-2000:]
    two = _run_preqx(["--gpus", "2", "--mixing"], nl, tmp_path, {"TSE_EXCHANGE": "staged"})
    assert pick(two) == lines
    plain = _run_preqx([], nl, tmp_path)
    assert pick(plain) == [] and rest(plain) == rest(one)
    for l in lines[::2]:
        v = [float(x.split("=")[1]) for x in l.split(":")[1].split()]
        assert len(v) == 3 and min(v) >= 0 and sum(v) > 0
    for l in lines[1::2]:
        v = [float(x.split("=")[1]) for x in l.split(":")[1].split()]
        assert len(v) == TAU.size and min(v) >= 0 and max(v) > 50
