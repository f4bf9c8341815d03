"""-m gpu: the DCMIP error norms from element partials formed on the device (tse_norm_setup / tse_norm_reference / tse_norm_partials,
PrimRun.norm_reference / norms, bin/preqx's norm line).  The element shares are held to the exact referee of tests/norm_model.py at the
textbook summation bound, their extrema and the snapshot to numpy bit for bit, and -- the point of the fixed order -- they do not change in a
bit with the wave-mates, the level-count build or the partition; the norms meet the golden reference run and the host route
(dcmip_norms on the fetched fields) at the forward bound derived in norm_model.forward_bounds."""
import ctypes as C
import json
import math
import os
import re
import threading

import numpy as np
import pytest

import norm_model as nm
import norms
from transport_se_amd import _lib
from transport_se_amd import cube_mesh as cm
from transport_se_amd import diagnostics as dg
from transport_se_amd.driver import PrimRun, partition
from transport_se_amd.hip_mod import HipMod, TseError
from transport_se_amd.hybvcoord import HvCoord

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VC = os.path.join(ROOT, "tests", "golden", "vcoord")
# steps and viscosities of the small meshes (DCMIP 1-2's vertical motion empties layers at the 1-1 steps: tests/test_gpu_state_q.py)
NU_Q = {2: 1e19, 3: 2e18}
TSTEP = {(2, 1): 1800.0, (2, 2): 600.0, (3, 1): 1200.0, (3, 2): 400.0}


def _same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _weights(run):
    owner, colw, dh = dg.column_weights(run.ne, *run._mesh_latlon, dg.level_heights(run.hv.hyam, run.hv.hybm))
    return owner[run.mine], colw[run.mine], dh


def _check_partials(P, q0, qf, owner, colw, dh, avg, what):
    """entries 0-3 within the element bound of the exact referee, entries 4-7 numpy's over the owned points bit for bit; and every entry the
    model's (tests/norm_model.py adds in the device's order) bit for bit"""
    S, n = nm.exact_element_sums(q0, qf, owner, colw, dh, avg)
    err, bound = np.abs(P[:, :4] - S), nm.element_bound(S, n)
    worst = (err / np.where(bound > 0, bound, 1.0)).max()
    print("%s: worst element-sum error / bound = %.3f" % (what, worst))
    assert (err <= bound).all(), (what, worst)
    model = nm.element_partials(q0, qf, owner, colw, dh, avg)
    assert np.array_equal(P[:, 4:], model[:, 4:]), what      # (numpy's max / min over the owned points)
    assert _same_bits(P[:, :4], model[:, :4]), what           # the documented order


def _partials_case(run, tc):
    """what test 1 asks of one run: at nstep 0 and after 6 steps (two remap cycles)"""
    n, nlev, hip = run.mine.size, run.nlev, run.hip
    tr = 0 if tc == 1 else 1
    owner, colw, dh = _weights(run)
    ps = hip.fetch("ps_v", (n, 4, 4))
    assert _same_bits(ps, np.full_like(ps, run.hv.ps0))                         # ps_v == ps0 in every bit after dcmip_set_initial
    assert hip.device_ptr("qref") == (None, 0)
    avg = run.norm_reference()
    Q1 = run.fetch_q(1)[0]
    q0 = hip.fetch("qref", (n, nlev, 4, 4))
    assert _same_bits(q0, Q1[:, tr]) and hip.device_ptr("qref")[1] == q0.nbytes
    assert _same_bits(q0, hip.fetch("qdp1", (n, run.qsize, nlev, 4, 4))[:, tr] / dg.hybrid_dp(run.hv.hyai, run.hv.hybi, ps))
    sum0 = hip.norm_reference(1, tr)                                            # (a second call overwrites the snapshot with the same field)
    x0 = nm.exact_sum0(q0, owner)
    assert (np.abs(sum0 - x0) <= nm.element_bound(x0, owner.reshape(n, 16).sum(1) * nlev)).all()
    assert _same_bits(sum0, nm.element_sum0(q0, owner)) and avg == nm.model_avg(q0, owner)
    P = hip.norm_partials(1, tr, avg)
    assert not P[:, [0, 2, 4]].any()                                            # nothing has moved yet: exactly 0
    _check_partials(P, q0, Q1[:, tr], owner, colw, dh, avg, "nstep 0")
    np1 = run.run(6)
    Qf = run.fetch_q(np1)[0][:, tr]
    assert _same_bits(hip.fetch("qref", (n, nlev, 4, 4)), q0)                   # the snapshot outlives the state changes
    P = hip.norm_partials(np1, tr, avg)
    assert (P[:, [0, 2, 4]] > 0).any()
    _check_partials(P, q0, Qf, owner, colw, dh, avg, "nstep 6")
    got = run.norms(np1)
    assert got == dg.norms_from_partials(P, run.mine, run.nelem)
    host = dg.dcmip_norms(run.ne, *run._mesh_latlon, q0, Qf, dg.level_heights(run.hv.hyam, run.hv.hybm))
    fb = nm.forward_bounds(q0, Qf, owner, colw, dh, avg)
    for k in ("L1", "L2", "Linf"):
        assert abs(got[k] - host[k]) <= fb[k] * host[k], (k, got[k], host[k], fb[k])
    assert got["q_max"] == host["q_max"] and got["q_min"] == host["q_min"]


@pytest.mark.parametrize("limiter", [8, 0])
@pytest.mark.parametrize("tc", [1, 2])
@pytest.mark.parametrize("ne,qsize", [(2, 4), (3, 5)])
def test_element_partials(ne, qsize, tc, limiter):
    run = PrimRun(ne, qsize, test_case=tc, nu_q=NU_Q[ne], tstep=TSTEP[ne, tc], limiter_option=limiter)
    try:
        _partials_case(run, tc)
    finally:
        run.close()


def _hv(nlev):
    return HvCoord(os.path.join(VC, "12k_top-%dm.ascii" % nlev), os.path.join(VC, "12k_top-%di.ascii" % nlev))


@pytest.mark.parametrize("limiter", [8, 0])
@pytest.mark.parametrize("tc", [1, 2])
@pytest.mark.parametrize("nlev", [64, 80])
def test_element_partials_on_the_64_and_80_level_libraries(nlev, tc, limiter):
    run = PrimRun(2, 4, test_case=tc, nu_q=NU_Q[2], tstep=TSTEP[2, tc], limiter_option=limiter, hvcoord=_hv(nlev))
    try:
        assert run.nlev == nlev and run.hip.L.tse_nlev() == nlev
        _partials_case(run, tc)
    finally:
        run.close()


def _write(hip_rt, ptr, arr):
    arr = np.ascontiguousarray(arr, np.float64)
    assert hip_rt.hipMemcpy(C.c_void_p(ptr), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), C.c_int(1)) == 0


def test_an_elements_partials_do_not_depend_on_its_wave_mates():
    """the other elements' Qdp, ps_v and reference field are overwritten through tse_device_ptr with scaled copies: one element's eight
    numbers keep every bit (and the others' change)"""
    run = PrimRun(3, 5, test_case=1, nu_q=NU_Q[3], tstep=TSTEP[3, 1])
    try:
        hip, n, nlev = run.hip, run.mine.size, run.nlev
        avg = run.norm_reference()
        np1 = run.run(6)
        before = hip.norm_partials(np1, 0, avg)
        rt = C.CDLL("libamdhip64.so")
        for keep in (0, 17, n - 1):
            fields = {"qdp%d" % np1: (n, run.qsize, nlev, 4, 4), "qref": (n, nlev, 4, 4), "ps_v": (n, 4, 4)}
            saved = {k: hip.fetch(k, s) for k, s in fields.items()}
            for (k, x), f in zip(saved.items(), (1.37, 0.81, 0.993)):
                y = x * f; y[keep] = x[keep]
                _write(rt, hip.device_ptr(k)[0], y)
            hip.invalidate_cache()
            after = hip.norm_partials(np1, 0, avg)
            assert _same_bits(after[keep], before[keep]), keep
            others = np.delete(np.arange(n), keep)
            assert (after[others] != before[others]).any()    # (not all of them: an element the tracer has not reached holds zeros)
            for k, x in saved.items():
                _write(rt, hip.device_ptr(k)[0], x)
            hip.invalidate_cache()
        assert _same_bits(hip.norm_partials(np1, 0, avg), before)
    finally:
        run.close()


# ---- rank independence: three contexts on one GPU (stepped as tests/test_gpu_multirank_emulated.py steps them) ----
QSIZE_MR, NU_Q_MR, DT_MR = 3, {2: 1e19, 3: 2e18}, {2: 1800.0, 3: 1200.0}


def _emulated(ne, world):
    """(sum0[nelem], partials at nstep 0 [nelem][8], partials after 6 steps [nelem][8], avg) of DCMIP 1-1 on `world` contexts over
    partition(ne, world); the exchange callback swaps the packed slots between the contexts with hipMemcpy"""
    hv = HvCoord()
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    nelem = 6 * ne * ne
    own_rank = partition(ne, world)
    descs = [cm.edge_descriptors(topo, own_rank, r) for r in range(world)]
    owner, colw, dh = dg.column_weights(ne, geo["lat"], geo["lon"], dg.level_heights(hv.hyam, hv.hybm))
    ncol = int(owner.sum())
    rt = C.CDLL("libamdhip64.so")
    barrier = threading.Barrier(world)
    bufs, lens, errors = [None] * world, [dict() for _ in range(world)], []
    sum0 = np.zeros(nelem); P0 = np.zeros((nelem, 8)); P6 = np.zeros((nelem, 8)); avgs = [None] * world

    class Exchange:
        def __init__(self, r):
            self.r = r
            lens[r][0] = ([s[2] for s in descs[r]["send"]], [s[2] for s in descs[r]["recv"]])

        def set_minmax_layout(self, send_len, recv_len):
            lens[self.r][1] = ([int(x) for x in send_len], [int(x) for x in recv_len])

        def __call__(self, sbuf, rbuf, nlyr, kind):
            r = self.r; d = descs[r]
            bufs[r] = (sbuf, nlyr)
            barrier.wait()
            roff = np.concatenate([[0], np.cumsum(lens[r][kind][1])]).astype(int)
            for i, (peer, _, _) in enumerate(d["recv"]):
                j = [k for k, s in enumerate(descs[peer]["send"]) if s[0] == r][0]
                soff = np.concatenate([[0], np.cumsum(lens[peer][kind][0])]).astype(int)
                ln = lens[r][kind][1][i]
                assert lens[peer][kind][0][j] == ln and bufs[peer][1] == nlyr
                rc = rt.hipMemcpy(C.c_void_p(rbuf + int(roff[i]) * nlyr * 8), C.c_void_p(bufs[peer][0] + int(soff[j]) * nlyr * 8),
                                  C.c_size_t(ln * nlyr * 8), C.c_int(3))
                assert rc == 0
            assert rt.hipDeviceSynchronize() == 0
            barrier.wait()
            return 0

    def worker(r):
        try:
            d = descs[r]; mine = d["elems"]
            elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                        rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
            h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), QSIZE_MR, NU_Q_MR[ne], device=0,
                       schedule=dict(send=d["send"], recv=d["recv"]), exchange=Exchange(r) if world > 1 else None)
            h.dcmip_init(1, geo["lat"][mine], geo["lon"][mine], hv.hyam, hv.hybm)
            h.dcmip_set_initial()
            h.norm_setup(owner[mine], colw[mine], dh)
            sum0[mine] = h.norm_reference(1, 0)
            barrier.wait()                                              # every rank's element sums are in
            avgs[r] = math.fsum(sum0.tolist()) / (hv.nlev * ncol)       # (what rank 0 forms and broadcasts in PrimRun.norm_reference)
            P0[mine] = h.norm_partials(1, 0, avgs[r])
            assert h.prim_run_subcycle(DT_MR[ne], 2, 0) == 6
            P6[mine] = h.norm_partials(1, 0, avgs[r])                   # the sixth step wrote time level 1 (TimeLevel_Qdp, time_mod.F90:85-109)
            h.close()
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)
            try:
                barrier.abort()
            except Exception:  # noqa: BLE001
                pass

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=240)
    assert not errors, errors
    assert len(set(avgs)) == 1
    return sum0, P0, P6, avgs[0], np.bincount(own_rank, minlength=world)


@pytest.mark.parametrize("ne,split", [(3, (18, 18, 18)), (2, (8, 8, 8))])
def test_partials_and_norms_do_not_depend_on_the_partition(ne, split):
    """three contexts over partition(ne, 3) against one context: the union of the element partials has the same bits, hence
    norms_from_partials gives the same five doubles"""
    one = _emulated(ne, 1)
    three = _emulated(ne, 3)
    assert tuple(three[4]) == split
    for a, b in zip(one[:3], three[:3]):
        assert _same_bits(a, b)
    assert one[3] == three[3]
    assert (one[2][:, [0, 2, 4]] > 0).any()
    gid, nelem = np.arange(6 * ne * ne), 6 * ne * ne
    n1, n3 = dg.norms_from_partials(one[2], gid, nelem), dg.norms_from_partials(three[2], gid, nelem)
    assert n1 == n3 and 0 < n1["L2"] < 2
    # (the exact sum does not care in what order the elements arrive)
    perm = np.random.default_rng(3).permutation(nelem)
    assert dg.norms_from_partials(three[2][perm], gid, nelem) == n1


def test_norms_meet_the_reference_run_and_the_host_route_at_ne8():
    """DCMIP 1-2 at ne8 for one day (the config and 216 steps of tests/golden/ref_ne8_norms.json)"""
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_ne8_norms.json")))["dcmip1-2"]
    cfg = ref["config"]
    assert cfg["nsteps"] == 216 and cfg["ne"] == 8
    run = PrimRun(cfg["ne"], cfg["qsize"], test_case=cfg["test"], nu_q=cfg["nu_q"], tstep=cfg["tstep"])
    try:
        tr = cfg["tracer"] - 1
        qdp0 = run.fetch_qdp(1)[:, tr].copy()
        avg = run.norm_reference()
        np1 = run.run(cfg["nsteps"])
        got = run.norms(np1)
        print("ne8 DCMIP 1-2 from element partials:", got)
        for k in ("L1", "L2", "Linf", "q_max"):
            assert abs(got[k] - ref[k]) <= 1e-6 * abs(ref[k]), (k, got[k], ref[k])
        assert abs(got["q_min"] - ref["q_min"]) < 1e-9
        qdp1 = run.fetch_qdp(np1)[:, tr]
        ps_v = run.hip.fetch("ps_v", (run.nelem, 4, 4))
        hv = run.hv
        host = norms.dcmip_norms_from_qdp(cfg["ne"], run.lat, run.lon, qdp0, qdp1, ps_v, hv.hyai, hv.hybi, hv.hyam, hv.hybm)
        owner, colw, dh = _weights(run)
        q0 = qdp0 / norms.hybrid_dp(hv.hyai, hv.hybi, np.full_like(ps_v, norms.P0)); qf = qdp1 / norms.hybrid_dp(hv.hyai, hv.hybi, ps_v)
        fb = nm.forward_bounds(q0, qf, owner, colw, dh, avg)
        for k in ("L1", "L2", "Linf"):
            rel = abs(got[k] - host[k]) / host[k]
            print("  %s: host route %.17g, relative difference %.3e, bound %.3e" % (k, host[k], rel, fb[k]))
            assert rel <= fb[k], (k, got[k], host[k], fb[k])
        assert got["q_max"] == host["q_max"] and got["q_min"] == host["q_min"]
    finally:
        run.close()


def test_misuse_is_refused_with_a_message_and_launches_nothing(monkeypatch):
    monkeypatch.setenv("TSE_LIB", _lib.HOOKS_SO)    # the twin with the tests' fault injection: same sources, same kernels
    monkeypatch.setenv("TSE_TEST_FAIL_NORM_ALLOC", "1")
    run = PrimRun(2, 4, test_case=1, nu_q=NU_Q[2], tstep=TSTEP[2, 1])
    try:
        hip, n = run.hip, run.mine.size
        hip.timing(True)
        owner, colw, dh = _weights(run)

        def refused(call, *words):
            with pytest.raises(TseError) as ex:
                call()
            assert all(w in str(ex.value) for w in words), str(ex.value)

        refused(lambda: hip.norm_reference(1, 0), "tse_norm_reference", "tse_norm_setup first")
        refused(lambda: hip.norm_partials(1, 0, 0.5), "tse_norm_partials", "tse_norm_setup first")
        hip.norm_setup(owner, colw, dh)
        refused(lambda: hip.norm_partials(1, 0, 0.5), "tse_norm_reference first")
        refused(lambda: hip.norm_reference(1, 0), "cannot allocate", "GB of device memory")     # the snapshot's allocation fails (on request)
        refused(lambda: hip.norm_partials(1, 0, 0.5), "tse_norm_reference first")                  # ... and leaves no reference behind
        assert hip.device_ptr("qref") == (None, 0)
        assert hip.kernel_time("norms") == (0.0, 0)
        monkeypatch.delenv("TSE_TEST_FAIL_NORM_ALLOC")
        hip.norm_reference(1, 0)
        assert hip.kernel_time("norms")[1] == 1
        for q in (-1, 4):
            refused(lambda: hip.norm_reference(1, q), "tracer q=%d" % q)
            refused(lambda: hip.norm_partials(1, q, 0.5), "tracer q=%d" % q)
        for nt in (0, 3):
            refused(lambda: hip.norm_reference(nt, 0), "nt=%d" % nt)
            refused(lambda: hip.norm_partials(nt, 0, 0.5), "nt=%d" % nt)
        with pytest.raises(TseError):
            hip.norm_setup(owner[:-1], colw, dh)
        assert hip.kernel_time("norms")[1] == 1      # none of the refused calls launched anything
        P = hip.norm_partials(1, 0, 0.5)
        ms, launches = hip.kernel_time("norms")
        assert launches == 2 and ms > 0 and np.isfinite(P[:, :6]).all()
    finally:
        run.close()


# ---- bin/preqx ----
def _norm_line(out, tc):
    lines = [l for l in out.splitlines() if l.startswith("DCMIP 1-%d:" % tc)]
    assert len(lines) == 1, out[-2000:]
    return lines[0]


@pytest.mark.parametrize("tc", [1, 2])
def test_preqx_prints_the_host_routes_digits_on_1_and_2_ranks(tmp_path, tc):
    """the namelist of tests/test_prim_main.py at ne2, six tracer steps: the `DCMIP 1-x:` line is the same string on 1 rank and on 2 staged
    ranks, and its values are dcmip_norms' on the fetched state, to the printed digits"""
    from test_prim_main import NL, _run_preqx
    nl = NL.replace("ne = 8", "ne = 2").replace('test_case = "dcmip1-1"', 'test_case = "dcmip1-%d"' % tc)
    assert "ne = 2" in nl and "dcmip1-%d" % tc in nl
    one = _norm_line(_run_preqx([], nl, tmp_path), tc)
    two = _norm_line(_run_preqx(["--gpus", "2"], nl, tmp_path, {"TSE_EXCHANGE": "staged"}), tc)
    assert one == two
    run = PrimRun(2, 4, test_case=tc, nu_q=6e16, tstep=400.0, rsplit=3, limiter_option=8)
    try:
        tr = tc - 1
        qdp0 = run.fetch_qdp(1)[:, tr].copy()
        np1 = run.run(6)
        hv = run.hv
        host = norms.dcmip_norms_from_qdp(2, run.lat, run.lon, qdp0, run.fetch_qdp(np1)[:, tr], run.hip.fetch("ps_v", (run.nelem, 4, 4)),
                                          hv.hyai, hv.hybi, hv.hyam, hv.hybm)
    finally:
        run.close()
    want = "DCMIP 1-%d: L1=%8.6f L2=%8.6f Linf=%8.6f q_max=%8.6f q_min=%14.6e" % (tc, host["L1"], host["L2"], host["Linf"], host["q_max"], host["q_min"])
    assert one == want
    got = {k: float(v) for k, v in re.findall(r"(\w+)=\s*([-+0-9.eE]+)", one.split(":", 1)[1])}
    assert got["L1"] > 0 and got["L2"] > 0
