"""-m gpu: tracer transport without a limiter (limiter_option = 0), on every route of the library.

The checker applies limiter 8; the reference model of the unlimited step is tests/unlimited_model.py (the checker's pieces without the
limiter line; test_unlimited_cpu.py shows it is the checker's euler_step once the limiter is put back).  Here:
* against the model: every stage of the per-stage API (ne2, ne4), the whole-step call and two prim_run_subcycle cycles (q_err bounds of
  test_gpu_tracer_invariance.py);
* exact: the outputs that do not depend on tracers equal a limited run's; slot invariance; 2^+-256 scaling; 2 and 3 emulated ranks,
  TSE_BOUNDARY_STRIPS and TSE_REMAP_FUSED=0 equal the one-context default run;
* the limiter is off (a 0/1 field overshoots, superposition holds) and no bounds work runs (no min/max launch, no kind-1 exchange,
  tse_get_qminmax refuses); a limited context after an unlimited one is a limited run;
* ne120/q35 consistency and mass; bin/preqx on a namelist without limiter_option."""
import contextlib
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import pyoracle as po
import unlimited_model as um
from conftest import record_margin
from gpu_common import elem_from_oracle, make_hip
from tracer_fields import BASE_NAMES, NBASE, base_tracers, layer_dp, q_err, slot_bases
from transport_se_amd import cube_mesh as cm
from transport_se_amd.driver import partition
from transport_se_amd.hip_mod import HipMod, TseError
from transport_se_amd.hybvcoord import HvCoord

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_TOL, Q_TOL_CYCLES = 1e-13, 5e-13        # as test_gpu_tracer_invariance.py (see there)
SWITCHES = ("TSE_REMAP_FUSED", "TSE_BOUNDARY_STRIPS", "TSE_DSS_ON_READ")


def _params(ne):
    return (1e19, 1800.0) if ne == 2 else (1e15 * (30.0 / ne) ** 3.2, 300.0 * 30.0 / ne)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@contextlib.contextmanager
def _env(**switches):
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(switches)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check(name, got, ref, dp, tol):
    got, ref, dp = np.array(got), np.array(ref), np.array(dp)
    err, (q, k, e) = q_err(got, ref, dp)
    for i, x in enumerate(err):
        record_margin("q_err unlimited %s %s" % (name, BASE_NAMES[i % NBASE]), x, tol)
    assert np.all(err <= tol), (name, err.tolist(), "worst: tracer %d level %d element %d" % (q, k, e))


def _load(o, elem, hip, b):
    o.qdp[0] = np.moveaxis(b, 0, 1); o.qdp[1] = o.qdp[0]
    elem["Qdp"][...] = np.moveaxis(o.qdp, 0, 1)
    hip.copy_qdp_h2d(elem, 1); hip.copy_qdp_h2d(elem, 2)


def _inputs(o, elem, hip):
    elem["vn0"][...] = o.vn0; elem["dp"][...] = o.dp; elem["eta_dot_dpdn"][...] = o.eta_dot_dpdn; elem["omega_p"][...] = o.omega_p
    hip.set_derived(elem)


@pytest.mark.parametrize("ne", [2, 4])
def test_per_stage_api_vs_model(ne):
    """tse_euler_step (plain unlimited kernels, one DSS pass per stage) after each of the three stages, then tse_qdp_time_avg"""
    nu, dt = _params(ne)
    o = po.Oracle(ne, NBASE, nu_q=nu)
    elem = elem_from_oracle(o)
    hip = make_hip(o, elem, limiter_option=0)
    try:
        o.dcmip_init(1); o.dcmip_step_inputs(1, 0, dt)
        _load(o, elem, hip, base_tracers(o)); _inputs(o, elem, hip)
        hip.compute_divdp()
        for e in range(o.nelem):
            for k in range(72):
                o.divdp[e, k] = o.divergence_sphere(e, o.vn0[e, k])
        o.divdp_proj[...] = o.divdp
        for (np1, n0, dss, rhs) in ((2, 1, 3, 0), (2, 2, 1, 1), (2, 2, 2, 2)):
            um.euler_step(o, np1, n0, dt / 2, dss, rhs)
            hip.euler_step(np1, n0, dt / 2, dss, rhs)
            hip.copy_qdp_d2h(elem, 2)
            _check("ne%d euler_step rhs=%d" % (ne, rhs), elem["Qdp"][:, 1], o.qdp[1], o.dp, Q_TOL)
        o.qdp[1] = (o.qdp[0] + 2.0 * o.qdp[1]) / 3.0
        hip.qdp_time_avg(3, 1, 2)
        hip.copy_qdp_d2h(elem, 2)
        _check("ne%d qdp_time_avg" % ne, elem["Qdp"][:, 1], o.qdp[1], o.dp, Q_TOL)
        with pytest.raises(TseError, match="limiter"):
            hip.get_qminmax()
    finally:
        hip.close(); o.close()


def test_whole_step_and_subcycle_vs_model():
    """tse_advec_tracers_remap_rk2 (DSS on read) x6 + 2 remaps on the model's inputs, and two prim_run_subcycle cycles (fused remap)"""
    nu, dt = _params(2)
    o = po.Oracle(2, NBASE, nu_q=nu)
    elem = elem_from_oracle(o)
    hip = make_hip(o, elem, limiter_option=0)
    try:
        o.dcmip_init(1)
        b = base_tracers(o)
        _load(o, elem, hip, b)
        nstep = 0
        for sub in range(2):
            for r in range(3):
                o.dcmip_step_inputs(1, nstep, dt); _inputs(o, elem, hip)
                n0 = 1 if nstep % 2 == 0 else 2
                hip.advec_tracers_remap_rk2(dt, n0, 3 - n0); um.advec_tracers_remap_rk2(o, dt, nstep)
                if nstep == 0:
                    hip.copy_qdp_d2h(elem, 2)
                    _check("advec_tracers_remap_rk2", elem["Qdp"][:, 1], o.qdp[1], o.dp - dt * o.divdp_proj, Q_TOL)
                nstep += 1
            hip.vertical_remap(3 * dt, 3 - n0); assert o.vertical_remap(3 * dt, 3 - n0) == 0
        hip.copy_qdp_d2h(elem, 1)
        _check("per-step x6 + 2 remaps", elem["Qdp"][:, 0], o.qdp[0], layer_dp(o.hyai, o.hybi, o.ps_v), Q_TOL_CYCLES)
        for fused in ("1", "0"):
            with _env(TSE_REMAP_FUSED=fused):
                hip.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm); hip.dcmip_set_initial()
                o.dcmip_init(1)
                _load(o, elem, hip, b)
                assert hip.prim_run_subcycle(dt, 2, 0) == 6
                assert um.prim_run(o, 1, dt, 2) == (6, 6)
                hip.copy_qdp_d2h(elem, 1)
                _check("prim_run_subcycle x2 fused=%s" % fused, elem["Qdp"][:, 0], o.qdp[0], layer_dp(o.hyai, o.hybi, o.ps_v), Q_TOL_CYCLES)
    finally:
        hip.close(); o.close()


class Run:
    """one context (ne, qsize, limiter_option) on the DCMIP 1-1 device loop"""

    def __init__(self, ne, qsize, limiter_option):
        self.nu, self.dt = _params(ne)
        self.o = po.Oracle(ne, qsize, nu_q=self.nu)
        self.elem = elem_from_oracle(self.o)
        self.hip = make_hip(self.o, self.elem, limiter_option=limiter_option)
        self.shape = (2, self.o.nelem, qsize, 72, 4, 4)

    def close(self):
        self.hip.close(); self.o.close()

    def cycles(self, qdp0, nsub=2, **env):
        o, hip = self.o, self.hip
        with _env(**env):
            hip.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm); hip.dcmip_set_initial()
            self.elem["Qdp"][:, 0] = np.moveaxis(qdp0, 0, 1); self.elem["Qdp"][:, 1] = self.elem["Qdp"][:, 0]
            hip.copy_qdp_h2d(self.elem, 1); hip.copy_qdp_h2d(self.elem, 2)
            assert hip.prim_run_subcycle(self.dt, nsub, 0) == 3 * nsub
            return hip.fetch("qdp", self.shape).copy()

    def step(self, qdp0):
        """one whole tracer step from Qdp = qdp0 on the device winds of step 0 -> Qdp(2)"""
        o, hip = self.o, self.hip
        hip.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm); hip.dcmip_set_initial()
        self.elem["Qdp"][:, 0] = np.moveaxis(qdp0, 0, 1); self.elem["Qdp"][:, 1] = self.elem["Qdp"][:, 0]
        hip.copy_qdp_h2d(self.elem, 1); hip.copy_qdp_h2d(self.elem, 2)
        hip.dcmip_step_inputs(0, self.dt)
        hip.advec_tracers_remap_rk2(self.dt, 1, 2)
        return hip.fetch("qdp", self.shape)[1].copy()


def test_tracer_independent_outputs_equal_a_limited_run():
    """divdp, divdp_proj, eta_dot_dpdn, omega_p, dp3d and ps_v do not depend on the tracers: the same bits with and without the limiter"""
    names = dict(divdp=(72,), divdp_proj=(72,), eta_dot_dpdn=(73,), omega_p=(72,), dp3d=(72,), ps_v=())
    out = {}
    for lim in (8, 0):
        r = Run(2, NBASE, lim)
        try:
            r.cycles(base_tracers(r.o), nsub=1)
            out[lim] = {k: r.hip.fetch(k, (r.o.nelem,) + s + (4, 4)).copy() for k, s in names.items()}
            out[lim]["qdp"] = r.hip.fetch("qdp", r.shape).copy()
        finally:
            r.close()
    for k in names:
        assert np.array_equal(_bits(out[0][k]), _bits(out[8][k])), k
    assert not np.array_equal(out[0]["qdp"], out[8]["qdp"])     # (the tracers themselves do differ)


def test_slot_invariance_and_scaling():
    """every slot holds the bits of its base field's run alone (qsize 1), at qsize 5, 9 and 35; Qdp * 2^+-256 exactly scales"""
    single = []
    r = Run(2, 1, 0)
    try:
        b = base_tracers(r.o)
        single = [r.cycles(b[i:i + 1]) for i in range(NBASE)]
    finally:
        r.close()
    for qsize in (5, 9, 35):
        r = Run(2, qsize, 0)
        try:
            sb = slot_bases(qsize)
            b = base_tracers(r.o)[sb]
            got = r.cycles(b)
            bad = [(s, BASE_NAMES[x]) for s, x in enumerate(sb) if not np.array_equal(_bits(got[:, :, s]), _bits(single[x][:, :, 0]))]
            assert not bad, (qsize, bad)
            if qsize == 35:
                for e in (256, -256):
                    sc = r.cycles(np.ldexp(b, e))
                    assert not np.any((sc != 0) & (np.abs(sc) < np.finfo(np.float64).tiny))
                    assert np.array_equal(_bits(sc), _bits(np.ldexp(got, e))), e
                assert np.array_equal(_bits(r.cycles(b, TSE_REMAP_FUSED="0")), _bits(got))
        finally:
            r.close()


def _emulated(world, ne, qsize, limiter_option, kinds):
    """as test_gpu_multirank_emulated.py: `world` contexts on one GPU exchanging through the callback; returns Qdp(1) of 2 cycles"""
    hv = HvCoord()
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    owner = partition(ne, world)
    descs = [cm.edge_descriptors(topo, owner, r) for r in range(world)]
    hip = C.CDLL("libamdhip64.so")
    barrier = threading.Barrier(world)
    bufs, result, errors = [None] * world, [None] * world, []
    lens = [dict() for _ in range(world)]
    nu, dt = _params(ne)

    class Exchange:
        def __init__(self, r):
            self.r = r
            lens[r][0] = ([s[2] for s in descs[r]["send"]], [s[2] for s in descs[r]["recv"]])

        def set_minmax_layout(self, send_len, recv_len):
            lens[self.r][1] = ([int(x) for x in send_len], [int(x) for x in recv_len])

        def __call__(self, sbuf, rbuf, nlyr, kind):
            r = self.r
            kinds.add(kind)
            bufs[r] = (sbuf, nlyr)
            barrier.wait()
            roff = np.concatenate([[0], np.cumsum(lens[r][kind][1])]).astype(int)
            for i, (peer, _, _) in enumerate(descs[r]["recv"]):
                j = [k for k, s in enumerate(descs[peer]["send"]) if s[0] == r][0]
                soff = np.concatenate([[0], np.cumsum(lens[peer][kind][0])]).astype(int)
                ln = lens[r][kind][1][i]
                assert lens[peer][kind][0][j] == ln and bufs[peer][1] == nlyr
                rc = hip.hipMemcpy(C.c_void_p(rbuf + int(roff[i]) * nlyr * 8), C.c_void_p(bufs[peer][0] + int(soff[j]) * nlyr * 8),
                                   C.c_size_t(ln * nlyr * 8), C.c_int(3))
                assert rc == 0
            assert hip.hipDeviceSynchronize() == 0
            barrier.wait()
            return 0

    def worker(r):
        try:
            d = descs[r]; mine = d["elems"]
            elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine],
                        spheremp=geo["spheremp"][mine], rspheremp=geo["rspheremp"][mine],
                        putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
            h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, nu, limiter_option=limiter_option, device=0,
                       schedule=dict(send=d["send"], recv=d["recv"]), exchange=Exchange(r) if world > 1 else None)
            h.dcmip_init(1, geo["lat"][mine], geo["lon"][mine], hv.hyam, hv.hybm)
            h.dcmip_set_initial()
            assert h.prim_run_subcycle(dt, 2, 0) == 6
            result[r] = (mine, h.fetch("qdp", (2, mine.size, qsize, 72, 4, 4))[0].copy())
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
    q = np.empty((6 * ne * ne, qsize, 72, 4, 4))
    for mine, qq in result:
        q[mine] = qq
    return q


def test_emulated_ranks_and_boundary_strips_equal_one_context():
    """2 and 3 contexts (split boundary/interior launches, callback exchange) = one context, bit for bit; so is TSE_BOUNDARY_STRIPS=1
    on 3; the callback never sees a kind-1 (min/max) exchange"""
    kinds = set()
    with _env():
        one = _emulated(1, 4, 3, 0, kinds)
        assert np.isfinite(one).all() and one.max() > 0
        for world in (2, 3):
            assert np.array_equal(_bits(_emulated(world, 4, 3, 0, kinds)), _bits(one)), world
    with _env(TSE_BOUNDARY_STRIPS="1"):
        assert np.array_equal(_bits(_emulated(3, 4, 3, 0, kinds)), _bits(one))
    assert kinds == {0}, kinds
    lim = set()
    with _env():
        _emulated(2, 4, 3, 8, lim)
    assert lim == {0, 1}                 # (a limited run on the same cut does exchange bounds: the check above is not vacuous)


def _checkerboard(r):
    """Qdp of the reference's 0/1 checkerboard (dcmip_wrapper_mod.F90:215-243; single-valued at ne2) on the device's dp of step 0"""
    o, hip = r.o, r.hip
    hip.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm); hip.dcmip_set_initial(); hip.dcmip_step_inputs(0, r.dt)
    chk = (np.sin(9 * o.lon) * np.sin(9 * o.lat) >= 0).astype(np.float64)
    return chk[:, None] * hip.fetch("dp", (o.nelem, 72, 4, 4))


def test_limiter_is_off_and_no_bounds_work_runs():
    """a 0/1 checkerboard overshoots [0, 1] by more than 1e-3 after one step without the limiter and stays inside with it; the step is
    linear in the tracer; no min/max kernel is launched over a prim_run_subcycle cycle"""
    res = {}
    for lim in (0, 8):
        r = Run(2, 3, lim)
        try:
            b = _checkerboard(r)
            rng = np.random.default_rng(7)
            a1 = base_tracers(r.o)[0] * rng.uniform(0.5, 1.5)
            qd = np.stack([b, a1, b + a1])
            out = r.step(qd)
            Q = out / (r.hip.fetch("dp", (r.o.nelem, 72, 4, 4)) - r.dt * r.hip.fetch("divdp_proj", (r.o.nelem, 72, 4, 4)))[:, None]
            res[lim] = (float(Q[:, 0].min()), float(Q[:, 0].max()))
            if lim == 0:
                lin = np.abs(out[:, 0] + out[:, 1] - out[:, 2]).max() / np.abs(out[:, 2]).max()
                assert lin <= 1e-14, lin
                r.hip.timing(True)
                r.cycles(qd, nsub=1)
                r.hip.synchronize()
                ms, n = r.hip.kernel_time("minmax")
                assert n == 0, (ms, n)
                _, nadv = r.hip.kernel_time("advance0")
                assert nadv > 0
        finally:
            r.close()
    assert res[0][0] < -1e-3 or res[0][1] > 1 + 1e-3, res[0]
    assert res[8][0] >= -1e-12 and res[8][1] <= 1 + 1e-12, res[8]


def test_no_leak_into_a_later_limited_context():
    """a limited context created after an unlimited one in the same process computes what a limited context alone does"""
    r = Run(2, NBASE, 8)
    try:
        ref = r.cycles(base_tracers(r.o), nsub=1)
    finally:
        r.close()
    u = Run(2, NBASE, 0)
    try:
        u.cycles(base_tracers(u.o), nsub=1)
        r = Run(2, NBASE, 8)
        try:
            assert np.array_equal(_bits(r.cycles(base_tracers(r.o), nsub=1)), _bits(ref))
        finally:
            r.close()
    finally:
        u.close()


def _dev_tensor(torch, ptr, shape):
    iface = {"shape": tuple(int(x) for x in shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(type("DevArr", (), {"__cuda_array_interface__": iface})(), device="cuda:0")


def test_ne120_q35_consistency_and_mass():
    """ne120/q35 without the limiter: a tracer with Q == 1 stays 1 through a tracer step (prim_advection_mod.F90:23-33), and the mass of
    every tracer is conserved over one step and a whole rsplit cycle (the DCMIP 1-1 tracers 1-4 made single-valued, as
    test_gpu_baseline_configs.py does for its mass check)"""
    import torch
    from transport_se_amd.driver import PrimRun
    ne, q = 120, 35
    run = PrimRun(ne, q, test_case=1, limiter_option=0)
    hip, n, dt = run.hip, run.nelem, run.tstep
    Q = [_dev_tensor(torch, hip.device_ptr("qdp%d" % tl)[0], (n, q, 72, 16)) for tl in (1, 2)]
    sph = torch.as_tensor(run.elem["spheremp"].reshape(n, 16), device="cuda:0")
    dp = _dev_tensor(torch, hip.device_ptr("dp")[0], (n, 72, 16))
    topo = cm.topology(ne)
    chk = (np.sin(9 * run.lon) * np.sin(9 * run.lat) >= 0).astype(np.float64).reshape(n, 16)
    cons = torch.as_tensor((cm.dss_sum(chk, topo) / cm.dss_sum(np.ones_like(chk), topo) >= 0.5).astype(np.float64), device="cuda:0")
    hip.dcmip_step_inputs(0, dt); hip.synchronize()
    for Qt in Q:
        Qt[:, :q - 1] = (cons[:, None, :] * dp).unsqueeze(1)
        Qt[:, q - 1] = dp
    torch.cuda.synchronize(); hip.invalidate_cache()

    def mass(tl):
        return torch.einsum("ep,eqkp->q", sph, Q[tl - 1]).cpu().numpy()

    m0 = mass(1)
    hip.advec_tracers_remap_rk2(dt, 1, 2); hip.synchronize()
    dvp = _dev_tensor(torch, hip.device_ptr("divdp_proj")[0], (n, 72, 16))
    one = Q[1][:, q - 1] / (dp - dt * dvp)
    assert float((one - 1).abs().max()) <= 1e-12, float((one - 1).abs().max())
    del one
    np.testing.assert_allclose(mass(2), m0, rtol=1e-12)
    run.nstep = 1
    np1 = run.run(2)
    assert run.nstep == 3 and np1 == 2
    hip.synchronize()
    np.testing.assert_allclose(mass(np1), m0, rtol=1e-12)
    run.close()


NL = """
&ctl_nl
  test_case = "dcmip1-1"
  ne = 8
  qsize = 4
  nmax = 6
  statefreq = 3
  tstep = 400
  qsplit = 1, rsplit = 3
  nu_q = 6e16
/
&vert_nl
  vform = "ccm"
/
"""


def test_preqx_runs_a_namelist_without_limiter_option(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    res = subprocess.run([os.path.join(ROOT, "bin", "preqx")], input=NL.encode(), cwd=str(tmp_path), env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600)
    out = res.stdout.decode()
    assert res.returncode == 0, out[-3000:]
    assert "DCMIP 1-1:" in out, out[-2000:]
    lines = [l for l in out.splitlines() if l.startswith("Q") and "relative change" in l]
    assert len(lines) >= 4, out[-2000:]
    for l in lines:
        assert abs(float(l.split("relative change")[1].strip(" )"))) < 1e-11, l
