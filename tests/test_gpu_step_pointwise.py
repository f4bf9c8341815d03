"""-m gpu: the unlimited tracer step (limiter_option = 0) held point by point to the forward-error bound of step_ld.py against longdouble:
|got - v| <= (gamma_m + gamma_m(2^-64)) * A * (1 + 2^-40) at every point, level, tracer and element (derivation and the m of every stage
and route: step_ld.py; the model and the bound are shown right and sharp on CPU in test_step_bound_cpu.py).

Routes:
* per-stage API, one kernel at a time: tse_compute_divdp, tse_euler_step (rhs, DSSopt) = (0, 3), (1, 1), (2, 2), tse_qdp_time_avg(3):
  each stage's reference starts from the device's own fp64 output of the stage before (exact inputs), so each kernel answers to a small
  m of its own;
* the whole step tse_advec_tracers_remap_rk2 from its fp64 inputs, DSS on read (default) and with TSE_DSS_ON_READ=0: Qdp(np1), divdp,
  the DSS'd divdp_proj, eta_dot_dpdn and omega_p; Qdp(n0) bit for bit untouched.
The LIM = false kernels are the templates of the limited path with the limiter code gated off, so the flux divergence, Vstar, dp of a
stage, both Laplacians, the biharmonic scaling, the spheremp weighting and the DSS are pinned for the production path as well.
Also: tse_qdp_time_avg(3) is numpy's (Qn0 + 2*Qnp1)/3 bit for bit; tse_element_mass under its bound (m = 87) at 2^+-200 scalings."""
import contextlib
import os

import numpy as np
import pytest

import pyoracle as po
import step_ld as sl
from conftest import record_margin
from gpu_common import elem_from_oracle
from tracer_fields import base_tracers, slot_bases
from transport_se_amd.hip_mod import HipMod

pytestmark = pytest.mark.gpu
DT = 1800.0
MID = 288                      # DCMIP 1-1 half way (t = 6 days at 1800 s)
STAGES = [(2, 1, 3, 0), (2, 2, 1, 1), (2, 2, 2, 2)]   # (np1, n0, DSSopt, rhs_multiplier)
STILL_NU = 1e20


def _nu(ne):
    return 1e19 if ne == 2 else 1e15 * (30.0 / ne) ** 3.2


@contextlib.contextmanager
def _dss_on_read(on):
    old = os.environ.get("TSE_DSS_ON_READ")
    if on:
        os.environ.pop("TSE_DSS_ON_READ", None)
    else:
        os.environ["TSE_DSS_ON_READ"] = "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("TSE_DSS_ON_READ", None)
        else:
            os.environ["TSE_DSS_ON_READ"] = old


def _tracers(o, family, qsize):
    """Qdp[e][q][k][4][4] of a tracer family on the oracle's dp"""
    n, dp = o.nelem, o.dp
    la, lo = np.asarray(o.lat)[:, None], np.asarray(o.lon)[:, None]
    k = np.arange(72.0)[None, :, None, None]
    rng = np.random.default_rng(1000 + qsize + o.ne)
    Q = np.empty((n, qsize, 72, 4, 4))
    for q in range(qsize):
        if family == "bells":
            la0, lo0 = 0.7 * np.sin(1.3 * q + 0.2), 2.1 * q + 0.5
            r = np.arccos(np.clip(np.sin(la) * np.sin(la0) + np.cos(la) * np.cos(la0) * np.cos(lo - lo0), -1, 1))
            Q[:, q] = 0.1 + np.exp(-(r / 0.6) ** 2) * (1.0 + 0.3 * np.sin(0.21 * k + q))
        elif family == "noise":
            Q[:, q] = rng.uniform(-1.0, 1.0, (n, 72, 4, 4))
        elif family == "halfzero":   # exact zeros over half the sphere, 1e-12 next to them
            Q[:, q] = np.where(np.sin(lo + 0.4 * q) > 0, 0.0, 1e-12 * (1.0 + 0.5 * np.cos(la) * np.cos(0.3 * k + q)))
        else:
            raise ValueError(family)
    return Q * dp[:, None]


def _scaled(o, qsize):
    """base fields in the slots' order (tracer_fields.slot_bases) at power-of-two scalings from 2^-200 to 2^200"""
    b = base_tracers(o, np.random.default_rng(77))
    ex = np.rint(np.linspace(-200, 200, qsize)).astype(int) if qsize > 1 else np.array([-200])
    return np.stack([np.ldexp(b[s], int(e)) for s, e in zip(slot_bases(qsize), ex)], axis=1)


class Ctx:
    """an oracle (geometry, DCMIP inputs) and an unlimited HIP context on the same mesh"""

    def __init__(self, ne, qsize, winds, family, nu=None):
        self.ne, self.qsize, self.nu = ne, qsize, _nu(ne) if nu is None else nu
        o = self.o = po.Oracle(ne, qsize, nu_q=self.nu)
        test, nstep = {"dcmip11-t0": (1, 0), "dcmip11-mid": (1, MID), "dcmip12": (2, 3), "still": (1, 0)}[winds]
        o.dcmip_init(test); o.dcmip_step_inputs(test, nstep, DT)
        if winds == "still":
            o.vn0[...] = 0.0
        o.omega_p[...] = np.random.default_rng(5).uniform(-0.05, 0.05, o.omega_p.shape)   # (the DCMIP inputs leave it 0)
        self.geo = sl.Geo(o)
        self.dp0 = sl.dp0_levels(o.hyai, o.hybi)
        self.Q0 = _scaled(o, qsize) if family == "scaled" else _tracers(o, family, qsize)
        self.family = "ne%d q%d %s %s%s" % (ne, qsize, winds, family, "" if nu is None else " nu_q=%g" % self.nu)
        e = self.elem = elem_from_oracle(o)
        e["vn0"][...] = o.vn0; e["dp"][...] = o.dp; e["eta_dot_dpdn"][...] = o.eta_dot_dpdn; e["omega_p"][...] = o.omega_p
        self.hip = HipMod(e, o.Dvv, (o.hyai, o.hybi, 1.0e5), qsize, self.nu, limiter_option=0, rsplit=o.rsplit)
        e["Qdp"][:, 0] = self.Q0; e["Qdp"][:, 1] = self.Q0
        self.hip.copy_qdp_h2d(e, 1); self.hip.copy_qdp_h2d(e, 2)
        self.hip.set_derived(e)

    def qdp(self, nt):
        self.hip.copy_qdp_d2h(self.elem, nt)
        return self.elem["Qdp"][:, nt - 1].copy()

    def derived(self):
        n = self.o.nelem
        out = dict(divdp_proj=np.zeros((n, 72, 4, 4)), eta_dot_dpdn=np.zeros((n, 73, 4, 4)), omega_p=np.zeros((n, 72, 4, 4)),
                   divdp=np.zeros((n, 72, 4, 4)))
        self.hip.get_derived(out)
        return out

    def close(self):
        self.hip.close(); self.o.close()


def _check(route, stage, family, got, t):
    worst, r = sl.ratio(got, t)
    record_margin("pointwise step %s %s %s" % (route, stage, family), worst, 1.0)
    if worst > 1.0:
        ix = np.unravel_index(int(np.argmax(r)), r.shape)
        where = dict(zip(("element", "tracer", "level", "j", "i") if r.ndim == 5 else ("element", "level", "j", "i"), map(int, ix)))
        pytest.fail("%s %s %s: |got - v| / bound = %.3g (m = %d) at %s; got %r, v %r, A %r; %d points over"
                    % (route, stage, family, worst, t.m, where, float(np.asarray(got)[ix]), float(t.v[ix]), float(t.A[ix]),
                       int((r > 1).sum())))


PER_STAGE = [   # (ne, qsize, winds, family, nu_q or None, amplify divdp_proj)
    (2, 5, "dcmip11-t0", "bells", None, False),
    (2, 5, "dcmip11-mid", "noise", None, False),
    (3, 2, "dcmip12", "halfzero", None, False),
    (5, 1, "dcmip12", "bells", None, False),
    (2, 35, "dcmip11-t0", "scaled", None, False),
    (2, 5, "still", "noise", STILL_NU, False),
    (2, 5, "dcmip12", "scaled", 0.0, False),
    (2, 5, "dcmip12", "bells", None, True),
]


@pytest.mark.parametrize("ne,qsize,winds,family,nu,amp", PER_STAGE, ids=["-".join(map(str, c[:4])) + ("-amp" if c[5] else "") +
                                                                          ("" if c[4] is None else "-nu%g" % c[4]) for c in PER_STAGE])
def test_per_stage_api_pointwise(ne, qsize, winds, family, nu, amp):
    assert sl.has_extended_precision(), np.finfo(np.longdouble)
    c = Ctx(ne, qsize, winds, family, nu)
    fam = c.family + (" amplified" if amp else "")
    o, geo, hip = c.o, c.geo, c.hip
    try:
        hip.compute_divdp()
        d = c.derived()
        ref = sl.compute_divdp(geo, o.vn0)
        _check("per-stage", "divdp", fam, d["divdp"], ref)
        _check("per-stage", "divdp_proj", fam, d["divdp_proj"], ref)
        dts = DT / 2
        for np1, n0, dss, rhs in STAGES:
            if amp and rhs == 1:   # rhs*dt*|divdp_proj| reaches 0.5*dp: kappa of dp_stage up to 3 in stages 2 and 3
                dvp = d["divdp_proj"]
                x = dvp * (0.5 / float((2 * dts * np.abs(dvp) / o.dp).max()))
                hip.set_divdp(dict(divdp_proj=x))
                d = c.derived()
                assert np.array_equal(d["divdp_proj"], x)
            q_in, d = c.qdp(n0), c.derived()
            var_name = {1: "eta_dot_dpdn", 2: "omega_p", 3: "divdp_proj"}[dss]
            var_in = d[var_name][:, :72].copy()
            dvp_in = d["divdp_proj"].copy()
            hip.euler_step(np1, n0, dts, dss, rhs)
            got, d = c.qdp(np1), c.derived()
            qt, vt = sl.euler_step(geo, sl.exact(q_in), o.dp, o.vn0, sl.exact(dvp_in), sl.exact(var_in), dts, rhs, c.nu, c.dp0)
            _check("per-stage", "stage%d Qdp" % (rhs + 1), fam, got, qt)
            _check("per-stage", "stage%d %s" % (rhs + 1, var_name), fam, d[var_name][:, :72], vt)
        qa, qb = c.qdp(1), c.qdp(2)
        hip.qdp_time_avg(3, 1, 2)
        got = c.qdp(2)
        _check("per-stage", "qdp_time_avg", fam, got, sl.qdp_time_avg(sl.exact(qa), sl.exact(qb)))
        assert np.array_equal(got.view(np.uint64), ((qa + 2.0 * qb) / 3.0).view(np.uint64))
        assert np.array_equal(c.qdp(1).view(np.uint64), qa.view(np.uint64))
    finally:
        c.close()


WHOLE = [   # (ne, qsize, winds, family, nu_q or None, DSS on read)
    (2, 5, "dcmip11-t0", "bells", None, True),
    (2, 5, "dcmip11-t0", "bells", None, False),
    (3, 2, "dcmip12", "halfzero", None, True),
    (3, 2, "dcmip12", "halfzero", None, False),
    (2, 35, "dcmip11-mid", "scaled", None, True),
    (2, 35, "dcmip11-mid", "scaled", None, False),
    (5, 1, "dcmip12", "noise", None, True),
    (2, 5, "still", "noise", STILL_NU, True),
    (2, 5, "dcmip12", "scaled", 0.0, True),
    (2, 5, "dcmip12", "scaled", 0.0, False),
]


@pytest.mark.parametrize("ne,qsize,winds,family,nu,on_read", WHOLE, ids=["-".join(map(str, c[:4])) + ("" if c[4] is None else "-nu%g" % c[4]) +
                                                                       ("-dss-on-read" if c[5] else "-dss-per-stage") for c in WHOLE])
def test_whole_step_pointwise(ne, qsize, winds, family, nu, on_read):
    assert sl.has_extended_precision(), np.finfo(np.longdouble)
    route = "whole-step-" + ("dss-on-read" if on_read else "dss-per-stage")
    c = Ctx(ne, qsize, winds, family, nu)
    o = c.o
    try:
        with _dss_on_read(on_read):
            c.hip.advec_tracers_remap_rk2(DT, 1, 2)
        ref = sl.advec_tracers_remap_rk2(c.geo, c.Q0, o.dp, o.vn0, o.eta_dot_dpdn[:, :72], o.omega_p, DT, c.nu, c.dp0)
        d = c.derived()
        _check(route, "Qdp", c.family, c.qdp(2), ref["Qdp"])
        for name in ("divdp", "divdp_proj", "omega_p"):
            _check(route, name, c.family, d[name], ref[name])
        _check(route, "eta_dot_dpdn", c.family, d["eta_dot_dpdn"][:, :72], ref["eta_dot_dpdn"])
        assert np.array_equal(c.qdp(1).view(np.uint64), c.Q0.view(np.uint64)), "Qdp(n0) changed"
    finally:
        c.close()


@pytest.mark.parametrize("ne,qsize", [(2, 5), (3, 35)])
def test_element_mass_pointwise(ne, qsize):
    """tse_element_mass (prim_main's mass lines) per element and tracer against the longdouble sum_k sum_p spheremp*Qdp, at slot scalings
    from 2^-200 to 2^200 (m = 16 + 71)"""
    c = Ctx(ne, qsize, "dcmip11-t0", "scaled")
    try:
        got = c.hip.element_mass(1)
        _check("element-mass", "Qdp(1)", c.family, got, sl.element_mass(c.geo, c.Q0))
    finally:
        c.close()
