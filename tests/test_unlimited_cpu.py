"""limiter_option = 0 (no limiter) without a GPU: the reference model of the unlimited step (unlimited_model.py), the namelist front end
and the C ABI's refusal rules.

* Model check: with pyoracle.limiter8 put back per slab, the model is the checker's euler_step bit for bit, stage by stage -- so the
  model differs from the checker in the limiter alone.
* Model properties: exact under Qdp * 2^+-256, and the tracer mass sum(spheremp * Qdp) of every level is conserved to rounding.
* prim_main.settings takes limiter_option = 0 and a namelist without the key (control_mod's default is 0), and still refuses 4 and 84.
* tse_init takes 0 (on this host it fails on the missing device, not on the limiter) and refuses 4 naming limiter_option=8."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as po
import unlimited_model as um
from tracer_fields import NBASE, base_tracers
from transport_se_amd import _lib
from transport_se_amd import prim_main as pm

DT = 1800.0
NU_Q = 1e19


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _state(qdp0=None):
    """ne2 oracle at the first tracer step of DCMIP 1-1, Qdp = the base fields (or qdp0) at both time levels, divdp formed"""
    o = po.Oracle(2, NBASE, nu_q=NU_Q)
    o.dcmip_init(1)
    b = base_tracers(o) if qdp0 is None else qdp0
    o.qdp[0] = np.moveaxis(b, 0, 1); o.qdp[1] = o.qdp[0]
    o.dcmip_step_inputs(1, 0, DT)
    for e in range(o.nelem):
        for k in range(um.NLEV):
            d = o.divergence_sphere(e, o.vn0[e, k])
            o.divdp[e, k] = d; o.divdp_proj[e, k] = d
    return o


class Limiter8:
    """the checker's bounds (prim_advection_mod.F90:764-812 + neighbor_minmax) and pyoracle.limiter8, in its comparison order"""

    def __init__(self, o):
        self.o, self.mn, self.mx = o, None, None

    def bounds(self, Q, rhs):
        mn, mx = Q[..., 0, 0].copy(), Q[..., 0, 0].copy()
        for p in range(1, 16):
            x = Q[..., p // 4, p % 4]
            mn = np.where(x < mn, x, mn); mx = np.where(x > mx, x, mx)
        if rhs == 1:
            self.mn = np.where(mn < self.mn, mn, self.mn); self.mx = np.where(mx > self.mx, mx, self.mx)
            return
        self.mn, self.mx = mn, mx
        m0, x0 = mn.copy(), mx.copy()
        for e in range(self.o.nelem):
            for d in range(8):
                n = self.o.nbr_elem[e, d]
                if n < 0:
                    continue
                self.mn[e] = np.where(m0[n] < self.mn[e], m0[n], self.mn[e])
                self.mx[e] = np.where(x0[n] > self.mx[e], x0[n], self.mx[e])

    def apply(self, e, q, k, qt, dp_star):
        out, mn, mx, _ = po.limiter8(qt, self.o.spheremp[e], self.mn[e, q, k], self.mx[e, q, k], dp_star)
        self.mn[e, q, k], self.mx[e, q, k] = mn, mx
        return out


STAGES = [(2, 1, 3, 0), (2, 2, 1, 1), (2, 2, 2, 2)]   # (np1_qdp, n0_qdp, dssopt, rhs_multiplier) of the three RK stages


def test_model_with_the_limiter_put_back_is_the_checker():
    o, m = _state(), _state()
    lim = Limiter8(m)
    try:
        for np1, n0, dssopt, rhs in STAGES:
            o.euler_step(np1, n0, DT / 2, dssopt, rhs)
            um.euler_step(m, np1, n0, DT / 2, dssopt, rhs, limiter=lim)
            for name in ("qdp", "divdp_proj", "eta_dot_dpdn", "omega_p"):
                assert np.array_equal(_bits(getattr(m, name)), _bits(getattr(o, name))), (rhs, name)
    finally:
        o.close(); m.close()


def test_model_without_the_limiter_is_not_the_checker():
    """the 0/1 noise field overshoots without the limiter: the two must differ there (else the comparison above proves nothing)"""
    o, m = _state(), _state()
    try:
        o.euler_step(2, 1, DT / 2, 3, 0)
        um.euler_step(m, 2, 1, DT / 2, 3, 0)
        assert not np.array_equal(m.qdp[1][:, 1], o.qdp[1][:, 1])
    finally:
        o.close(); m.close()


@pytest.mark.parametrize("e", [256, -256])
def test_model_power_of_two_scaling(e):
    a = _state()
    b = _state(np.ldexp(base_tracers(a), e))
    try:
        um.advec_tracers_remap_rk2(a, DT, 0)
        um.advec_tracers_remap_rk2(b, DT, 0)
        assert np.all(np.isfinite(b.qdp))
        assert np.array_equal(_bits(b.qdp), _bits(np.ldexp(a.qdp, e)))
    finally:
        a.close(); b.close()


CONTINUOUS = [0, 3, 4, 5]   # base fields that are functions of (lat, lon, level): the same value on both sides of an element edge


def test_model_conserves_mass_per_level():
    """sum(spheremp * Qdp) of every level and tracer is what it was, to rounding (the DSS'd flux divergence and the weak Laplacians
    integrate to zero over the sphere when the tracer is continuous across element edges; the 0/1 noise and spike fields are not)"""
    o = _state()
    try:
        def mass(tl, f=lambda x: x):
            return np.einsum("eqkji,eji->qk", f(o.qdp[tl - 1][:, CONTINUOUS]), o.spheremp)
        m0 = mass(1)
        for np1, n0, dssopt, rhs in STAGES:
            um.euler_step(o, np1, n0, DT / 2, dssopt, rhs)
            rel = np.abs(mass(np1) - m0) / np.maximum(mass(np1, np.abs), 1e-300)
            assert rel.max() < 1e-13, (rhs, rel.max())
    finally:
        o.close()


NL = """
&ctl_nl
  test_case = "dcmip1-1"
  ne = 8
  qsize = 4
  nmax = 6
  tstep = 400
  qsplit = 1, rsplit = 3
  nu_q = 6e16
  limiter_option = 0
/
&vert_nl
  vform = "ccm"
/
"""


def test_settings_take_limiter_option_0_and_its_default():
    assert pm.settings(pm.parse_namelists(NL))["limiter_option"] == 0
    s = pm.settings(pm.parse_namelists(NL.replace("  limiter_option = 0\n", "")))
    assert s["limiter_option"] == 0          # control_mod's default
    assert pm.settings(pm.parse_namelists(NL.replace("limiter_option = 0", "limiter_option = 8")))["limiter_option"] == 8
    for bad in (4, 84, 1, -1):
        with pytest.raises(SystemExit, match="limiter_option"):
            pm.settings(pm.parse_namelists(NL.replace("limiter_option = 0", "limiter_option = %d" % bad)))


def _init_error(limiter_option):
    L = _lib.lib()
    a = _lib.InitArgs()
    # device 4096 exists nowhere: tse_init fails before it touches a field, on a host with GPUs as on one without
    a.nelemd, a.qsize, a.device, a.limiter_option = 1, 1, 4096, limiter_option
    h = C.c_void_p()
    assert L.tse_init(C.byref(h), C.byref(a)) != 0
    assert not h.value
    return L.tse_last_error().decode()


def test_init_takes_limiter_option_0():
    err = _init_error(0)
    assert err and "limiter" not in err, err
    assert "limiter_option=8" in _init_error(4)
    assert "limiter_option=8" in _init_error(84)
