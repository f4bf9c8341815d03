"""The longdouble model of the unlimited tracer step and its pointwise error bound (step_ld.py), without a GPU.

* The triple arithmetic counts divergence_sphere at 13 and laplace_sphere_wk at 19 roundings -- elem_ops_ld's hand count -- and gives
  elem_ops_ld's values and magnitudes at every element of ne2 within the longdouble term.
* Its DSS is the oracle's: Dss.fp64 is Oracle.dss bit for bit, and the 8 cube corners are nodes of 3 elements.
* The fp64 model of the unlimited step (unlimited_model.py: serial sums in the reference's operand order) is within the bound at every
  point at ne2 with 5 tracers (scaled by 2^-200 .. 2^200): each of the three stages from identical inputs, the whole step, and the
  DSS'd extra variables.
* The bound has teeth: a vectorised fp64 copy of the step (other sums, other associations) is within the bound, and each of six
  realistic mutations of that copy breaks it somewhere."""
import numpy as np
import pytest

import pyoracle as po
import step_ld as sl
import elem_ops_ld as el
import unlimited_model as um
from conftest import record_margin
from tracer_fields import base_tracers

DT, NU_Q = 1800.0, 1e19
SCALES = (0, -17, 200, 3, -200)        # per-slot power-of-two exponents of the 5 tracers
TINY = 4                               # the slot scaled by 2^-200


@pytest.fixture(scope="module")
def case():
    assert sl.has_extended_precision(), np.finfo(np.longdouble)
    o = po.Oracle(2, len(SCALES), nu_q=NU_Q)
    o.dcmip_init(1); o.dcmip_step_inputs(1, 0, DT)
    o.omega_p[...] = np.random.default_rng(5).uniform(-0.05, 0.05, o.omega_p.shape)   # (the DCMIP inputs leave it 0)
    b = base_tracers(o)[:len(SCALES)]
    Q0 = np.moveaxis(np.stack([np.ldexp(b[i], s) for i, s in enumerate(SCALES)]), 0, 1).copy()
    geo = sl.Geo(o)
    dp0 = sl.dp0_levels(o.hyai, o.hybi)
    ins = dict(Q0=Q0, dp=o.dp.copy(), vn0=o.vn0.copy(), eta=o.eta_dot_dpdn[:, :72].copy(), om=o.omega_p.copy())
    ref = sl.advec_tracers_remap_rk2(geo, Q0, ins["dp"], ins["vn0"], ins["eta"], ins["om"], DT, NU_Q, dp0)
    yield o, geo, dp0, ins, ref
    o.close()


def _worst(got, t):
    return sl.ratio(got, t)[0]


# ---- the operators ----
def test_operator_counts_and_values_match_elem_ops_ld(case):
    o, geo = case[0], case[1]
    v, s = el.smooth_vector(o, 1), el.smooth_scalar(o, 1)
    rng = np.random.default_rng(7)
    for v, s in ((v, s), (rng.uniform(-20, 20, v.shape), rng.uniform(-300, 300, s.shape))):
        d = sl.divergence_sphere(geo, sl.exact(v[:, 0]), sl.exact(v[:, 1]))
        l = sl.laplace_sphere_wk(geo, sl.exact(s))
        assert d.m <= el.N_DIV and l.m <= el.N_LAP, (d.m, l.m)
        for t, (ref, A) in ((d, el.divergence_sphere(o, v)), (l, el.laplace_sphere_wk(o, s))):
            ld_term = 2 * sl.gamma(t.m, 2.0 ** -64) * A
            assert np.all(np.abs(t.v - ref) <= ld_term)
            assert np.all(np.abs(t.A - A) <= ld_term)


def test_dss_is_the_oracles(case):
    o, geo = case[0], case[1]
    f = np.random.default_rng(3).standard_normal((o.nelem, 5, 4, 4))
    f[:, 1] = -0.0
    assert np.array_equal(geo.dss.fp64(f).view(np.uint64), o.dss(f.copy(), 0).view(np.uint64))
    assert (geo.dss.count == 3).sum() == 8 * 3          # the cube corners
    assert (geo.dss.count == 4).sum() == o.nelem * 4 - 8 * 3   # every other element corner
    t = geo.dss.ld(sl.exact(f))
    assert t.m == 3 and np.all(np.abs(t.v - geo.dss.fp64(f)) <= sl.bound(3, t.A))


# ---- the fp64 reference model within the bound ----
STAGES = [(2, 1, 3, 0), (2, 2, 1, 1), (2, 2, 2, 2)]   # (np1, n0, dssopt, rhs_multiplier)


def test_unlimited_model_stages_within_bound(case):
    o, geo, dp0, ins, _ = case
    o.qdp[0] = ins["Q0"]; o.qdp[1] = ins["Q0"]
    o.dp[...] = ins["dp"]; o.vn0[...] = ins["vn0"]
    for e in range(o.nelem):
        for k in range(um.NLEV):
            o.divdp[e, k] = o.divergence_sphere(e, o.vn0[e, k])
    o.divdp_proj[...] = o.divdp
    for np1, n0, dss, rhs in STAGES:
        var = {1: o.eta_dot_dpdn[:, :72], 2: o.omega_p, 3: o.divdp_proj}[dss]
        q, vd = sl.euler_step(geo, sl.exact(o.qdp[n0 - 1]), o.dp, o.vn0, sl.exact(o.divdp_proj), sl.exact(var), DT / 2, rhs, NU_Q, dp0)
        um.euler_step(o, np1, n0, DT / 2, dss, rhs)
        var = {1: o.eta_dot_dpdn[:, :72], 2: o.omega_p, 3: o.divdp_proj}[dss]
        for name, got, t in (("Qdp", o.qdp[np1 - 1], q), ("extra", var, vd)):
            r = _worst(got, t)
            record_margin("pointwise step cpu-model stage%d %s" % (rhs + 1, name), r, 1.0)
            assert r <= 1.0, (rhs, name, r, t.m)


def test_unlimited_model_whole_step_within_bound(case):
    o, geo, dp0, ins, ref = case
    o.qdp[0] = ins["Q0"]; o.qdp[1] = ins["Q0"]
    o.dp[...] = ins["dp"]; o.vn0[...] = ins["vn0"]; o.eta_dot_dpdn[:, :72] = ins["eta"]; o.omega_p[...] = ins["om"]
    um.advec_tracers_remap_rk2(o, DT, 0)
    for name, got in (("Qdp", o.qdp[1]), ("divdp", o.divdp), ("divdp_proj", o.divdp_proj), ("eta_dot_dpdn", o.eta_dot_dpdn[:, :72]),
                      ("omega_p", o.omega_p)):
        r = _worst(got, ref[name])
        record_margin("pointwise step cpu-model whole-step %s" % name, r, 1.0)
        assert r <= 1.0, (name, r, ref[name].m)
    assert ref["Qdp"].m == 161 and [t.m for t in ref["stages"]] == [38, 81, 158]


# ---- teeth: a vectorised fp64 copy of the step, and mutations of it ----
def _div(G, v1, v2):
    D = G["D"]
    gv1 = G["met"] * (D[0][0] * v1 + D[0][1] * v2)
    gv2 = G["met"] * (D[1][0] * v1 + D[1][1] * v2)
    s = np.einsum("li,e...ji->e...jl", G["Dvv"], gv1) + np.einsum("li,e...ij->e...lj", G["Dvv"], gv2)
    return s * (G["rmet"] * sl.RREARTH)


def _lap(G, s):
    D, Dvv, rr = G["D"], G["Dvv"], sl.RREARTH
    v1 = np.einsum("li,e...ji->e...jl", Dvv, s) * rr
    v2 = np.einsum("li,e...ij->e...lj", Dvv, s) * rr
    ds1, ds2 = D[0][0] * v1 + D[1][0] * v2, D[0][1] * v1 + D[1][1] * v2
    vt1, vt2 = D[0][0] * ds1 + D[0][1] * ds2, D[1][0] * ds1 + D[1][1] * ds2
    return -(np.einsum("jm,e...nj->e...nm", Dvv, G["sph"] * vt1) + np.einsum("jn,e...jm->e...nm", Dvv, G["sph"] * vt2)) * rr


def _geo64(geo, mut, e_swap):
    ex = lambda x: x[:, None, None]                     # noqa: E731  ([e][4][4] against [e][q][k][4][4])
    D = [[geo.D[a][b].copy() for b in range(2)] for a in range(2)]
    if mut == "dinv_swap":
        D[0][1][e_swap], D[1][0][e_swap] = geo.D[1][0][e_swap].copy(), geo.D[0][1][e_swap].copy()
    rsp = geo.rspheremp.astype(np.float32).astype(np.float64) if mut == "rspheremp_f32" else geo.rspheremp
    return dict(D=[[ex(d) for d in r] for r in D], Dvv=geo.Dvv, met=ex(geo.metdet), rmet=ex(geo.rmetdet), sph=ex(geo.spheremp),
                rsp=ex(rsp)), dict(D=[[d[:, None] for d in r] for r in D], Dvv=geo.Dvv, met=geo.metdet[:, None],
                                   rmet=geo.rmetdet[:, None], sph=geo.spheremp[:, None], rsp=rsp[:, None])


def _step64(geo, ins, dp0, mut=None, where=None):
    Gq, Gk = _geo64(geo, mut, where.get("e_swap"))
    drop = where["drop"] if mut == "dss_drop" else None
    dss = lambda f: geo.dss.fp64(f, drop)                 # noqa: E731
    dp, vn0 = ins["dp"], ins["vn0"]
    d0 = dp0.copy()
    if mut == "dp0_next_level":
        d0[where["k"]] = dp0[where["k"] + 1]

    def stage(Q, dvp, var, dt, rhs):
        dpk = dp - (rhs * dt) * dvp
        vs1, vs2 = (vn0[:, :, 0] / dpk)[:, None], (vn0[:, :, 1] / dpk)[:, None]
        qt = Q - dt * _div(Gq, vs1 * Q, vs2 * Q)
        if rhs == 2:
            lap = Gq["rsp"] * dss(_lap(Gq, Q / dpk[:, None]))
            qt = qt + (-3.0 * dt * NU_Q * d0[None, None, :, None, None]) * _lap(Gq, lap) / Gq["sph"]
        return Gq["rsp"] * dss(Gq["sph"] * qt), Gk["rsp"] * dss(Gk["sph"] * var)

    Q0 = ins["Q0"]
    divdp = _div(Gk, vn0[:, :, 0], vn0[:, :, 1])
    q1, dvp = stage(Q0, divdp, divdp, DT / 2, 0)
    q2, eta = stage(q1, divdp if mut == "stage2_dp_before_dss" else dvp, ins["eta"], DT / 2, 1)
    q3, om = stage(q2, dvp, ins["om"], DT / 2, 2)
    q = (Q0 + 2.0 * q3) / 3.0
    if mut == "perturb_tiny_top":
        e, j, i = where["point"]
        q[e, TINY, 0, j, i] *= 1.0 + 2.0 ** -30
    return dict(Qdp=q, divdp=divdp, divdp_proj=dvp, eta_dot_dpdn=eta, omega_p=om)


MUTATIONS = ("dss_drop", "dinv_swap", "dp0_next_level", "stage2_dp_before_dss", "rspheremp_f32", "perturb_tiny_top")


def _where(geo):
    e, p = np.argwhere(geo.dss.count == 3)[0]                       # a cube-corner node
    d = np.abs(geo.D[0][1] - geo.D[1][0]).max(axis=(1, 2))          # the element where Dinv(1,2) and Dinv(2,1) differ most
    return dict(drop=(int(e), int(p), 1), e_swap=int(np.argmax(d)), k=40, point=(5, 1, 2))


@pytest.mark.parametrize("mut", (None,) + MUTATIONS)
def test_mutations_of_the_fp64_step_are_caught(case, mut):
    o, geo, dp0, ins, ref = case
    got = _step64(geo, ins, dp0, mut, _where(geo))
    worst = {name: _worst(got[name], ref[name]) for name in got}
    r = max(worst.values())
    record_margin("pointwise step cpu-model vectorised %s" % (mut or "unmutated"), r, 1.0)
    if mut is None:
        assert r <= 1.0, worst
    else:
        assert r > 1.0, (mut, worst)
