"""-m gpu: level-order invariance of the production kernels, through the public ABI.

Within a tracer step the levels are independent (no remap): permuting the levels of every input -- Qdp, dp, vn0 and with it the divdp_proj
formed from it; eta_dot_dpdn and omega_p are zero -- must permute Qdp(np1) and tse_get_qminmax bit for bit.  A wavefront of k_advance holds
16 consecutive levels of one element and tracer, and limiter8_quad leaves its loop on a wave-wide vote, so a permutation changes every
slab's wave-mates: a slab "left untouched" while its wave iterates on, or a wave-wide test that should have been per slab, shows here in the
copies of the limiters inlined in the production kernels (tests/test_gpu_limiter_slab.py holds the limiters' own source to the same).
The slot-invariance tests (test_gpu_tracer_invariance.py) change the tracer and keep the levels; the 80-level window tests shift levels by
multiples of 4 and keep their order.

dp0(k) of the biharmonic is the one level-dependent constant; the vertical coordinate here has uniform dp0 (hyai = k/128, hybi = 0: every
(hyai(k+1)-hyai(k))*ps0 is exactly ps0/128), so stage 3's biharmonic runs (nu_q > 0).  Tracer q at level k is one of 0/1 noise, uniform,
5 % spikes of 50, smooth -- kind (k + q) mod 4 -- so the limiter's work differs between neighbouring levels."""
import contextlib
import os

import numpy as np
import pytest

import pyoracle as po
from gpu_common import elem_from_oracle
from transport_se_amd import HipMod

pytestmark = pytest.mark.gpu

NLEV, QSIZE = 72, 4
ROUTES = ("stages", "whole_step", "whole_step_dss_per_stage")


def _params(ne):
    return (1e19, 1800.0) if ne == 2 else (1e15 * (30.0 / ne) ** 3.2, 300.0 * 30.0 / ne)


def permutations():
    """{name: level permutation}: whole aligned chunks of 4 levels moved about (chunk order reversed; a seeded shuffle of the chunks), and
    arbitrary permutations (reversal, rotation by 5, a seeded shuffle)"""
    k = np.arange(NLEV)
    rng = np.random.default_rng(20261102)
    chunks = k.reshape(NLEV // 4, 4)
    return {"chunks reversed": chunks[::-1].ravel(), "chunks shuffled": chunks[rng.permutation(NLEV // 4)].ravel(),
            "reversed": k[::-1].copy(), "rotated by 5": np.roll(k, 5), "shuffled": rng.permutation(NLEV)}


def _fields(o, dt):
    """(Qdp[ie][q][k][j][i], vn0, dp) on the oracle's grid: DCMIP 1-1 winds and layer thicknesses, the tracer kinds cycling with the level"""
    o.dcmip_init(1); o.dcmip_step_inputs(1, 0, dt)
    vn0, dp = o.vn0.copy(), o.dp.copy()
    rng = np.random.default_rng(20261101)
    shp = (o.nelem, NLEV, 4, 4)
    k = np.arange(NLEV)[None, :, None, None]
    la, lo = o.lat[:, None], o.lon[:, None]
    kinds = [rng.choice([0.0, 1.0], size=shp), np.full(shp, 0.75), np.where(rng.uniform(size=shp) < 0.05, 50.0, 0.0),
             1.0 + 0.45 * np.sin(3.0 * lo + 0.37 * k) * np.cos(2.0 * la) + 0.3 * np.cos(0.53 * k + 2.0 * la)]
    Q = np.stack([np.choose((k + q) % 4 + np.zeros(shp, int), kinds) for q in range(QSIZE)], axis=1)
    return Q * dp[:, None], vn0, dp


@contextlib.contextmanager
def _dss_on_read(value):
    old = os.environ.pop("TSE_DSS_ON_READ", None)
    if value is not None:
        os.environ["TSE_DSS_ON_READ"] = value
    try:
        yield
    finally:
        os.environ.pop("TSE_DSS_ON_READ", None)
        if old is not None:
            os.environ["TSE_DSS_ON_READ"] = old


def _run(hip, elem, route, dt, limiter, qdp, vn0, dp):
    """one tracer step without remap from Qdp in both time levels: (Qdp(np1), qmin, qmax); no bounds exist without a limiter"""
    elem["Qdp"][:, 0] = qdp; elem["Qdp"][:, 1] = qdp
    elem["vn0"][...] = vn0; elem["dp"][...] = dp
    elem["eta_dot_dpdn"][...] = 0.0; elem["omega_p"][...] = 0.0
    hip.copy_qdp_h2d(elem, 1); hip.copy_qdp_h2d(elem, 2)
    hip.set_derived(elem)
    with _dss_on_read("0" if route == "whole_step_dss_per_stage" else None):
        if route == "stages":   # Prim_Advec_Tracers_remap_rk2 through the per-stage entries (prim_advection_mod.F90:579-640)
            hip.compute_divdp()
            hip.euler_step(2, 1, dt / 2, 3, 0); hip.euler_step(2, 2, dt / 2, 1, 1); hip.euler_step(2, 2, dt / 2, 2, 2)
            hip.qdp_time_avg(3, 1, 2)
        else:
            hip.advec_tracers_remap_rk2(dt, 1, 2)
    hip.copy_qdp_d2h(elem, 2)
    out = elem["Qdp"][:, 1].copy()
    assert np.isfinite(out).all()
    return (out,) + (tuple(hip.get_qminmax()) if limiter else ())


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("limiter", [8, 9, 0])
@pytest.mark.parametrize("ne", [2, 3])
def test_permuting_the_levels_permutes_the_result(ne, limiter):
    nu, dt = _params(ne)
    o = po.Oracle(ne, QSIZE, nu_q=nu)
    elem = elem_from_oracle(o)
    hip = HipMod(elem, o.Dvv, (np.arange(NLEV + 1) / 128.0, np.zeros(NLEV + 1), 1.0e5), QSIZE, nu, limiter_option=limiter, rsplit=o.rsplit)
    try:
        qdp, vn0, dp = _fields(o, dt)
        if limiter:   # the limiter has work in a good share of the slabs, and differently from one level to the next
            free = HipMod(elem, o.Dvv, (np.arange(NLEV + 1) / 128.0, np.zeros(NLEV + 1), 1.0e5), QSIZE, nu, limiter_option=0, rsplit=o.rsplit)
            try:
                unlimited = _run(free, elem, "stages", dt, 0, qdp, vn0, dp)[0]
            finally:
                free.close()
            touched = (_run(hip, elem, "stages", dt, limiter, qdp, vn0, dp)[0] != unlimited).any(axis=(3, 4))   # [ie][q][k]
            kind = (np.arange(NLEV)[None, :] + np.arange(QSIZE)[:, None]) % 4
            share = [float(touched[:, kind == i].mean()) for i in range(4)]
            print("ne%d limiter %d: slabs the limiter changed, by kind (noise, uniform, spikes, smooth): %s" % (ne, limiter, share))
            assert share[0] > 0.5 and touched.mean() > 0.25, share
        bad = []
        for route in ROUTES:
            base = _run(hip, elem, route, dt, limiter, qdp, vn0, dp)
            assert not np.array_equal(base[0], qdp)
            for name, p in permutations().items():
                assert sorted(p.tolist()) == list(range(NLEV))
                got = _run(hip, elem, route, dt, limiter, qdp[:, :, p], vn0[:, p], dp[:, p])
                for what, g, b in zip(("Qdp", "qmin", "qmax"), got, base):
                    eq = _bits(g) == _bits(b[:, :, p])
                    if not eq.all():
                        lev = np.nonzero(~eq.reshape(eq.shape[:3] + (-1,)).all(axis=(0, 1, 3)))[0]
                        bad.append((route, name, what, "levels (new positions) %s" % lev[:12].tolist(), int((~eq).sum())))
        assert not bad, bad
    finally:
        hip.close(); o.close()
