"""The tracer forcing without a GPU: the C ABI (tse_apply_forcing, tse_apply_forcing_host) in the header, the symbol list, the product
libraries and the Fortran seam; the numpy model tests/forcing_model.py held to its own claims -- the families of the generator take the
branches they are built for, exact scaling by powers of two, the budget closes within the summation bound, four planted errors are caught by
a bit comparison -- and the paths tse_view_plan gives the layouts of the GPU test."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import forcing_model as fm
from transport_se_amd import _lib
from transport_se_amd.hip_mod import view_plan
from transport_se_amd.hybvcoord import HvCoord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NE, QS, NLEV = 6, 3, 72   # the model's shapes: six elements are enough for every family and sub-case to occur thousands of times

SIGNATURES = {
    "tse_apply_forcing": "int tse_apply_forcing(tse_ctx *ctx, int nt, double dt, int mode, const tse_view *fq, void *stream, double *budget)",
    "tse_apply_forcing_host": "int tse_apply_forcing_host(tse_ctx *ctx, int nt, double dt, int mode, const double *fq_elem1, size_t elem_stride, "
                              "int qsize_d, double *budget)",
}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def hv():
    h = HvCoord()
    return (h.hyai, h.hybi, h.ps0)


@pytest.fixture(scope="module")
def spheremp():
    return np.random.default_rng(7).uniform(0.5e-3, 2e-3, (NE, 4, 4))


@pytest.fixture(scope="module")
def cases(hv):
    """mode -> (Qdp, FQ, dp, dt, result of the model), computed once"""
    out = {}
    for mode in (0, 1):
        qdp, fq, ps_v, dt = fm.forcing_fields(NE, QS, NLEV, mode=mode, hv=hv)
        dp = fm.level_dp(hv[0], hv[1], hv[2], ps_v)
        out[mode] = (qdp, fq, dp, dt, fm.apply(qdp, fq, dt, mode, dp))
    return out


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_symbols_libraries_and_seam():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()).rstrip(";").strip() for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    for name, sig in SIGNATURES.items():
        assert decl.get(name) == sig, decl.get(name)
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+TSE_FORCING_TENDENCY\s+0\b", text) and re.search(r"#define\s+TSE_FORCING_ADJUST\s+1\b", text)
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
        L = _lib.lib(nlev=nlev)
        assert all(hasattr(L, n) for n in SIGNATURES), nlev
    assert all(hasattr(_lib.lib(_lib.HOOKS_SO), n) for n in SIGNATURES)
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    for c_name in SIGNATURES:
        assert "name='%s'" % c_name in src, c_name
    for name, args in (("apply_forcing_hip", "nt, dt, mode, ptr, strides, stream"), ("apply_forcing_elem_hip", "elem, nt, tl, dt, mode")):
        assert re.search(r"subroutine\s+%s\s*\(\s*%s\s*\)" % (name, args), src), name
        assert re.search(r"public\s*::[^\n]*\b%s\b" % name, src), name
        body = src.split("subroutine %s" % name)[1].split("end subroutine")[0]
        assert "call check(" in body and "!$omp master" in body and body.count("!$omp barrier") == 2, name
    assert "c_loc(elem(1)%derived%fq(1,1,1,1,tl))" in src


# ---- the generator and the branches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_every_family_takes_its_branch(cases, mode):
    qdp, fq, dp, dt, res = cases[mode]
    N = NE * QS * NLEV * 16
    fam = fm.family_of(qdp.shape)
    assert all(int((fam == f).sum()) == N // 8 for f in range(8))
    want = fm.intended_branch(qdp, fq, dt, mode, dp)
    free = want < 0
    assert np.array_equal(res["branch"][~free], want[~free])
    per = {f: np.bincount(res["branch"][fam == f], minlength=3).tolist() for f in range(8)}
    for f, b in ((0, 0), (1, 0), (2, 1), (3, 2), (4, 0), (6, 1), (7, 0)):
        assert per[f][b] == N // 8, (f, per[f])
    assert per[5][2] == 0 and per[5][0] > 0 and per[5][1] > 0, per[5]
    if mode == 0:
        sub = (np.arange(N) // 8).reshape(qdp.shape)
        land = qdp + dt * fq
        m = fam == 5
        assert (land[m & (sub % 3 == 0)] == 0).all()
        up, dn = m & (sub % 3 == 1), m & (sub % 3 == 2)
        assert (land[up] > 0).all() and (land[up] <= np.spacing(qdp[up])).all()
        assert (land[dn] < 0).all() and (-land[dn] <= np.spacing(qdp[dn])).all()
        assert per[5] == [N // 8 - int((m & (sub % 3 == 2)).sum()), int((m & (sub % 3 == 2)).sum()), 0]
        assert (np.abs(dt * fq[fam == 1]) < qdp[fam == 1] / 2).all()
        z = fq[fam == 7]
        assert (z == 0).all() and np.signbit(z).sum() == z.size // 2
    else:
        v = dp[:, None] * (fq - qdp / dp[:, None])
        m = fam == 5
        assert (np.abs(qdp[m] + v[m]) <= np.spacing(qdp[m])).all()          # within one ulp of zero, on either side
        assert (res["applied"][fam == 7] == 0).all()
    # what the families promise about the result
    assert (res["new"][fam == 2] == 0).all() and not np.signbit(res["new"][fam == 2]).any()
    assert _same(res["new"][fam == 3], qdp[fam == 3]) and (qdp[fam == 3] < 0).all()
    assert (res["new"][fam == 4] > 0).all() and (qdp[fam == 4] < 0).all()
    assert (res["new"][fam == 6] == 0).all() and not np.signbit(res["new"][fam == 6]).any()
    assert (res["new"][qdp >= 0] >= 0).all() and (res["new"] >= np.minimum(qdp, 0)).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("power", [200, -200])
def test_scaling_by_a_power_of_two_is_exact(cases, spheremp, mode, power):
    qdp, fq, dp, dt, res = cases[mode]
    s = 2.0 ** power
    scaled = fm.apply(qdp * s, fq * s, dt, mode, dp)
    for key in ("new", "applied", "withheld"):
        assert _same(scaled[key], res[key] * s), key
    assert np.array_equal(scaled["branch"], res["branch"])
    assert _same(fm.budget(spheremp, scaled), fm.budget(spheremp, res) * s)


# ---- the budget ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_the_budget_closes_within_the_summation_bound(cases, spheremp, mode):
    qdp, fq, dp, dt, res = cases[mode]
    b = fm.budget(spheremp, res)
    bound = fm.closure_bound(spheremp, res)
    exact = fm.exact_mass_change(spheremp, qdp, res["new"])
    worst = 0.0
    for e in range(NE):
        for q in range(QS):
            err = abs(Fraction(float(b[e, q, 0])) - exact[e, q])
            assert err <= Fraction(float(bound[e, q])), (e, q, float(err), bound[e, q])
            worst = max(worst, float(err) / bound[e, q])
    assert 0 < worst < 1
    # the order of addition against the exact sum of the same rounded terms: the plain summation bound
    ref = fm.exact_budget(spheremp, res)
    w = spheremp.reshape(NE, 1, 1, 16)
    for j, key in enumerate(("applied", "withheld")):
        T = np.abs(w * res[key].reshape(NE, QS, NLEV, 16)).sum(axis=(2, 3))
        assert (np.abs(b[:, :, j] - ref[:, :, j]) <= (fm.gamma(16 * NLEV - 1) + 2 * fm.U) * T * (1 + 1e-12)).all(), key
    assert (b[:, :, 1] < 0).all()   # mass was withheld everywhere: what the clip keeps back is negative


def test_nothing_withheld_is_bit_zero(hv, spheremp):
    """Without a clipped entry the withheld share is +0.0 in every bit.  Families 2 and 3 clip by design; so do family 6 (a zero mass with
    FQ < 0) and the one-ulp-below third of family 5, whose withheld mass is one ulp or dt*FQ -- they are left out as well."""
    for mode in (0, 1):
        qdp, fq, ps_v, dt = fm.forcing_fields(NE, QS, NLEV, mode=mode, hv=hv, families=(0, 1, 4, 7))
        res = fm.apply(qdp, fq, dt, mode, fm.level_dp(hv[0], hv[1], hv[2], ps_v))
        assert (res["branch"] == fm.NOCLIP).all()
        b = fm.budget(spheremp, res)
        assert (_bits(b[:, :, 1]) == 0).all() and (b[:, :, 0] != 0).all()


# ---- planted errors --------------------------------------------------------------------------------------------------------------
def test_planted_errors_are_caught_by_a_bit_comparison(cases, spheremp):
    qdp, fq, dp, dt, res = cases[0]
    fam = fm.family_of(qdp.shape)
    # 1: the clip ignores Qdp < 0 -- an undershoot is zeroed
    bad = fm.apply(qdp, fq, dt, 0, plant="ignore_negative")
    diff = _bits(bad["new"]) != _bits(res["new"])
    assert diff.any() and set(np.unique(fam[diff])) == {3}
    # 2: v <= 0 in place of v < 0 -- a zero tendency on a negative mass is "clipped": the applied -0.0 turns into +0.0
    bad = fm.apply(qdp, fq, dt, 0, plant="le")
    diff = _bits(bad["applied"]) != _bits(res["applied"])
    assert diff.any() and set(np.unique(fam[diff])) == {7}
    # 3: a contracted fma(dt, FQ, Qdp) on a sample of families 0 and 1 (no clip there: the result is the sum itself)
    idx = np.flatnonzero((fam.reshape(-1) == 0) | (fam.reshape(-1) == 1))[:4000]
    fused = fm.fma_contracted(dt, fq.reshape(-1)[idx], qdp.reshape(-1)[idx])
    differs = _bits(fused) != _bits(res["new"].reshape(-1)[idx])
    assert differs.mean() >= 0.01, differs.mean()
    assert (np.abs(fused - res["new"].reshape(-1)[idx]) <= np.spacing(np.abs(fused))).all()
    # 4: the budget leaves out the withheld part
    b = fm.budget(spheremp, res)
    bad = fm.budget(spheremp, res, plant="no_withheld")
    assert _same(bad[:, :, 0], b[:, :, 0]) and (_bits(bad[:, :, 1]) != _bits(b[:, :, 1])).all()


def test_fma_emulation_rounds_once():
    """the rational route of fma_contracted against a case worked by hand: 2^-53 * 2^-53 + 1 is 1 after one rounding, and
    (1 + 2^-52) * (1 + 2^-52) - (1 + 2^-51) = 2^-104 survives a single rounding where two roundings give 0"""
    a = 1.0 + 2.0 ** -52
    fd = Fraction(a) * Fraction(a) + Fraction(-(1.0 + 2.0 ** -51))
    assert float(fd) == 2.0 ** -104 and a * a + -(1.0 + 2.0 ** -51) == 0.0
    got = fm.fma_contracted(a, np.array([a]), np.array([-(1.0 + 2.0 ** -51)]))
    assert got[0] == 2.0 ** -104


# ---- the layouts of the GPU test -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [72, 64, 80])
@pytest.mark.parametrize("qsize", [1, 3, 4])
def test_view_plan_gives_the_expected_path(nlev, qsize):
    import view_model as vm
    rows = fm.layouts(24, qsize, nlev)
    assert [r[4] for r in rows] == [0, 0, 0, 1, 1, 2, 0, 0, 1]
    for label, strides, size, base, path, const in rows:
        p = view_plan("qdp", 24, qsize, strides, nlev=nlev)
        assert p["path"] == path, (label, p)
        off = vm.offsets("qdp", 24, qsize, nlev, strides) + base
        assert p["lo"] + base == off.min() and p["hi"] + base == off.max() + 1, label
        assert off.min() >= 0 and off.max() < size, label
