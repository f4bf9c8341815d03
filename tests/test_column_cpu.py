"""tse_column_view without a GPU: the numpy model of the three vertical scans (tests/column_model.py) against its longdouble referee
within the bounds its docstring derives, the identities that tie it to the physics, six planted errors, and tse_column_view_plan: paths,
footprints and every refusal that needs no device.

The reference carries preq_hydrostatic (src/asp_tests.F90:1708-1757) and no preq_omega_ps; no fixture made by it exists for these ops,
so the model is held to the definition by the identities below and shown to see the plants."""
import math

import numpy as np
import pytest

import column_model as cm
import stats_layouts as sl

N, NCOL = 72, 4000
LAYOUTS = ("dense", "dense_odd8", "dense_odd_e", "dense_odd_k", "lev0", "lev_even", "lev_odd", "ij")
LD = np.longdouble


@pytest.fixture(scope="module")
def fam():
    f = cm.family(N, NCOL)
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


def _cases(f):
    """(label, op, views): every op, PHI and OMEGA with the pressure formed and with one given (an Eulerian one: no prefix sum)"""
    pe = cm.pmid(f["dp"], f["ptop"]) * (1.0 + 1e-3 * np.sin(np.arange(N))[:, None])
    out = [(op, op, cm.views_of(op, f)) for op in cm.OPS]
    out += [(op + "(p)", op, cm.views_of(op, f, p=pe)) for op in ("phi", "omega")]
    return out


def test_the_model_lies_under_its_bounds(fam):
    worst = {}
    for label, op, views in _cases(fam):
        got = cm.model(op, fam["ptop"], fam["rgas"], **views)
        ref = cm.referee(op, fam["ptop"], fam["rgas"], **views)
        bnd = cm.bound(op, fam["ptop"], fam["rgas"], **views)
        assert got.dtype == np.float64 and ref.dtype == LD and bnd.shape == got.shape
        err = np.abs(got.astype(LD) - ref)
        assert (bnd[err > 0] > 0).all()
        ratio = float(np.max(np.where(err > 0, err / np.where(bnd > 0, bnd, 1), 0)))
        worst[label] = ratio
        print("column_model: worst |model - referee| / bound, %-9s %.4f" % (label, ratio))
    assert all(0 < r < 1 for r in worst.values()), worst


def test_identities(fam):
    ptop, rgas = fam["ptop"], fam["rgas"]
    ld = lambda x: np.asarray(x).astype(LD)
    dp, tv, phis = ld(fam["dp"]), ld(fam["tv"]), ld(fam["phis"])
    eps = LD(2.0) ** -64
    # phi[k] - phi[k+1] = rgas * (T[k] hkk[k] + T[k+1] hkk[k+1])
    p = cm.pmid(dp, ptop)
    ph = cm.phi(tv, dp, phis, rgas, ptop=ptop)
    hkk = (dp * LD(0.5)) / p
    rhs = LD(rgas) * (tv[:-1] * hkk[:-1] + tv[1:] * hkk[1:])
    assert np.max(np.abs((ph[:-1] - ph[1:]) - rhs)) <= 8 * N * eps * np.max(np.abs(ph))
    # an isothermal column: phi - phis -> rgas T ln(ps / p), second order as the levels are halved
    T0, pt, ps = LD(250.0), LD(2.0e4), LD(1.0e5)
    errs = []
    for n in (36, 72, 144):
        d = np.full((n, 1), (ps - pt) / n, dtype=LD)
        pm = cm.pmid(d, pt)
        got = cm.phi(np.full((n, 1), T0), d, np.zeros(1, dtype=LD), rgas, ptop=pt)
        errs.append(float(np.max(np.abs(got - LD(rgas) * T0 * np.log(ps / pm)))))
    # the error is C h^2 (1 + O(h)) with h = dp / p, 0.06 at the top of the 36-level column: the ratios approach 4 from nearby
    r1, r2 = errs[0] / errs[1], errs[1] / errs[2]
    assert 3.5 < r1 < 4.5 and 3.5 < r2 < 4.5 and abs(r2 - 4) < abs(r1 - 4), errs
    # vgrad_p = 0, divdp = c dp: omega[k] = -c (p[k] - ptop) / p[k]
    c = 3.0e-6
    div64 = c * fam["dp"]
    closed = -LD(c) * (p - LD(ptop)) / p
    ref = cm.omega(np.zeros_like(dp), LD(c) * dp, dp=dp, ptop=ptop)
    assert np.max(np.abs(ref - closed) / np.abs(closed)) <= 8 * N * eps
    views = dict(dp=fam["dp"], a=np.zeros_like(fam["dp"]), b=div64)
    got = cm.model("omega", ptop, rgas, **views)
    assert (np.abs(got.astype(LD) - closed) <= cm.bound("omega", ptop, rgas, **views) + 2 * LD(cm.U) * np.abs(closed)).all()
    # pi[n] - ptop = sum dp, and p[k] = (pi[k] + pi[k+1]) / 2, both to the bounds
    pi64, p64 = cm.model("pint", ptop, rgas, dp=fam["dp"]), cm.model("pmid", ptop, rgas, dp=fam["dp"])
    bi, bm = cm.bound("pint", ptop, rgas, dp=fam["dp"]), cm.bound("pmid", ptop, rgas, dp=fam["dp"])
    total = np.array([math.fsum(col) for col in fam["dp"].T])
    assert (np.abs((pi64[N].astype(LD) - LD(ptop)) - total.astype(LD)) <= bi[N] + LD(cm.U) * total).all()
    assert (np.abs(p64.astype(LD) - (pi64[:-1].astype(LD) + pi64[1:].astype(LD)) / 2) <= bm + (bi[:-1] + bi[1:]) / 2).all()


PLANTED = (("hkk_for_hkl", "phi"), ("half_dropped", "pmid"), ("pint_for_pmid", "phi"), ("phii_shifted", "phi"), ("s_early", "omega"),
           ("reversed", "pint"), ("reversed", "phi"), ("reversed", "omega"))


def test_planted_errors_are_seen(fam):
    """each wrong version, in fp64, leaves the referee by many times the bound"""
    assert {p for p, _ in PLANTED} == set(cm.PLANTS) and len(cm.PLANTS) >= 6
    for plant, op in PLANTED:
        views = cm.views_of(op, fam)
        bad = cm.run(op, np.float64, fam["ptop"], fam["rgas"], plant=plant, **views)
        ref = cm.referee(op, fam["ptop"], fam["rgas"], **views)
        bnd = cm.bound(op, fam["ptop"], fam["rgas"], **views)
        assert not cm.same(bad, cm.model(op, fam["ptop"], fam["rgas"], **views))
        factor = float(np.max(np.abs(bad.astype(LD) - ref) / np.where(bnd > 0, bnd, np.inf)))
        print("column_model: planted %-14s in %-5s  %.3g x the bound" % (plant, op, factor))
        assert factor > 100.0, (plant, op, factor)


# ---- the plan ----
def _plan(*a, **k):
    from transport_se_amd.hip_mod import column_view_plan
    return column_view_plan(*a, **k)


def _views(op, name, other, E, nlev, surface=None):
    """strides of the views of one op: `name` for out, `other` for every input"""
    nko = nlev + 1 if op == "pint" else nlev
    v = dict(out=sl.layout(name, E, 1, nko)[0])
    lay = sl.layout(other, E, 1, nlev)[0]
    if op in ("pint", "pmid"):
        v.update(dp=lay)
    elif op == "phi":
        v.update(dp=lay, p=lay, a=lay, b=surface or [16, 0, 0, 4, 1])
    else:
        v.update(p=lay, a=lay, b=lay)
    return v


@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_plan_paths_and_footprints(nlev):
    E = 24
    other = dict(zip(LAYOUTS, LAYOUTS[3:] + LAYOUTS[:3]))
    seen = set()
    for op in cm.OPS:
        nko = nlev + 1 if op == "pint" else nlev
        for name in LAYOUTS:
            v = _views(op, name, other[name], E, nlev)
            plan = _plan(E, op, nlev=nlev, **v)
            assert plan["out"] == dict(path=sl.expected_path(name, nko, nlev), lo=0, hi=sl.footprint(name, E, 1, nko)[1]), (op, name, plan)
            for role in ("dp", "p", "a", "b"):
                if role not in v:
                    assert plan[role] is None
                elif role == "b" and op == "phi":
                    assert plan[role] == dict(path=0, lo=0, hi=(E - 1) * 16 + 16)
                else:
                    assert plan[role] == dict(path=sl.expected_path(other[name], nlev, nlev), lo=0, hi=sl.footprint(other[name], E, 1, nlev)[1]), (op, name, role)
            seen.add((op, plan["out"]["path"]))
    assert {p for o, p in seen if o == "pint"} == {0, 2} and all({p for o, p in seen if o == x} == {0, 1, 2} for x in cm.OPS[1:])
    # surface layouts of phis: [e][j][i]; the last level of a level-fastest array, with the level stride left at 1 and at 0; one level
    # of a point-fastest array
    S = nlev + 2
    for strides, path, hi in (([16, 0, 0, 4, 1], 0, (E - 1) * 16 + 16), ([16 * S, 0, 1, 4 * S, S], 2, (E - 1) * 16 * S + 15 * S + 1),
                              ([16 * S, 0, 0, 4 * S, S], 2, (E - 1) * 16 * S + 15 * S + 1), ([16 * nlev, 7, 16, 4, 1], 0, (E - 1) * 16 * nlev + 16)):
        plan = _plan(E, "phi", nlev=nlev, **_views("phi", "dense", "lev0", E, nlev, surface=strides))
        assert plan["b"] == dict(path=path, lo=0, hi=hi), (strides, plan["b"])
        assert plan["p"]["path"] == 1 and plan["out"]["path"] == 0


def test_plan_refusals():
    from transport_se_amd.hip_mod import TseError
    E, nlev = 24, 72
    d = sl.layout("dense", E, 1, nlev)[0]
    d1 = sl.layout("dense", E, 1, nlev + 1)[0]
    surf = [16, 0, 0, 4, 1]
    for op in (-1, 4):
        with pytest.raises(TseError, match="op=%d" % op):
            _plan(E, op, dp=d, out=d)
    # the table of views: (op, views, what the message names)
    table = [
        ("pint", dict(out=d1), "needs the view dp"), ("pint", dict(dp=d), "needs the view out"), ("pint", dict(dp=d, out=d1, p=d), "takes no view p"),
        ("pint", dict(dp=d, out=d1, a=d), "takes no view a"), ("pmid", dict(dp=d, out=d, b=d), "takes no view b"), ("pmid", dict(out=d), "needs the view dp"),
        ("phi", dict(p=d, a=d, b=surf, out=d), "needs the view dp"), ("phi", dict(dp=d, b=surf, out=d), "needs the view a"),
        ("phi", dict(dp=d, a=d, out=d), "needs the view b"), ("phi", dict(dp=d, a=d, b=surf), "needs the view out"),
        ("omega", dict(a=d, b=d, out=d), "needs the view dp when p is null"), ("omega", dict(dp=d, p=d, a=d, b=d, out=d), "takes no view dp beside p"),
        ("omega", dict(p=d, b=d, out=d), "needs the view a"), ("omega", dict(p=d, a=d, out=d), "needs the view b"),
    ]
    for op, views, text in table:
        with pytest.raises(TseError, match="tse_column_view: TSE_COL_%s %s" % (op.upper(), text)):
            _plan(E, op, **views)
    # accepted: every row of the table
    for op, views in (("pint", dict(dp=d, out=d1)), ("pmid", dict(dp=d, out=d)), ("phi", dict(dp=d, a=d, b=surf, out=d)), ("phi", dict(dp=d, p=d, a=d, b=surf, out=d)),
                      ("omega", dict(dp=d, a=d, b=d, out=d)), ("omega", dict(p=d, a=d, b=d, out=d))):
        _plan(E, op, **views)
    # strides
    with pytest.raises(TseError, match=r"stride 0 on the j axis.*\(out\)"):
        _plan(E, "pmid", dp=d, out=[d[0], 0, 16, 0, 1])
    with pytest.raises(TseError, match=r"stride 0 on the level axis.*\(out\)"):
        _plan(E, "pmid", dp=d, out=[d[0], 0, 0, 4, 1])
    with pytest.raises(TseError, match=r"overlap itself.*\(out\)"):
        _plan(E, "pmid", dp=d, out=[d[0] // 2, 0, 16, 4, 1])
    with pytest.raises(TseError, match=r"stride 0 on the level axis.*\(dp\)"):
        _plan(E, "pmid", dp=[d[0], 0, 0, 4, 1], out=d)
    with pytest.raises(TseError, match=r"stride 0 on the element axis.*\(b\)"):
        _plan(E, "phi", dp=d, a=d, b=[0, 0, 0, 4, 1], out=d)
    with pytest.raises(TseError, match="nelemd = 0"):
        _plan(0, "pmid", dp=d, out=d)
    # out overlapping each input in turn: (strides, address) pairs in one address space; touching is disjoint
    size = E * nlev * 16 * 8
    base = 1 << 30
    place = dict(dp=base, p=base + 2 * size, a=base + 4 * size, b=base + 6 * size)
    for op, roles in (("pmid", ("dp",)), ("pint", ("dp",)), ("phi", ("dp", "p", "a", "b")), ("omega", ("dp", "a", "b")), ("omega", ("p", "a", "b"))):
        lay = lambda r: surf if (op == "phi" and r == "b") else d
        views = {r: (lay(r), place[r]) for r in roles}
        do = d1 if op == "pint" else d
        osize = (nlev + 1 if op == "pint" else nlev) * E * 16 * 8
        _plan(E, op, out=(do, base + 8 * size), **views)
        for r in roles:
            rsize = E * 16 * 8 if lay(r) is surf else size
            for addr in (place[r], place[r] + rsize - 8, place[r] - osize + 8):
                with pytest.raises(TseError, match=r"out \[.*overlaps %s \[" % r):
                    _plan(E, op, out=(do, addr), **views)
            if r == roles[-1]:
                _plan(E, op, out=(do, place[r] + rsize), **views)
                _plan(E, op, out=(do, place[r] - osize), **views)
    # strides alone: nothing is known of where the views lie
    _plan(E, "pmid", dp=d, out=d)


def test_abi_seam_and_timer_group():
    """the two symbols in every library, the wrapper in the Fortran seam, and a timer group no other group is a prefix of"""
    import os
    import re
    from transport_se_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "transport_se_hip.h")).read()
    for i, name in enumerate(("PINT", "PMID", "PHI", "OMEGA")):
        assert re.search(r"#define\s+TSE_COL_%s\s+%d\b" % (name, i), text)
    for name in ("tse_column_view", "tse_column_view_plan"):
        assert name in _lib.SYMBOLS and re.search(r"\bint %s\(" % name, text), name
        for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
            assert hasattr(_lib.lib(nlev=nlev), name), (name, nlev)
    src = open(os.path.join(root, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    assert re.search(r"subroutine\s+column_view_hip\s*\(", src) and re.search(r"public\s*::[^\n]*\bcolumn_view_hip\b", src)
    assert "name='tse_column_view'" in src
    groups = [g for unit, _ in _lib.UNITS if unit.endswith(".hip")   # every HIP unit: the view entries have one of their own
              for g in re.findall(r'Scope \w+\(c, "([a-z0-9_]+)"', open(os.path.join(root, "transport_se_amd", "csrc", unit)).read())]
    assert "fieldcol" in groups
    for g in set(groups) - {"fieldcol"}:
        assert not g.startswith("fieldcol") and not "fieldcol".startswith(g), g
