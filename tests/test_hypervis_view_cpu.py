"""tse_hypervis_view without a GPU: the entries in the header, the symbol list, the product libraries and the Fortran seam; the model the
GPU tests rest on (hypervis_model) against the reference's own biharmonics of tests/golden/ref_ne2_fieldops.npz continued in longdouble;
the planted errors; tse_hypervis_view_plan (paths, footprints and every refusal that needs no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dss_view_model as dm
import elem_ops_ld as ld
import fieldops_ref as fr
import hypervis_model as hm
from conftest import record_margin
from transport_se_amd import _lib
from transport_se_amd.hip_mod import TseError, hypervis_view_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tse_hypervis_view", "tse_hypervis_view_plan")
E = 24
BASE = 1 << 20   # a made-up address: the plan never touches memory
COEF = (-3.1e21, -1.7e21, -7.3e20)   # two scalar fields and the wind: distinct, no powers of two (-nu * dt / hypervis_subcycle of a host)


def test_entries_are_declared_listed_and_exported_by_every_product_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()) for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    assert decl["tse_hypervis_view"] == ("int tse_hypervis_view(tse_ctx *ctx, int nf, int nk, const double *coef, double nu_ratio, const tse_view *s, "
                                         "const tse_view *v, const tse_view *s_out, const tse_view *v_out, void *stream);")
    assert decl["tse_hypervis_view_plan"] == ("int tse_hypervis_view_plan(int nelemd, int nf, int nk, const tse_view *s, const tse_view *v, "
                                              "const tse_view *s_out, const tse_view *v_out, int path[4], long long lo[4], long long hi[4]);")
    for name in NAMES:
        assert name in _lib.SYMBOLS, name
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
        L = _lib.lib(nlev=nlev)
        assert not [n for n in NAMES if not hasattr(L, n)], nlev
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    assert re.search(r"subroutine\s+hypervis_view_hip\s*\(", src) and re.search(r"public\s*::[^\n]*\bhypervis_view_hip\b", src)
    assert "name='tse_hypervis_view'" in src


def test_timer_group_names_do_not_match_each_other():
    """tse_kernel_time matches a name against every group it is a prefix of"""
    others = ("dss", "lap", "view", "level", "fielddss", "fieldlap", "fieldremap", "remap", "advance", "minmax", "forcing", "stateq", "fieldvlap", "fieldop",
              "fieldstats", "fieldcol", "comm")
    assert not any("fieldhv".startswith(g) or g.startswith("fieldhv") for g in others)


# ---- the model against the reference ------------------------------------------------------------------------------------------
needs_ld = pytest.mark.skipif(not ld.has_extended_precision(), reason="needs an 80-bit longdouble")


@pytest.fixture(scope="module")
def ctx(gold):
    st, fx = gold("ref_ne2_static.npz"), gold("ref_ne2_fieldops.npz")
    st = {k: st[k] for k in st.files}
    fx = {k: fx[k] for k in fx.files}
    o = fr.mesh(st)
    yield o, (st["D"], fx["metinv"], st["mp"]), fx, fr.cases(fx)
    o.close()


def _state(fx):
    """two scalar fields -- the fixture's scalar and its averaged twin -- and the fixture's wind, three levels each"""
    s = np.ascontiguousarray(np.concatenate([fx["s"], fx["dss_average"]], axis=1))
    assert s.shape == (E, 2, 3, 4, 4) and fx["v"].shape == (E, 2, 3, 4, 4)
    return s, np.ascontiguousarray(fx["v"])


@needs_ld
def test_model_and_reference_lie_under_the_bound(ctx):
    """ratio <= 1 with N = the biharmonic case's count + hypervis_model.N_AFTER, for every nu_ratio of the fixture: (a) the fp64 model
    against its own longdouble chain, two scalar fields and the wind; (b) the REFERENCE's scalar and vector biharmonic (fixture keys
    bih, vbih_nu*), continued in longdouble with coef, the weak node sum and the addition, against the same chain -- the reference lies
    under the biharmonic's bound, and exact steps behind it carry that bound along; (c) the model against (b)'s values, under the sum
    of both.  Measured: worst ratio (a) 0.018 scalars, 0.013 wind; (b) 0.003, 0.005."""
    o, geo, fx, cases = ctx
    s, v = _state(fx)
    worst = {}
    for i, nu in enumerate(fx["nu_ratio"]):
        nu = float(nu)
        new_s, new_v, _, _ = hm.fp64(o, geo, s, v, COEF, nu)
        (rs, As), (rv, Av) = hm.longdouble(o, geo, s, v, COEF, nu)
        for key, got, ref, A, wind in (("scalars", new_s, rs, As, False), ("wind", new_v, rv, Av, True)):
            r = float(hm.ratio(got, ref, A, wind).max())
            worst[("a", key)] = max(worst.get(("a", key), 0.0), r)
            assert r <= 1.0, (key, nu, r)
        # the reference's own biharmonics: field 0 of s is the fixture's scalar
        cb, cv = cases["bih"], cases["vbih_nu%d" % i]
        assert cb.N + hm.N_AFTER == hm.steps(False) and cv.N + hm.N_AFTER == hm.steps(True)
        for key, x, c, ref, A, fac, wind in (("scalars", fx["s"], cb, rs[:, :1], As[:, :1], np.full((1, 1, 1, 1, 1), COEF[0]), False),
                                             ("wind", v, cv, rv, Av, np.full((1, 2, 1, 1, 1), COEF[2]), True)):
            _, Ab = c.ld(o, geo, fx[c.src], None)
            cont, _ = hm.continue_ld(o, x, fx[c.out], Ab, fac)
            r = float(hm.ratio(cont, ref, A, wind).max())
            worst[("b", key)] = max(worst.get(("b", key), 0.0), r)
            assert r <= 1.0, (key, nu, r)
            got = (new_s[:, :1] if key == "scalars" else new_v)
            assert float(fr.ratio(got, cont, 2.0 * A, hm.steps(wind)).max()) <= 1.0, (key, nu)
    for (part, key), r in sorted(worst.items()):
        print("hypervis model (%s) %s: worst error / bound(%d, A) = %.3f" % (part, key, hm.steps(key == "wind"), r))
        record_margin("hypervis %s (%s) / bound" % (key, part), r, 1.0)


@needs_ld
def test_planted_errors_break_the_bound(ctx):
    """coef[f] applied to field f + 1, the wind's factor applied to the scalars, the final rspheremp dropped: each beyond the bound"""
    o, geo, fx, _ = ctx
    s, v = _state(fx)
    new_s, new_v, _, _ = hm.fp64(o, geo, s, v, COEF, 2.5)
    for plant in hm.PLANTS:
        (bs, As), (bv, Av) = hm.longdouble(o, geo, s, v, COEF, 2.5, plant)
        rs, rv = float(hm.ratio(new_s, bs, As, False).max()), float(hm.ratio(new_v, bv, Av, True).max())
        print("hypervis planted %s: worst ratio scalars %.3g, wind %.3g" % (plant, rs, rv))
        assert rs > 1.0, (plant, rs)
        assert (rv > 1.0) == (plant == "no_rspheremp"), (plant, rv)      # the factor plants touch the scalars alone


def test_model_algebra():
    """the model's own identities, bit for bit: a zero factor leaves its field, a factor times 2^k scales the tendency exactly, an
    absent half does not change the other"""
    import pyoracle as po
    import vlaplace_model as vm
    o = po.Oracle(2, 1)
    geo = vm.host_fields(o)
    s, v = hm.bm.random_field(o.nelem, 2, 2, seed=1), vm.random_field(o.nelem, 2, seed=1)
    a = hm.fp64(o, geo, s, v, COEF)
    z = hm.fp64(o, geo, s, v, (COEF[0], 0.0, COEF[2]))
    assert dm.same(z[0][:, 1], s[:, 1]) and dm.same(z[0][:, 0], a[0][:, 0]) and dm.same(z[1], a[1])
    k = hm.fp64(o, geo, s, v, (COEF[0] * 8.0, COEF[1], COEF[2] / 4.0))
    assert dm.same(k[2][:, 0], a[2][:, 0] * 8.0) and dm.same(k[2][:, 1], a[2][:, 1]) and dm.same(k[3], a[3] / 4.0)
    only = hm.fp64(o, geo, s, None, COEF)
    assert only[1] is None and dm.same(only[0], a[0])
    assert dm.same(hm.fp64(o, geo, None, v, COEF[2:])[1], a[1])
    o.close()


# ---- tse_hypervis_view_plan ---------------------------------------------------------------------------------------------------
def _sizes(nf, nk):
    return E * nf * nk * 16


@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_plan_paths_and_footprints(nlev):
    nf = 3
    seen = set()
    for nk in (1, 3, nlev, nlev + 1):
        ls = {name: dm.layout(name, E, nf, nk) for name in dm.LAYOUTS}
        lv = {name: dm.layout(name, E, 2, nk) for name in dm.LAYOUTS}
        for i, name in enumerate(dm.LAYOUTS):
            other = dm.LAYOUTS[(i + 3) % len(dm.LAYOUTS)]
            # strides alone, in place
            got = hypervis_view_plan(E, nf, nk, ls[name][0], lv[other][0], nlev=nlev)
            assert got["s_out"] is None and got["v_out"] is None
            assert got["s"]["path"] == dm.expected_path(name, nk, nlev) and got["v"]["path"] == dm.expected_path(other, nk, nlev), (name, other, nk, got)
            assert (got["s"]["lo"], got["s"]["hi"]) == dm.footprint(name, E, nf, nk) and (got["v"]["lo"], got["v"]["hi"]) == dm.footprint(other, E, 2, nk)
            seen.add((got["s"]["path"], got["v"]["path"]))
            # four views behind one another in one made-up allocation
            at, views = BASE, []
            for lay in (ls[name], lv[other], ls[other], lv[name]):
                views.append((lay[0], at)); at += 8 * lay[2]
            got = hypervis_view_plan(E, nf, nk, *views, nlev=nlev)
            assert [got[k]["path"] for k in ("s", "v", "s_out", "v_out")] == [dm.expected_path(n, nk, nlev) for n in (name, other, other, name)]
            # a half alone
            assert hypervis_view_plan(E, 0, nk, None, lv[name][0], nlev=nlev)["s"] is None
            assert hypervis_view_plan(E, nf, nk, ls[name][0], None, nlev=nlev)["v"] is None
    assert {a for a, _ in seen} == {b for _, b in seen} == {0, 1, 2}
    # E3SM: T and dp3d two members of elem(:) at one element stride -> one s view whose q stride is their distance; state%v(np,np,2,nlev,tl)
    es, dist = 40 * 16 * nlev, 7 * 16 * nlev
    got = hypervis_view_plan(E, 2, nlev, [es, dist, 16, 4, 1], [es, 16, 32, 4, 1], nlev=nlev)
    assert got["s"] == dict(path=0, lo=0, hi=(E - 1) * es + dist + 16 * nlev) and got["v"] == dict(path=0, lo=0, hi=(E - 1) * es + 32 * nlev)


def test_plan_refusals():
    nlev, nf = 72, 2
    plane = nlev * 16
    ds, dv = [nf * plane, plane, 16, 4, 1], [2 * plane, plane, 16, 4, 1]
    n = _sizes(2, nlev)
    S, V, SO, VO = (ds, BASE), (dv, BASE + 8 * n), (ds, BASE + 16 * n), (dv, BASE + 24 * n)
    assert [hypervis_view_plan(E, nf, nlev, S, V, SO, VO)[k]["path"] for k in ("s", "v", "s_out", "v_out")] == [0, 0, 0, 0]
    # presence
    for args, text in (((0, nlev, None, None), "neither scalar fields"), ((0, nlev, S, V), "nf = 0 takes no view s"), ((2, nlev, None, V), "nf = 2 needs the view s"),
                       ((-1, nlev, None, V), "nf = -1"), ((65, nlev, S, V), "nf = 65"),
                       ((nf, nlev, S, V, SO, None), "v is given and v_out is not"), ((nf, nlev, S, V, None, VO), "s is given and s_out is not"),
                       ((nf, nlev, S, None, SO, VO), "v_out is given and v is not"), ((0, nlev, None, V, SO, VO), "s_out is given and s is not"),
                       ((nf, 0, S, V), "nk = 0"), ((nf, nlev + 2, S, V), "nk = %d" % (nlev + 2))):
        with pytest.raises(TseError, match="tse_hypervis_view: " + text):
            hypervis_view_plan(E, *args)
    # the rules of a view of tse_dss_view for every one of the four, the view named
    roles = ("s", "v", "s_out", "v_out")
    for i, role in enumerate(roles):
        good = [S, V, SO, VO]
        dense = ds if i % 2 == 0 else dv

        def plan(bad):
            views = list(good); views[i] = (bad, good[i][1])
            return hypervis_view_plan(E, nf, nlev, *views)
        for axis, word in enumerate(("element", "q", "level", "j", "i")):
            z = list(dense); z[axis] = 0
            with pytest.raises(TseError, match=r"tse_hypervis_view.*stride 0 on the %s axis.*\(%s\)" % (word, role)):
                plan(z)
        with pytest.raises(TseError, match=r"overlap itself.*\(%s\)" % role):
            plan([dense[0], plane // 2, 16, 4, 1])
    # overlap: every pair of the four
    at = [BASE, BASE + 8 * n, BASE + 16 * n, BASE + 24 * n]
    for i in range(4):
        for j in range(i + 1, 4):
            for off in (8, 8 * (n - 1)):                                 # one slab's worth inside, one double shared
                a = list(at); a[j] = a[i] + off
                views = [((ds if k % 2 == 0 else dv), a[k]) for k in range(4)]
                with pytest.raises(TseError, match=r"tse_hypervis_view: %s .* overlaps %s " % (roles[j], roles[i])):
                    hypervis_view_plan(E, nf, nlev, *views)
    with pytest.raises(TseError, match="v .* overlaps s "):              # in place: s and v are both written
        hypervis_view_plan(E, nf, nlev, S, (dv, BASE + 8 * (n - 16)))
    assert hypervis_view_plan(E, nf, nlev, S, (dv, BASE - 8 * n))["v"]["path"] == 0   # touching is disjoint
    # members of one elem(:) interleave: the same element stride, footprints within an element disjoint and inside one stride
    es = 40 * plane
    T_dp, wind = [es, 7 * plane, 16, 4, 1], [es, 16, 32, 4, 1]
    got = hypervis_view_plan(E, 2, nlev, (T_dp, BASE), (wind, BASE + 8 * 12 * plane))
    assert got["s"]["hi"] > 12 * plane and got["v"]["path"] == 0
    hypervis_view_plan(E, 2, nlev, (T_dp, BASE), (wind, BASE + 8 * 8 * plane))                  # v right behind dp3d
    hypervis_view_plan(E, 2, nlev, (T_dp, BASE), (wind, BASE + 8 * 38 * plane))                 # ... and ending with the element
    for at in (7 * plane, 8 * plane - 1, 38 * plane + 1, 39 * plane):                           # v inside dp3d; reaching into the next element's T
        with pytest.raises(TseError, match="v .* overlaps s "):
            hypervis_view_plan(E, 2, nlev, (T_dp, BASE), (wind, BASE + 8 * at))
    with pytest.raises(TseError, match="v .* overlaps s "):                                      # another element stride: footprints alone decide
        hypervis_view_plan(E, 2, nlev, (T_dp, BASE), ([es + 16, 16, 32, 4, 1], BASE + 8 * 12 * plane))
    # the size rule: nelemd * (nf + 2) * nk layers
    big = 1 << 21
    with pytest.raises(TseError, match=r"tse_hypervis_view: %d elements x %d layers" % (big, 64)):
        hypervis_view_plan(big, 62, 1, [62 * 16, 16, 0, 4, 1], [32, 16, 0, 4, 1])
    assert hypervis_view_plan(big, 61, 1, [61 * 16, 16, 0, 4, 1], [32, 16, 0, 4, 1])["s"]["path"] == 0
    # refused before any device call
    L = _lib.lib()
    c = (C.c_double * 3)(1.0, 1.0, 1.0)
    assert L.tse_hypervis_view(None, 2, nlev, c, 1.0, None, None, None, None, None) != 0 and b"null context" in L.tse_last_error()
    assert L.tse_hypervis_view_plan(E, 2, nlev, None, None, None, None, None, None, None) != 0 and b"needs the view s" in L.tse_last_error()
