"""tse_stats_view without a GPU: the entries in the header, the symbol list, the product libraries and the Fortran seam; tse_stats_view_plan
(csrc/tse_views.cpp: paths, footprints, refusals); the model the GPU comparison rests on (tests/stats_model.py), held to an exact referee
within the bound that file derives, shown to see five planted errors; diagnostics.stats_from_partials and the prim_printstate lines."""
import math
import os
import re

import numpy as np
import pytest

import dss_view_model as dm
import stats_model as sm
from transport_se_amd import _lib, diagnostics as dg
from transport_se_amd.hip_mod import TseError, stats_view_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 24
GEOM_U = 4 * sm.U   # how far the fixture's own area is from 4 pi (test_the_fixture_geometry)


def test_entries_are_declared_listed_and_exported_by_every_product_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()) for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    assert decl["tse_stats_view"] == ("int tse_stats_view(tse_ctx *ctx, int nf, int nk, int per_level, const tse_view *field, const tse_view *ref , "
                                      "const tse_view *weight , void *stream, double *out );")
    assert decl["tse_stats_view_plan"] == ("int tse_stats_view_plan(int nelemd, int nf, int nk, const tse_view *field, const tse_view *ref, "
                                           "const tse_view *weight, int path[3], long long lo[3], long long hi[3]);")
    assert re.search(r"#define\s+TSE_STATS\s+16\b", text)
    for name in ("tse_stats_view", "tse_stats_view_plan"):
        assert name in _lib.SYMBOLS, name
        for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
            assert hasattr(_lib.lib(nlev=nlev), name), (name, nlev)
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    assert re.search(r"subroutine\s+stats_view_hip\s*\(", src) and re.search(r"public\s*::[^\n]*\bstats_view_hip\b", src)
    assert "name='tse_stats_view'" in src
    # the timer group: no existing group is a prefix of it and it is a prefix of none
    groups = [g for unit, _ in _lib.UNITS if unit.endswith(".hip")   # every HIP unit: the view entries have one of their own
              for g in re.findall(r'Scope \w+\(c, "([a-z0-9_]+)"', open(os.path.join(ROOT, "transport_se_amd", "csrc", unit)).read())]
    assert "fieldstats" in groups
    for g in set(groups) - {"fieldstats"}:
        assert not g.startswith("fieldstats") and not "fieldstats".startswith(g), g


# ---- tse_stats_view_plan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_plan_paths_and_footprints(nlev):
    """every layout of tests/test_dss_view_cpu.py on the field, and a different one on ref and weight: each view its own path"""
    seen = set()
    other = {"dense": "lev_even", "epad": "ij", "lev0": "dense", "lev_even": "ij", "lev_odd": "epad", "ij": "lev0", "dense_odd8": "lev_odd", "lev_odd8": "dense"}
    for nf in (1, 2, 5):
        for nk in (1, nlev, nlev + 1):
            for name in dm.LAYOUTS:
                fs, rs, ws = dm.layout(name, E, nf, nk)[0], dm.layout(other[name], E, nf, nk)[0], dm.layout(other[other[name]], E, 1, nk)[0]
                got = stats_view_plan(E, nf, nk, fs, rs, ws, nlev=nlev)
                want = [(dm.expected_path(name, nk, nlev), dm.footprint(name, E, nf, nk)),
                        (dm.expected_path(other[name], nk, nlev), dm.footprint(other[name], E, nf, nk)),
                        (dm.expected_path(other[other[name]], nk, nlev), dm.footprint(other[other[name]], E, 1, nk))]
                for g, (path, (lo, hi)) in zip(got, want):
                    assert g == dict(path=path, lo=lo, hi=hi), (name, nf, nk, got, want)
                    seen.add(path)
                assert stats_view_plan(E, nf, nk, fs, nlev=nlev) == [got[0], None, None]
                assert stats_view_plan(E, nf, nk, fs, None, ws, nlev=nlev) == [got[0], None, got[2]]
    assert seen == {0, 1, 2}
    # the weight's q stride is not looked at: a stride that would overlap, or zero
    dense = [2 * nlev * 16, nlev * 16, 16, 4, 1]
    for q in (0, 1, 7, nlev * 16):
        assert stats_view_plan(E, 2, nlev, dense, None, [nlev * 16, q, 16, 4, 1], nlev=nlev)[2] == dict(path=0, lo=0, hi=E * nlev * 16)


def test_plan_of_the_point_fastest_layouts_with_one_odd_stride():
    """tests/stats_layouts.py: path 0 and the footprint; the hooks library's view_wide says that a lane may not move 16 bytes there"""
    import ctypes as C
    import stats_layouts as sl
    H = C.CDLL(_lib.HOOKS_SO)
    H.tse_test_view_wide.argtypes = [C.c_int, C.POINTER(_lib.View)]
    for name in sl.ODD:
        for nf, nk in ((1, 3), (2, 72), (5, 73)):
            s_, base, size = sl.layout(name, E, nf, nk)
            got = stats_view_plan(E, nf, nk, s_)[0]
            assert base == 0 and got == dict(path=0, lo=0, hi=sl.footprint(name, E, nf, nk)[1]) and got["hi"] <= size
            v = _lib.View(1 << 20, (C.c_longlong * 5)(*s_))                   # a 16-byte aligned base
            assert H.tse_test_view_wide(0, C.byref(v)) == 0, (name, s_)
    v = _lib.View(1 << 20, (C.c_longlong * 5)(2 * 72 * 16, 72 * 16, 16, 4, 1))
    assert H.tse_test_view_wide(0, C.byref(v)) == 1


def test_plan_refusals():
    nlev, nf = 72, 2
    dense = [nf * nlev * 16, nlev * 16, 16, 4, 1]
    wdense = [nlev * 16, 0, 16, 4, 1]
    with pytest.raises(TseError, match="tse_stats_view: null view"):
        stats_view_plan(E, nf, nlev, None)
    with pytest.raises(TseError, match="tse_stats_view: nf = 0"):
        stats_view_plan(E, 0, nlev, dense)
    with pytest.raises(TseError, match="nk = 0"):
        stats_view_plan(E, nf, 0, dense)
    with pytest.raises(TseError, match="nk = %d" % (nlev + 2)):
        stats_view_plan(E, nf, nlev + 2, dense)
    with pytest.raises(TseError, match="nelemd = 0"):
        stats_view_plan(0, nf, nlev, dense)
    for axis, word in enumerate(("element", "q", "level", "j", "i")):     # a zero stride on an extent above 1, the axis and the view named
        z = list(dense); z[axis] = 0
        with pytest.raises(TseError, match=r"stride 0 on the %s axis.*\(field\)" % word):
            stats_view_plan(E, nf, nlev, z)
        with pytest.raises(TseError, match=r"stride 0 on the %s axis.*\(ref\)" % word):
            stats_view_plan(E, nf, nlev, dense, z)
        if axis != 1:
            z = list(wdense); z[axis] = 0
            with pytest.raises(TseError, match=r"stride 0 on the %s axis.*\(weight\)" % word):
                stats_view_plan(E, nf, nlev, dense, None, z)
    with pytest.raises(TseError, match=r"overlap itself.*q stride.*\(field\)"):
        stats_view_plan(E, nf, nlev, [nf * nlev * 16, nlev * 8, 16, 4, 1])
    with pytest.raises(TseError, match=r"overlap itself.*\(ref\)"):
        stats_view_plan(E, nf, nlev, dense, [nf * nlev * 16, nlev * 16, 2, 4, 1])
    with pytest.raises(TseError, match="out of range"):
        stats_view_plan(E, nf, nlev, [1 << 59, nlev * 16, 16, 4, 1])
    # an axis of extent 1 may carry stride 0: a surface field [e][j][i]
    assert stats_view_plan(E, 1, 1, [16, 0, 0, 4, 1])[0] == dict(path=0, lo=0, hi=E * 16)
    # the views may overlap each other: the same view three times
    assert stats_view_plan(E, 1, nlev, wdense, wdense, wdense) == [dict(path=0, lo=0, hi=E * nlev * 16)] * 3
    L = _lib.lib()
    assert L.tse_stats_view(None, 1, 1, 0, None, None, None, None, None) != 0 and b"null context" in L.tse_last_error()   # (before any device call)


# ---- the model -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(gold):
    st, fo, dc = gold("ref_ne2_static.npz"), gold("ref_ne2_fieldops.npz"), gold("ref_ne2_dcmip11.npz")
    return dict(spheremp=st["spheremp"], mp=st["mp"], metdet=st["metdet"], s=fo["s"], v=fo["v"], grad=fo["grad"],
                ps=dc["ps_v_step3"][:, None, None], dp=dc["dp3d_step3"][:, None])


def _cases(fx):
    """name -> (h, ht, w): the fixtures' fields; the gradient as the 'true solution' of the wind, three layers of dp3d as a weight"""
    return {"s": (fx["s"], None, None), "v": (fx["v"], None, None), "v-grad": (fx["v"], fx["grad"], None),
            "s*dp": (fx["s"], None, fx["dp"][:, 0, 20:23]), "v-grad*dp": (fx["v"], fx["grad"], fx["dp"][:, 0, 20:23]),
            "ps": (fx["ps"], None, None), "dp3d": (fx["dp"], None, None)}


def test_the_fixture_geometry(fx):
    assert sm.same(fx["spheremp"], fx["mp"] * fx["metdet"])
    # the reference scales the metric so that the sphere's area is 4 pi: one quotient 4 pi / area, the factor carried into metdet, the
    # product mp * metdet -- a few roundings per value, so the exact sum of the stored spheremp is 4 pi within GEOM_U = 4 u
    area = math.fsum(fx["spheremp"].ravel().tolist()) / (4.0 * math.pi)
    assert abs(area - 1.0) <= GEOM_U and "%.15g" % area == "1", area


def test_model_within_the_bound_of_the_exact_referee(fx):
    worst = {}
    for name, (h, ht, w) in _cases(fx).items():
        nk = h.shape[2]
        for per_level in (False, True):
            got = sm.model(h, fx["spheremp"], ht, w, per_level=per_level)
            S, A = sm.exact_sums(h, fx["spheremp"], ht, w, per_level=per_level)
            r = sm.worst_ratio(got, S, sm.bound(A, nk, weight=w is not None, per_level=per_level))
            worst[(name, per_level)] = r
            assert r <= 1.0, (name, per_level, r)
            if ht is None:
                assert not got[..., 8:14].any()
            assert not got[..., 15].any()
    print("stats model: worst error / bound = %.3f (%s)" % (max(worst.values()), max(worst, key=worst.get)))


def test_extrema_and_count_are_numpy_s(fx):
    for name, (h, ht, w) in _cases(fx).items():
        x = h.reshape(h.shape[:3] + (16,))
        lev, el = sm.model(h, fx["spheremp"], ht, w, per_level=True), sm.model(h, fx["spheremp"], ht, w)
        assert sm.same(lev[..., 0], x.min(-1)) and sm.same(lev[..., 1], x.max(-1)) and sm.same(lev[..., 6], np.abs(x).max(-1))
        assert sm.same(el[..., 0], x.min((2, 3))) and sm.same(el[..., 1], x.max((2, 3))) and sm.same(el[..., 6], np.abs(x).max((2, 3)))
        assert not lev[..., 7].any() and not el[..., 7].any()
        if ht is not None:
            y = ht.reshape(x.shape)
            assert sm.same(el[..., 12], np.abs(x - y).max((2, 3))) and sm.same(el[..., 13], np.abs(y).max((2, 3)))
    # special values: the count is exact, the extrema skip the NaN, the sums of that slab are NaN and no other's
    h = fx["v"].copy()
    h[3, 1, 2, 1, 1] = np.nan; h[5, 0, 0, 0, 0] = np.inf; h[5, 0, 0, 3, 3] = -np.inf; h[7, 1, 1, 2, 0] = -0.0; h[9, 0, 1] = np.nan
    lev = sm.model(h, fx["spheremp"], per_level=True)
    want = np.zeros(h.shape[:3]); want[3, 1, 2] = 1; want[5, 0, 0] = 2; want[9, 0, 1] = 16
    assert np.array_equal(lev[..., 7], want)
    x = h.reshape(h.shape[:3] + (16,))
    assert sm.same(lev[3, 1, 2, :2], [np.nanmin(x[3, 1, 2]), np.nanmax(x[3, 1, 2])])
    assert sm.same(lev[9, 0, 1, [0, 1, 6]], [np.inf, -np.inf, 0.0]) and sm.same(lev[5, 0, 0, [0, 1, 6]], [-np.inf, np.inf, np.inf])
    nan = np.isnan(lev[..., [2, 3, 4, 5]]).any(-1)
    only = np.zeros(h.shape[:3], bool); only[3, 1, 2] = only[9, 0, 1] = only[5, 0, 0] = True   # (inf - inf, too)
    assert np.array_equal(nan, only)
    el = sm.model(h, fx["spheremp"])
    assert np.array_equal(el[..., 7], want.sum(2)) and sm.same(el, sm.element_shares(lev))


def test_integral_of_one_and_the_mass(fx):
    sp = fx["spheremp"]
    one = np.ones((E, 1, 1, 4, 4))
    el = sm.model(one, sp)
    S, A = sm.exact_sums(one, sp)
    B = sm.bound(A, 1)
    st = dg.stats_from_partials(el)
    # the shares carry B; fsum adds them exactly and rounds once, the division rounds once: 2u of a value near 1
    tol = math.fsum(B[..., 3].ravel().tolist()) / (4 * math.pi) + 3 * sm.U
    exact = math.fsum(S[..., 3].ravel().tolist()) / (4 * math.pi)
    assert abs(st["integral"][0] - exact) <= tol and abs(exact - 1.0) <= GEOM_U and abs(st["integral"][0] - 1.0) <= tol + GEOM_U
    assert st["mean"][0] == 1.0 and st["area"][0] == st["integral"][0] and st["sum"][0] == 16 * E
    ps = fx["ps"]
    st = dg.stats_from_partials(sm.model(ps, sp))
    M = math.fsum((sp * ps[:, 0, 0]).ravel().tolist()) / (4 * math.pi)                 # the same rounded products, added exactly
    A = math.fsum(np.abs(sp * ps[:, 0, 0]).ravel().tolist())
    assert abs(st["integral"][0] - M) <= (4 * sm.U * A) / (4 * math.pi) + 3 * sm.U * M, (st["integral"][0], M)
    print("M = %r (shares) %r (fsum of the products)" % (float(st["integral"][0]), M))


def test_any_split_of_the_elements_gives_the_same_bits(fx):
    h, ht, w = _cases(fx)["v-grad*dp"]
    for per_level in (False, True):
        parts = sm.model(h, fx["spheremp"], ht, w, per_level=per_level)
        whole = dg.stats_from_partials(parts, ref=True)
        perm = np.random.default_rng(3).permutation(E)
        for cut in ([parts], [parts[:10], parts[10:]], [parts[perm[:5]], parts[perm[5:17]], parts[perm[17:]]]):
            got = dg.stats_from_partials(cut if len(cut) > 1 else cut[0], ref=True)
            assert got.keys() == whole.keys() and {"min", "max", "sum", "integral", "absmax", "nonfinite", "mean", "l1", "l2", "linf"} <= got.keys()
            for k in whole:
                assert sm.same(got[k].astype(np.float64), whole[k].astype(np.float64)) and got[k].shape == parts.shape[1:-1], k


def test_norms_against_the_reference_s_three_functions(fx):
    """l1_snorm, l2_snorm, linf_snorm transcribed (stats_model.snorms: global_integral's loop over i, j, the element sums added exactly),
    level by level.  Both routes add the same non-negative terms, each in its own order: the tree's 4 additions and n_ops roundings of a term
    here, 15 additions and the same n_ops there, so an integral differs by at most (4 + 15 + 2 n_ops + 2) u relatively (+ 2: one exact sum
    rounded and one division by 4 pi each), a quotient of two by the sum of both and one more rounding each; a root halves its argument's
    error and adds one rounding.  The maxima are exact and divided once: equal bits."""
    h, ht, _ = _cases(fx)["v-grad"]
    st = dg.stats_from_partials(sm.model(h, fx["spheremp"], ht, per_level=True), ref=True)
    u = sm.U
    rel = lambda n_ops: (4 + 15 + 2 * n_ops + 2) * u
    tol = dict(l1=rel(2) + rel(1) + 2 * u, l2=0.5 * (rel(4) + rel(2)) + 6 * u)
    worst = 0.0
    for f in range(h.shape[1]):
        for k in range(h.shape[2]):
            l1, l2, linf = sm.snorms(h[:, f, k], ht[:, f, k], fx["spheremp"])
            for key, want in (("l1", l1), ("l2", l2)):
                r = abs(st[key][f, k] - want) / want / tol[key]
                worst = max(worst, r)
                assert r <= 1.0, (key, f, k, st[key][f, k], want)
            assert st["linf"][f, k] == linf
    print("stats norms: worst difference / bound = %.3f" % worst)


def test_element_share_is_the_ascending_sum_of_the_level_shares(fx):
    h = fx["dp"]
    lev, el = sm.model(h, fx["spheremp"], per_level=True), sm.model(h, fx["spheremp"])
    S = lev[:, :, 0].copy()
    for k in range(1, lev.shape[2]):
        for j in range(16):
            S[..., j] = (np.minimum if j == 0 else np.maximum if j in (1, 6, 12, 13) else np.add)(S[..., j], lev[:, :, k, j])
    assert sm.same(S, el)


@pytest.mark.parametrize("power", [200, -200])
def test_scaling_by_a_power_of_two_is_exact(fx, power):
    h, ht, w = _cases(fx)["v-grad*dp"]
    c = 2.0 ** power
    for per_level in (False, True):
        a = sm.model(h, fx["spheremp"], ht, w, per_level=per_level)
        b = sm.model(c * h, fx["spheremp"], c * ht, w, per_level=per_level)
        for j in sm.SCALE_1:
            assert sm.same(b[..., j], c * a[..., j]), j
        for j in sm.SCALE_2:
            assert sm.same(b[..., j], (c * c) * a[..., j]), j
        assert sm.same(b[..., [7, 14, 15]], a[..., [7, 14, 15]])


def test_planted_errors_are_seen(fx):
    """A dropped point, the weight leaking into entry 2 and spheremp transposed leave the bound of the exact referee.  Levels added descending
    and m*(h*h) formed as (m*h)*h are other roundings of the same sums: they stay inside the bound and are seen in bits only -- which is
    what the GPU comparison looks at."""
    h, ht, w = _cases(fx)["v-grad*dp"]
    sp = fx["spheremp"]
    want = sm.model(h, sp, ht, w)
    S, A = sm.exact_sums(h, sp, ht, w)
    B = sm.bound(A, h.shape[2], weight=True)
    assert sm.worst_ratio(want, S, B) <= 1.0
    for plant, entry, at_bound in (("drop_point", 3, True), ("weight_in_sum", 2, True), ("transpose", 3, True), ("descending", 3, False),
                                   ("fused_square", 5, False)):
        got = sm.model(h, sp, ht, w, plant=plant)
        ndiff = int((sm.bits(got[..., entry]) != sm.bits(want[..., entry])).sum())
        r = sm.worst_ratio(got, S, B)
        print("stats planted %s: %d of %d shares differ in entry %d, error / bound = %.3g" % (plant, ndiff, want[..., entry].size, entry, r))
        assert ndiff >= 1, (plant, ndiff)                      # seen: a bit comparison fails
        assert (r > 1.0) == at_bound, (plant, r)
    # an unweighted entry 2 is untouched by the weight
    assert sm.same(want[..., 2], sm.model(h, sp)[..., 2])


def test_stats_from_partials_where_a_sum_overflows_or_holds_a_nan():
    parts = np.zeros((3, 1, 16)); parts[:, 0, 10] = 1.5e308; parts[:, 0, 11] = 1.0; parts[:, 0, 3] = [1.0, np.nan, 2.0]; parts[:, 0, 14] = 1.0
    st = dg.stats_from_partials(parts)
    assert np.isnan(st["integral"][0]) and st["area"][0] == 3.0 / (4 * math.pi)
    assert np.isinf(dg.stats_from_partials(parts, ref=True)["l2"][0])          # three finite shares whose sum is not: inf, no exception
    tot = dg.stats_from_partials([parts[:1], parts[1:]])
    assert np.isnan(tot["mean"][0])


# ---- prim_printstate's lines -----------------------------------------------------------------------------------------------------
def test_fortran_e_and_the_printstate_lines():
    e = dg.fortran_e
    assert e(1.0) == "  0.100000000000000E+01" and e(-1234.5678) == " -0.123456780000000E+04"
    assert e(0.0) == "  0.000000000000000E+00" and e(-0.0) == " -0.000000000000000E+00"
    assert e(1e100) == "  0.100000000000000+101" and e(-1e-101) == " -0.100000000000000-100" and e(1e-100) == "  0.100000000000000E-99"
    assert e(9.9999999999999995e-1) == "  0.100000000000000E+01"              # (the rounding carries into the exponent)
    assert e(0.1) == "  0.100000000000000E+00" and e(2.0 ** -1074) == "  0.494065645841247-323"
    assert e(123456789.123456789, 15, 7) == "  0.1234568E+09"
    assert e(float("nan")).strip() == "NaN" and e(float("-inf")).strip() == "-Infinity" and len(e(float("inf"))) == 23
    st = lambda lo, hi, s: dict(min=np.array([lo]), max=np.array([hi]), sum=np.array([s]))
    lines = dg.printstate_field_lines([("u", st(-1.5, 2.5, 1e100)), ("v", st(-0.0, 0.0, 0.0)), ("T", st(200.0, 300.0, 1.0e7)), ("ps", st(9.9e4, 1.01e5, 3.84e7)),
                                       ("dp3d", st(1.0, 2.0, 3.0))], mass=1.0e5, scale=0.5)
    assert lines == ["  u     =  -0.150000000000000E+01  0.250000000000000E+01  0.100000000000000+101",
                     "  v     =  -0.000000000000000E+00  0.000000000000000E+00  0.000000000000000E+00",
                     "  T     =   0.200000000000000E+03  0.300000000000000E+03  0.100000000000000E+08",
                     "      ps=   0.990000000000000E+05  0.101000000000000E+06  0.384000000000000E+08",
                     "  dp3d  =   0.100000000000000E+01  0.200000000000000E+01  0.300000000000000E+01",
                     "      M =   0.500000000000000E+05 kg/m^2  0.100000000000000E+06 mb     "]
