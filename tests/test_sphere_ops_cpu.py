"""tse_sphere_op_view without a GPU: the entries in the header, the symbol list, the product libraries and the Fortran seam;
tse_sphere_op_view_plan (paths and footprints of the nine path pairs, every refusal that needs no device); and the model the GPU bound
rests on (sphere_ops_model): its fp64 restatements of gradient_sphere and divergence_sphere have the oracle's bits, every restatement
lies under its bound against the longdouble chain, planted errors do not, and the C0 fields converge to the analytic ones."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import dss_view_model as dm
import elem_ops_ld as ld
import pyoracle as po
import sphere_ops_model as sm
from transport_se_amd import _lib
from transport_se_amd.hip_mod import SPHERE_OPS, TseError, sphere_op_view_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tse_sphere_op_view", "tse_sphere_op_view_plan")
E = 24
BASE = 1 << 20   # a made-up address: the plan never touches memory


def test_entries_are_declared_listed_and_exported_by_every_product_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()) for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    assert decl["tse_sphere_op_view"] == "int tse_sphere_op_view(tse_ctx *ctx, int nk, int op, int c0, const tse_view *in, const tse_view *out, void *stream);"
    assert decl["tse_sphere_op_view_plan"] == ("int tse_sphere_op_view_plan(int nelemd, int nk, int op, const tse_view *in, const tse_view *out, int path[2], "
                                               "long long lo[2], long long hi[2]);")
    for name, val in (("TSE_OP_GRADIENT", 0), ("TSE_OP_DIVERGENCE", 1), ("TSE_OP_VORTICITY", 2), ("TSE_OP_LOCAL", 0), ("TSE_OP_C0", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), text), name
    assert SPHERE_OPS == dict(gradient=0, divergence=1, vorticity=2)
    for name in NAMES:
        assert name in _lib.SYMBOLS, name
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
        L = _lib.lib(nlev=nlev)
        assert not [n for n in NAMES if not hasattr(L, n)], nlev
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    assert re.search(r"subroutine\s+sphere_op_view_hip\s*\(", src) and re.search(r"public\s*::[^\n]*\bsphere_op_view_hip\b", src)
    assert "name='tse_sphere_op_view'" in src
    for const, val in (("op_gradient", 0), ("op_divergence", 1), ("op_vorticity", 2), ("op_local", 0), ("op_c0", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (const, val), src), const


def test_timer_group_names_do_not_match_each_other():
    """tse_kernel_time matches a name against every group it is a prefix of: no group named in the header is a prefix of "fieldop", and
    "fieldop" is a prefix of none"""
    text = open(os.path.join(ROOT, "include", "transport_se_hip.h")).read()
    doc = text[text.index("accumulated HIP-event time"):text.index("int tse_kernel_time")]
    groups = set(re.findall(r'"([a-z_0-9]+)"', doc)) - {"fieldop"}
    assert {"lap", "dss", "fieldlap", "fielddss", "fieldvlap", "fieldremap", "forcing", "view"} <= groups
    assert not [g for g in groups if "fieldop".startswith(g) or g.startswith("fieldop")]


# ---- tse_sphere_op_view_plan -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [72, 64, 80])
@pytest.mark.parametrize("op", sm.OPS)
def test_plan_paths_and_footprints_of_the_nine_pairs(op, nlev):
    nfi, nfo = sm.NF[op]
    seen = set()
    for nk in (1, 3, nlev, nlev + 1):
        for name in dm.LAYOUTS:
            for other in dm.LAYOUTS:
                li, lo = dm.layout(name, E, nfi, nk), dm.layout(other, E, nfo, nk)
                got = sphere_op_view_plan(E, nk, op, (li[0], BASE), (lo[0], BASE + 8 * li[2]), nlev=nlev)   # out right behind in's allocation
                for g, nm, nf, lay in zip(got, (name, other), (nfi, nfo), (li, lo)):
                    assert g["path"] == dm.expected_path(nm, nk, nlev), (op, name, other, nk, got)
                    assert (g["lo"], g["hi"]) == dm.footprint(nm, E, nf, nk) and g["hi"] <= lay[2], (op, name, other, nk, got)
                if nk == nlev:
                    seen.add((got[0]["path"], got[1]["path"]))
                else:                     # a level-fastest view of another depth is not given path 1: it takes the generic path
                    assert 1 not in (got[0]["path"], got[1]["path"]), (op, name, other, nk, got)
    assert seen == {(a, b) for a in range(3) for b in range(3)}, seen
    # E3SM's state%v(np,np,2,nlev,tl) on the two-field side, a dense scalar with q stride 0 on the other: both point-fastest
    wind, scal = [32 * nlev * 3, 16, 32, 4, 1], [16 * nlev, 0, 16, 4, 1]
    a, b = (scal, wind) if op == "gradient" else (wind, scal)
    got = sphere_op_view_plan(E, nlev, op, a, b, nlev=nlev)                   # strides alone: the overlap rule is not asked
    assert [g["path"] for g in got] == [0, 0]
    fp = {id(wind): (0, (E - 1) * 96 * nlev + 32 * nlev), id(scal): (0, E * 16 * nlev)}
    assert [(g["lo"], g["hi"]) for g in got] == [fp[id(a)], fp[id(b)]]


@pytest.mark.parametrize("op", sm.OPS)
def test_plan_refusals_and_touching_footprints(op):
    nlev = 72
    nfi, nfo = sm.NF[op]
    plane = nlev * 16
    dense = lambda nf: [nf * plane, plane, 16, 4, 1]
    lev = lambda nf: [nf * 16 * nlev, 16 * nlev, 1, 4 * nlev, nlev]
    si, so = E * nfi * plane, E * nfo * plane                              # doubles of the dense fields
    # touching footprints on either side are disjoint
    assert [g["path"] for g in sphere_op_view_plan(E, nlev, op, (dense(nfi), BASE), (lev(nfo), BASE + 8 * si))] == [0, 1]
    assert [g["path"] for g in sphere_op_view_plan(E, nlev, op, (dense(nfi), BASE), (dense(nfo), BASE - 8 * so))] == [0, 0]
    # overlap: there is no in-place form, not even for the same pointer
    for off in (0, 1, si - 1, -(so - 1), 16):
        with pytest.raises(TseError, match="tse_sphere_op_view: out .* overlaps in"):
            sphere_op_view_plan(E, nlev, op, (dense(nfi), BASE), (dense(nfo), BASE + 8 * off))
    with pytest.raises(TseError, match="overlaps in"):
        sphere_op_view_plan(E, nlev, op, (dense(nfi), BASE), (lev(nfo), BASE + 8 * 5))
    # the two-field side needs a q stride; the one-field side may carry 0 there
    two = "in" if nfi == 2 else "out"
    z = list(dense(2)); z[1] = 0
    a, b = ((z, BASE), (dense(1), BASE + 8 * si)) if two == "in" else ((dense(1), BASE), (z, BASE + 8 * si))
    with pytest.raises(TseError, match=r"tse_sphere_op_view.*stride 0 on the q axis.*\(%s\)" % two):
        sphere_op_view_plan(E, nlev, op, a, b)
    with pytest.raises(TseError, match=r"overlap itself.*\(%s\)" % two):    # the components half a field apart
        h = [2 * plane, plane // 2, 16, 4, 1]
        a, b = ((h, BASE), (dense(1), BASE + 8 * si)) if two == "in" else ((dense(1), BASE), (h, BASE + 8 * si))
        sphere_op_view_plan(E, nlev, op, a, b)
    for which, nf in (("in", nfi), ("out", nfo)):
        for axis, word in ((0, "element"), (2, "level"), (3, "j"), (4, "i")):
            z = list(dense(nf)); z[axis] = 0
            a, b = ((z, BASE), (dense(nfo), BASE + 8 * si)) if which == "in" else ((dense(nfi), BASE), (z, BASE + 8 * si))
            with pytest.raises(TseError, match=r"tse_sphere_op_view.*stride 0 on the %s axis.*\(%s\)" % (word, which)):
                sphere_op_view_plan(E, nlev, op, a, b)
    for nk in (0, nlev + 2, -1):
        with pytest.raises(TseError, match="tse_sphere_op_view: nk = %d" % nk):
            sphere_op_view_plan(E, nk, op, dense(nfi), dense(nfo))
    with pytest.raises(TseError, match="null view"):
        sphere_op_view_plan(E, nlev, op, None, dense(nfo))
    with pytest.raises(TseError, match="null view"):
        sphere_op_view_plan(E, nlev, op, dense(nfi), None)
    # a level-fastest view whose depth is not nlev: path 1 is not for it
    got = sphere_op_view_plan(E, 3, op, [nfi * 48, 48, 1, 12, 3], [nfo * 48, 48, 1, 12, 3])
    assert [g["path"] for g in got] == [2, 2]


def test_plan_refuses_an_unknown_operator_and_the_entry_a_null_context():
    dense = [72 * 16, 0, 16, 4, 1]
    for op in (-1, 3, 7):
        with pytest.raises(TseError, match="tse_sphere_op_view: op=%d" % op):
            sphere_op_view_plan(E, 72, op, dense, dense)
    with pytest.raises(TseError, match="unknown op 'curl'"):
        sphere_op_view_plan(E, 72, "curl", dense, dense)
    L = _lib.lib()
    assert L.tse_sphere_op_view(None, 1, 2, 0, None, None, None) != 0 and b"null context" in L.tse_last_error()


# ---- the model -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh(ne):
    o = po.Oracle(ne, 1)
    return o, np.array(o.D)


NK = 3


def _fields(o, nf):
    return (("random", sm.random_field(o.nelem, nf, NK)), ("smooth", sm.smooth_field(o, nf, NK)))


@pytest.mark.parametrize("ne", [2, 3])
def test_gradient_and_divergence_restatements_have_the_oracles_bits(ne, gold):
    """the oracle is bit-exact against the reference (test_oracle_golden.py); ref_ops.npz holds reference output of both"""
    o, D = _mesh(ne)
    for name, s in _fields(o, 1):
        got = sm.reference_fp64(o, D, "gradient", s)
        for ie in range(o.nelem):
            for k in range(NK):
                assert dm.same(got[ie, :, k], o.gradient_sphere(ie, s[ie, 0, k])), (name, ie, k)
    for name, v in _fields(o, 2):
        got = sm.reference_fp64(o, D, "divergence", v)
        for ie in range(o.nelem):
            for k in range(NK):
                assert dm.same(got[ie, 0, k], o.divergence_sphere(ie, v[ie, :, k])), (name, ie, k)
    if ne == 2:
        g = gold("ref_ops.npz")
        o5 = po.Oracle(2, 5, nu_q=1e19)     # the mesh the golden file was made on
        try:
            D5 = np.array(o5.D)
            for n, ie in enumerate(g["ie"]):
                s = np.zeros((o5.nelem, 1, 1, 4, 4)); s[ie, 0, 0] = g["s"][n]
                v = np.zeros((o5.nelem, 2, 1, 4, 4)); v[ie, :, 0] = g["v"][n]
                assert dm.same(sm.reference_fp64(o5, D5, "gradient", s)[ie, :, 0], g["grad"][n])
                assert dm.same(sm.reference_fp64(o5, D5, "divergence", v)[ie, 0, 0], g["div"][n])
        finally:
            o5.close()


@pytest.mark.parametrize("ne", [2, 3])
def test_restatements_within_the_longdouble_bound(ne):
    """bound(N, A), N = 7 / 13 / 12 (+ 5 for C0), for the source-order and the device-order restatement of every operator.  Measured here,
    worst error / bound over ne2, ne3 and the two fields (source order, device order): gradient 0.454, 0.396; divergence 0.222, 0.168;
    vorticity 0.220, 0.166; C0: gradient 0.292, 0.271; divergence 0.114, 0.108; vorticity 0.153, 0.121."""
    assert ld.has_extended_precision(), np.finfo(np.longdouble)
    o, D = _mesh(ne)
    for op in sm.OPS:
        for name, f in _fields(o, sm.NF[op][0]):
            for c0 in (False, True):
                ref, A = sm.longdouble(o, D, op, f, c0)
                assert ref.shape == (o.nelem, sm.NF[op][1], NK, 4, 4) and (A >= np.abs(ref)).all()
                for kind, fn in (("source", sm.reference_fp64), ("device", sm.device_order)):
                    got = fn(o, D, op, f)
                    if c0:
                        got = sm.make_c0(o, got)
                    worst = float(sm.ratio(got, ref, A, op, c0).max())
                    print("sphere_ops model ne%d %s c0=%d %s %s order: worst error / bound = %.3f" % (o.ne, op, c0, name, kind, worst))
                    assert worst < 1.0, (op, c0, name, kind, worst)


@pytest.mark.parametrize("ne", [2, 3])
def test_planted_errors_exceed_the_bound(ne):
    """D(1,2) and D(2,1) swapped in the covariant map, a dropped rmetdet, a wrong sign on dudy: each beyond the bound in every element"""
    o, D = _mesh(ne)
    assert len(sm.PLANTS) >= 3
    for name, f in _fields(o, 2):
        for c0 in (False, True):
            ref, A = sm.longdouble(o, D, "vorticity", f, c0)
            for plant in sm.PLANTS:
                got = sm.longdouble(o, D, "vorticity", f, c0, plant)[0].astype(np.float64)
                per_elem = sm.ratio(got, ref, A, "vorticity", c0).reshape(o.nelem, -1).max(axis=1)
                print("sphere_ops planted %s ne%d c0=%d %s: least error / bound over the elements = %.3g" % (plant, o.ne, c0, name, per_elem.min()))
                assert (per_elem > 1.0).all(), (plant, c0, name, per_elem.min())


def test_an_error_a_field_maximum_norm_would_pass():
    """a wrong sign on dudy on the last level alone, where the wind is 2^-40 of the other levels' (a tail of the level loop gone wrong
    under a quantity that is small aloft): the error is 1e-12 of the field's maximum, and far beyond the pointwise bound"""
    o, D = _mesh(2)
    f = sm.random_field(o.nelem, 2, NK, seed=4)
    f[:, :, NK - 1] = np.ldexp(f[:, :, NK - 1], -40)
    ref, A = sm.longdouble(o, D, "vorticity", f)
    got = sm.reference_fp64(o, D, "vorticity", f)
    assert float(sm.ratio(got, ref, A, "vorticity").max()) < 1.0
    bad = sm.longdouble(o, D, "vorticity", f, plant="dudy_sign")[0].astype(np.float64)
    got[:, :, NK - 1] = bad[:, :, NK - 1]
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    rel = float(err.max() / np.abs(ref).max().astype(np.float64))
    worst = float(sm.ratio(got, ref, A, "vorticity").max())
    print("sphere_ops last-level plant: error / field maximum = %.3g, error / bound = %.3g" % (rel, worst))
    assert rel < 1e-10 and worst > 1e3


def test_c0_fields_converge_to_the_analytic_ones():
    """solid-body rotation u = U cos(lat): zeta = 2 U sin(lat) * rrearth, div = 0;  s = sin(lat): grad = (0, cos(lat) * rrearth).  The
    largest error of the C0 model, relative to the largest analytic value (for div: to that of zeta), falls by more than 4 from ne4 to
    ne8.  Measured with this model:
         field        ne4        ne8        factor
         C0 zeta      3.45e-03   5.30e-04   6.50
         C0 div       2.07e-03   3.57e-04   5.80
         C0 grad      8.51e-04   1.49e-04   5.70
    (about 8 would be third order; the largest errors sit at element corners)"""
    err = {}
    for ne in (4, 8):
        o, D = _mesh(ne)
        v, zeta, div = sm.solid_body(o)
        s, grad = sm.sine_of_latitude(o)
        c0 = lambda op, x: sm.make_c0(o, sm.reference_fp64(o, D, op, x))
        zs, gs = np.abs(zeta).max(), np.abs(grad).max()
        err[(ne, "zeta")] = float(np.abs(c0("vorticity", v) - zeta).max() / zs)
        err[(ne, "div")] = float(np.abs(c0("divergence", v) - div).max() / zs)
        err[(ne, "grad")] = float(np.abs(c0("gradient", s) - grad).max() / gs)
    for name in ("zeta", "div", "grad"):
        factor = err[(4, name)] / err[(8, name)]
        print("sphere_ops analytic C0 %-5s ne4 %.3g ne8 %.3g factor %.2f" % (name, err[(4, name)], err[(8, name)], factor))
        assert factor > 4.0 and err[(8, name)] < 1e-3, (name, err)
