"""tse_vlaplace_view without a GPU: the entries in the header, the symbol list, the product libraries and the Fortran seam;
tse_vlaplace_view_plan (paths and footprints of every layout of tests/dss_view_model.py for `in` and for `out`, the in-place and the
disjoint form, every refusal that needs no device); cube_mesh.metinv; and the model the GPU bound rests on (vlaplace_model): the fp64
restatement of the reference lies under its bound against the longdouble chain, planted errors do not, and the operator has the
eigenvalues of the sphere's vector Laplacian."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import dss_view_model as dm
import elem_ops_ld as ld
import pyoracle as po
import vlaplace_model as vm
from transport_se_amd import _lib
from transport_se_amd import cube_mesh as cm
from transport_se_amd.hip_mod import TseError, vlaplace_view_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tse_vector_setup", "tse_vlaplace_view", "tse_vlaplace_view_plan")
E = 24
BASE = 1 << 20   # a made-up address: the plan never touches memory


def test_entries_are_declared_listed_and_exported_by_every_product_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()) for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    assert decl["tse_vector_setup"] == ("int tse_vector_setup(tse_ctx *ctx, const double *D, size_t D_stride, const double *metinv, size_t metinv_stride, "
                                        "const double *mp, size_t mp_stride);")
    assert decl["tse_vlaplace_view"] == ("int tse_vlaplace_view(tse_ctx *ctx, int nk, int order, double nu_ratio, const tse_view *in, const tse_view *out, "
                                         "void *stream);")
    assert decl["tse_vlaplace_view_plan"] == ("int tse_vlaplace_view_plan(int nelemd, int nk, const tse_view *in, const tse_view *out, int path[2], "
                                              "long long lo[2], long long hi[2]);")
    assert re.search(r"#define\s+TSE_VLAPLACE\s+1\b", text) and re.search(r"#define\s+TSE_VBIHARMONIC\s+2\b", text)
    for name in NAMES:
        assert name in _lib.SYMBOLS, name
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
        L = _lib.lib(nlev=nlev)
        assert not [n for n in NAMES if not hasattr(L, n)], nlev
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    for sub in ("vector_setup_hip", "vlaplace_view_hip"):
        assert re.search(r"subroutine\s+%s\s*\(" % sub, src) and re.search(r"public\s*::[^\n]*\b%s\b" % sub, src), sub
    assert "name='tse_vlaplace_view'" in src and "name='tse_vector_setup'" in src


def test_timer_group_names_do_not_match_each_other():
    """tse_kernel_time matches a name against every group it is a prefix of"""
    others = ("lap", "fieldlap", "fielddss")
    assert not any("fieldvlap".startswith(g) or g.startswith("fieldvlap") for g in others)


# ---- tse_vlaplace_view_plan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_plan_paths_and_footprints_of_in_and_out(nlev):
    seen = set()
    for nk in (1, 2, nlev, nlev + 1):
        lay = {name: dm.layout(name, E, 2, nk) for name in dm.LAYOUTS}
        for i, name in enumerate(dm.LAYOUTS):
            other = dm.LAYOUTS[(i + 3) % len(dm.LAYOUTS)]
            # in place (strides alone), then `out` another layout in an allocation of its own right behind in's
            got = vlaplace_view_plan(E, nk, lay[name][0], nlev=nlev)
            assert got[0] == got[1] and got[0]["path"] == dm.expected_path(name, nk, nlev), (name, nk, got)
            assert (got[0]["lo"], got[0]["hi"]) == dm.footprint(name, E, 2, nk), (name, nk, got)
            got = vlaplace_view_plan(E, nk, (lay[name][0], BASE), (lay[other][0], BASE + 8 * lay[name][2]), nlev=nlev)
            for g, nm in zip(got, (name, other)):
                assert g["path"] == dm.expected_path(nm, nk, nlev), (name, other, nk, got)
                assert (g["lo"], g["hi"]) == dm.footprint(nm, E, 2, nk) and g["hi"] <= lay[nm][2], (name, other, nk, got)
            seen.add((got[0]["path"], got[1]["path"]))
    assert {a for a, _ in seen} == {b for _, b in seen} == {0, 1, 2} and any(a != b for a, b in seen)
    # E3SM's state%v(np,np,2,nlev,tl): component stride 16, level stride 32 -- point-fastest
    got = vlaplace_view_plan(E, nlev, [32 * nlev * 3, 16, 32, 4, 1], nlev=nlev)
    assert got[0]["path"] == 0 and (got[0]["lo"], got[0]["hi"]) == (0, (E - 1) * 96 * nlev + 32 * nlev)


def test_plan_in_place_disjoint_and_refusals():
    nlev, nf = 72, 2
    plane = nlev * 16
    dense = [nf * plane, plane, 16, 4, 1]
    size = E * nf * plane                                               # doubles of the dense field
    lev = [nf * 16 * nlev, 16 * nlev, 1, 4 * nlev, nlev]
    # identical views: in place
    assert vlaplace_view_plan(E, nlev, (dense, BASE), (dense, BASE)) == [dict(path=0, lo=0, hi=size)] * 2
    # disjoint: touching footprints on either side, other strides
    for off in (size, -size):
        assert [g["path"] for g in vlaplace_view_plan(E, nlev, (dense, BASE), (lev, BASE + 8 * off))] == [0, 1]
    # out overlapping in without being it: a shifted pointer (by one double, by all but one), other strides inside one footprint
    for off in (1, -1, size - 1, -(size - 1), 16):
        with pytest.raises(TseError, match="tse_vlaplace_view: out .* overlaps in"):
            vlaplace_view_plan(E, nlev, (dense, BASE), (dense, BASE + 8 * off))
    with pytest.raises(TseError, match="overlaps in"):
        vlaplace_view_plan(E, nlev, (dense, BASE), (lev, BASE))
    with pytest.raises(TseError, match="overlaps in"):                  # the same addresses, the components' order reversed
        vlaplace_view_plan(E, nlev, (dense, BASE), ([nf * plane, -plane, 16, 4, 1], BASE + 8 * plane))
    # the refusals of either view, the view named
    for which in ("in", "out"):
        def plan(n_k, bad):
            a, b = ((bad, BASE), (dense, BASE + 8 * size)) if which == "in" else ((dense, BASE), (bad, BASE + 8 * size))
            return vlaplace_view_plan(E, n_k, a, b)
        for axis, word in enumerate(("element", "q", "level", "j", "i")):   # a zero stride on an extent above 1, the axis named
            z = list(dense); z[axis] = 0
            with pytest.raises(TseError, match=r"tse_vlaplace_view.*stride 0 on the %s axis.*\(%s\)" % (word, which)):
                plan(nlev, z)
        with pytest.raises(TseError, match=r"overlap itself.*q stride.*\(%s\)" % which):     # the components half a field apart
            plan(nlev, [nf * plane, plane // 2, 16, 4, 1])
        with pytest.raises(TseError, match=r"overlap itself.*\(%s\)" % which):               # levels interleaved with the points of a row
            plan(nlev, [nf * plane, plane, 2, 4, 1])
    with pytest.raises(TseError, match="tse_vlaplace_view: nk = 0"):
        vlaplace_view_plan(E, 0, dense)
    with pytest.raises(TseError, match="tse_vlaplace_view: nk = %d" % (nlev + 2)):
        vlaplace_view_plan(E, nlev + 2, dense)
    with pytest.raises(TseError, match="null view"):
        vlaplace_view_plan(E, nlev, None)
    L = _lib.lib()
    v = _lib.View(BASE, (C.c_longlong * 5)(*dense))
    assert L.tse_vlaplace_view_plan(E, nlev, C.byref(v), None, None, None, None) != 0 and b"null view" in L.tse_last_error()
    # the level axis of extent 1 may carry stride 0: a wind on one surface [e][c][j][i]; interfaces
    assert vlaplace_view_plan(E, 1, [32, 16, 0, 4, 1]) == [dict(path=0, lo=0, hi=E * 32)] * 2
    assert vlaplace_view_plan(E, nlev + 1, [2 * (nlev + 1) * 16, (nlev + 1) * 16, 16, 4, 1])[0]["path"] == 0
    # refused before any device call
    assert L.tse_vlaplace_view(None, 1, 2, 1.0, None, None, None) != 0 and b"null context" in L.tse_last_error()
    assert L.tse_vector_setup(None, None, 0, None, 0, None, 0) != 0 and b"null context" in L.tse_last_error()


# ---- cube_mesh.metinv ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [2, 3, 8])
def test_metinv_is_dinv_dinv_transposed_and_symmetric(ne):
    """metinv = Dinv Dinv^T to 8 ulps of the point's largest entry; metinv(1,2) and metinv(2,1) are the same bits"""
    g = cm.geometry(ne)
    mi = cm.metinv(g["D"])
    assert mi.shape == g["D"].shape
    assert dm.same(mi[..., 0, 1], mi[..., 1, 0])
    Di = g["Dinv"]                                   # [...][b][a]
    A = lambda a, b: Di[..., b, a]
    want = np.empty(mi.shape)
    for a in range(2):
        for b in range(2):
            want[..., b, a] = A(a, 0) * A(b, 0) + A(a, 1) * A(b, 1)
    big = np.abs(want).max(axis=(-1, -2), keepdims=True)
    assert (np.abs(mi - want) <= 8 * np.spacing(big)).all(), float((np.abs(mi - want) / np.spacing(big)).max())
    assert (mi[..., 0, 0] > 0).all() and (mi[..., 1, 1] > 0).all()


# ---- the model -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh(ne):
    o = po.Oracle(ne, 1)
    return o, vm.host_fields(o)


NK = 3


def _fields(o):
    return (("random", vm.random_field(o.nelem, NK)), ("smooth", vm.smooth_field(o, NK)))


def test_the_oracle_mesh_is_cube_mesh():
    """the D and mp the model takes from the oracle are cube_mesh.geometry's, the host side of every GPU test"""
    o, (D, mi, mp) = _mesh(2)
    g = cm.geometry(2)
    assert dm.same(D, g["D"]) and dm.same(mp, g["mp"]) and dm.same(np.array(o.Dinv), g["Dinv"])


@pytest.mark.parametrize("ne", [2, 3])
def test_reference_fp64_within_the_longdouble_bound(ne):
    """bound(28, A) for order 1, bound(60, A) for order 2.  Measured here (worst error / bound over ne2, ne3, the two fields and nu_ratio
    1.0, 2.5): order 1 0.067, order 2 0.010."""
    assert ld.has_extended_precision(), np.finfo(np.longdouble)
    o, (D, mi, mp) = _mesh(ne)
    for nu in (1.0, 2.5):
        for order in vm.ORDERS:
            for name, f in _fields(o):
                ref, A = vm.longdouble(o, D, mi, mp, f, order, nu)
                assert (A >= np.abs(ref)).all()
                got = vm.reference_chain_fp64(o, D, mi, mp, f, order, nu)
                if order == 1:
                    assert dm.same(got[:, :, 1], vm.reference_fp64(o, D, mi, mp, f[:, :, 1], nu))
                worst = float(vm.ratio(got, ref, A, order).max())
                print("vlaplace model ne%d order %d nu_ratio %.1f %s: worst error / bound = %.3f" % (o.ne, order, nu, name, worst))
                assert worst < 1.0, (order, nu, name, worst)


@pytest.mark.parametrize("ne", [2, 3])
def test_planted_errors_exceed_the_bound(ne):
    """each planted error (nu_ratio 2.5, so that a misplaced ratio shows) is beyond the bound in every element it touches"""
    o, (D, mi, mp) = _mesh(ne)
    nu = 2.5
    for name, f in _fields(o):
        for order in vm.ORDERS:
            ref, A = vm.longdouble(o, D, mi, mp, f, order, nu)
            for plant in vm.PLANTS1 + (vm.PLANTS2 if order == 2 else ()):
                got = vm.longdouble(o, D, mi, mp, f, order, nu, plant)[0].astype(np.float64)
                per_elem = vm.ratio(got, ref, A, order).reshape(o.nelem, -1).max(axis=1)
                touched = [vm.bm.dropped_copy(o)[0]] if plant == "dropped" else list(range(o.nelem))
                print("vlaplace planted %s ne%d order %d %s: least error / bound over the touched elements = %.3g" % (plant, o.ne, order, name, per_elem[touched].min()))
                assert (per_elem[touched] > 1.0).all(), (plant, order, name, per_elem[touched].min())


MEASURED_NE8 = {"l1 rigid rotation": 0.0602, "l2 rotational": 0.0599, "l2 divergent": 0.0599, "l3 rotational": 0.131}


def test_eigenvalues_of_the_vector_laplacian():
    """rspheremp * DSS(vlaplace(v)) / rrearth^2 against -(l(l+1) - 2) v, the largest error relative to max|v|.  Measured with this model:
         field               ne4     ne8     factor
         l1 rigid rotation   0.2353  0.0602  3.9
         l2 rotational       0.3538  0.0599  5.9
         l2 divergent        0.3538  0.0599  5.9     (nu_ratio 2.5, against -(6 * 2.5 - 2): 0.2435, 0.0593)
         l3 rotational       0.3933  0.1313  3.0
    (the largest errors sit at element corners: cubics, pointwise second order).  Asserted: at most twice the ne8 figure, at least a
    factor 2 from ne4 to ne8.  The planted errors of the operator leave errors of 0.5 and more at ne8 on the fields they touch."""
    err = {}
    for ne in (4, 8):
        o, (D, mi, mp) = _mesh(ne)
        for name, (v, lam, divergent) in vm.harmonic_fields(o).items():
            scale = np.abs(v).max()
            err[(ne, name)] = float(np.abs(vm.strong_laplacian(o, D, mi, mp, v) - lam * v).max() / scale)
            print("vlaplace eigenvalue ne%d %-18s %.4f" % (ne, name, err[(ne, name)]))
            if divergent:
                r = 2.5
                e = float(np.abs(vm.strong_laplacian(o, D, mi, mp, v, r) - (-(6.0 * r - 2.0)) * v).max() / scale)
                print("vlaplace eigenvalue ne%d %-18s %.4f (nu_ratio %.1f)" % (ne, name, e, r))
                err[(ne, name + " nu")] = e
            if ne == 8:
                for plant in vm.PLANTS1[:3]:
                    if plant == "curl_added" and divergent:
                        continue                     # (no vorticity: the curl term is zero)
                    e = float(np.abs(vm.strong_laplacian(o, D, mi, mp, v, 1.0, plant) - lam * v).max() / scale)
                    print("vlaplace eigenvalue ne8 %-18s planted %s: %.3f" % (name, plant, e))
                    assert e > 4 * MEASURED_NE8[name] and e > 0.5, (name, plant, e)
    for name, m in MEASURED_NE8.items():
        assert err[(8, name)] <= 2 * m, (name, err[(8, name)])
        assert err[(4, name)] >= 2 * err[(8, name)], (name, err[(4, name)], err[(8, name)])
    assert err[(8, "l2 divergent nu")] <= 2 * MEASURED_NE8["l2 divergent"] and err[(4, "l2 divergent nu")] >= 2 * err[(8, "l2 divergent nu")]
