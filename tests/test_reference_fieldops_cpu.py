"""The view models against the reference's own Fortran (no GPU): tests/golden/ref_ne2_fieldops.npz, made by oracle/ref/ref_harness.F90's
dump_fieldops from derivative_mod.F90 and viscosity_mod.F90 on all 24 elements of ne2 and three levels.

The models (sphere_ops_model, biharmonic_model, vlaplace_model, dss_view_model) restate those routines in numpy with index conventions of
their own; the kernels are held to the models.  Here the models are held to the reference: geometry from ref_ne2_static.npz and the
fixture (never from cube_mesh), node identity from the static file's lat/lon.
 1 geometry      cube_mesh.metinv against elem%metinv
 2 under bound   the reference's fp64 output lies under every model's own bound against the model's longdouble chain
 3 restatements  the models' fp64 restatements against the reference's output: the bound asserted, the bits that differ recorded
 4 plants        every planted error of the models, and the two transpositions (D(a,b), (i,j)), are seen by the reference's output
"""
import functools

import numpy as np
import pytest

import dss_view_model as dm
import elem_ops_ld as ld
import fieldops_ref as fr
from conftest import record_margin
from transport_se_amd import cube_mesh as cm

pytestmark = pytest.mark.skipif(not ld.has_extended_precision(), reason="needs an 80-bit longdouble")


@pytest.fixture(scope="module")
def ctx(gold):
    st, fx = gold("ref_ne2_static.npz"), gold("ref_ne2_fieldops.npz")
    st = {k: st[k] for k in st.files}
    fx = {k: fx[k] for k in fx.files}
    o = fr.mesh(st)
    geo = (st["D"], fx["metinv"], st["mp"])
    yield o, geo, fx, fr.cases(fx)
    o.close()


@functools.lru_cache(maxsize=None)
def _chain(key):
    """(value, A) of a case's longdouble chain, computed once (set by the ctx of the module)"""
    o, geo, fx, cases = _chain.ctx
    c = cases[key]
    return c.ld(o, geo, fx[c.src], None)


@pytest.fixture(scope="module")
def chain(ctx):
    _chain.ctx = ctx
    _chain.cache_clear()
    return _chain


KEYS = tuple(fr.cases(dict(nu_ratio=(1.0, 2.5))))


def test_fixture_is_what_the_issue_of_its_making_says(ctx, gold):
    o, geo, fx, cases = ctx
    assert bool(fx["bfb_1v2"]), "the reference's two-rank run did not give the one-rank bits"
    assert fx["s"].shape == (24, 1, 3, 4, 4) and fx["v"].shape == (24, 2, 3, 4, 4) and tuple(fx["nu_ratio"]) == (1.0, 2.5)
    assert np.array_equal(fx["gid"], gold("ref_ne2_static.npz")["gid"])
    assert np.abs(fx["v"].mean()) < 1.0 and fx["s"].min() > 0           # the wind centred on 0
    ok, nbad, n = dm.continuous(o, fx["dss_average"])                   # the second scalar is continuous: in every bit at a node of two
    ok2, _, n2 = dm.continuous(o, fx["dss_average"], copies=(2,))
    assert ok2 and n2 > 0
    # compute_zeta_C0 / compute_div_C0 are vorticity_sphere / divergence_sphere of state%v behind make_C0
    assert dm.same(fx["zeta_c0"], fx["vor_c0"]) and dm.same(fx["divergence_c0"], fx["div_c0"])


# ---- 1 ----
def test_metinv_matches_the_reference(ctx):
    """cube_mesh.metinv(D) against elem%metinv by the rule test_geometry_matches_reference_ne2 applies to every other key: 1e-15 of the
    field's maximum.  (The reference forms metinv from the D of before the area correction and divides by alpha; cube_mesh.metinv has
    only the corrected D.  The 2x2 determinant does not cancel on this mesh -- (|D11 D22| + |D12 D21|) / |det D| is printed -- so the
    rule holds as it stands.)"""
    o, geo, fx, _ = ctx
    Dr, ref = geo[0], fx["metinv"]
    D11, D21, D12, D22 = Dr[..., 0, 0], Dr[..., 0, 1], Dr[..., 1, 0], Dr[..., 1, 1]
    kappa = float(((np.abs(D11 * D22) + np.abs(D12 * D21)) / np.abs(D11 * D22 - D12 * D21)).max())
    assert np.array_equal(ref[..., 0, 1], ref[..., 1, 0])      # symmetric in every bit
    for name, D in (("the reference's D", Dr), ("cube_mesh.geometry(2)", cm.geometry(2)["D"])):
        err = float(np.abs(cm.metinv(D) - ref).max() / np.abs(ref).max())
        print("metinv from %s: error / field maximum = %.3g (condition of the determinant %.3f)" % (name, err, kappa))
        record_margin("cube_mesh.metinv vs reference elem%%metinv (%s)" % name, err, 1e-15)
        assert err < 1e-15, (name, err)


# ---- 2 ----
@pytest.mark.parametrize("key", KEYS)
def test_reference_output_lies_under_the_models_bound(ctx, chain, key):
    """ratio <= 1 at every point: the models' rounding counts claim to cover the reference's association"""
    o, geo, fx, cases = ctx
    c = cases[key]
    ref, A = chain(key)
    r = fr.ratio(fx[c.out], ref, A, c.N)
    worst = float(r.max())
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    print("reference %s under bound(%d, A): worst ratio %.3f at (element, field, level, j, i) = %s" % (key, c.N, worst, at))
    record_margin("reference %s vs the model's longdouble chain / bound(%d, A)" % (key, c.N), worst, 1.0)
    assert np.isfinite(np.asarray(ref, dtype=np.float64)).all() and float(np.abs(fx[c.out]).max()) > 0
    assert worst <= 1.0, (key, worst, at)


# ---- 3 ----
@pytest.mark.parametrize("key", KEYS)
def test_fp64_restatements_against_the_reference(ctx, chain, key):
    """the models' fp64 restatements and the reference's output both lie under the bound, so they differ by at most twice the bound (the
    triangle inequality); how many values differ in a bit is recorded, not asserted -- the Fortran compiler may contract"""
    o, geo, fx, cases = ctx
    c = cases[key]
    got = c.fp64(o, geo, fx[c.src])
    ref, A = chain(key)
    own = float(fr.ratio(got, ref, A, c.N).max())
    b = 2.0 * ld.bound(c.N, A)
    d = np.abs(got - fx[c.out])
    worst = float(np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d > 0, np.inf, 0.0)).max())
    ndiff = int((dm.bits(got) != dm.bits(fx[c.out])).sum())
    print("fp64 restatement of %s: %d of %d values differ from the reference in a bit; |diff| / (2 bound) = %.3g; own ratio %.3f" % (key, ndiff, got.size, worst, own))
    record_margin("fp64 restatement of %s vs reference / 2 bound(%d, A)" % (key, c.N), worst, 1.0)
    record_margin("fp64 restatement of %s vs reference: share of values that differ in a bit" % key, ndiff / got.size, 1.0)
    assert own <= 1.0 and worst <= 1.0, (key, own, worst)


# ---- 4 ----
@pytest.mark.parametrize("key", [k for k in KEYS if not k.startswith("dss")])
def test_the_reference_sees_every_plant(ctx, key):
    """the reference's output against a model with one planted error exceeds the bound somewhere: a transposed D(a,b), a transposed
    (i,j), a wrong sign on the curl or a misplaced nu_ratio in model and kernel alike would not pass part 2"""
    o, geo, fx, cases = ctx
    c = cases[key]
    assert set(("D_transposed", "ij_transposed")) <= set(c.plants)
    for plant in c.plants:
        bad, A = c.ld(o, geo, fx[c.src], plant)
        r = fr.ratio(fx[c.out], bad, A, c.N)
        print("reference %s against the model planted %s: worst ratio %.3g, share of points beyond the bound %.3f" % (key, plant, r.max(), (r > 1).mean()))
        assert r.max() > 1.0, (key, plant, float(r.max()))
