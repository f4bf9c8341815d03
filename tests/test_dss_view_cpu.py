"""tse_dss_view without a GPU: the two entries in the header, the symbol list, the product libraries and the Fortran seam;
tse_dss_view_plan (csrc/tse_views.cpp: path and footprint of every layout of tests/dss_view_model.py, the refusals that need no device);
and the model the GPU comparison rests on (dss_view_model.model = rspheremp * Oracle.dss(w)): held to step_ld's longdouble DSS within the
bound that file derives, shown to see four planted errors, and continuous across elements."""
import os
import re

import numpy as np
import pytest

import dss_view_model as dm
import pyoracle as po
import step_ld
from transport_se_amd import _lib
from transport_se_amd.hip_mod import TseError, dss_view_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tse_dss_view", "tse_dss_view_plan")
E = 24


def test_entries_are_declared_listed_and_exported_by_every_product_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "transport_se_hip.h")).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(0).split()) for m in re.finditer(r"\bint\s+(tse_[a-z0-9_]+)\s*\([^)]*\)\s*;", text)}
    assert decl["tse_dss_view"] == "int tse_dss_view(tse_ctx *ctx, int nf, int nk, int mode, const tse_view *field, void *stream);"
    assert decl["tse_dss_view_plan"] == ("int tse_dss_view_plan(int nelemd, int nf, int nk, const tse_view *field, int *path, long long *lo, "
                                         "long long *hi);")
    assert re.search(r"#define\s+TSE_DSS_AVERAGE\s+0\b", text) and re.search(r"#define\s+TSE_DSS_WEAK\s+1\b", text)
    for name in NAMES:
        assert name in _lib.SYMBOLS, name
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
        L = _lib.lib(nlev=nlev)
        assert not [n for n in NAMES if not hasattr(L, n)], nlev
    src = open(os.path.join(ROOT, "transport_se_amd", "fortran", "cuda_mod_hip.F90")).read().lower()
    assert re.search(r"subroutine\s+dss_view_hip\s*\(", src) and re.search(r"public\s*::[^\n]*\bdss_view_hip\b", src)
    assert re.search(r"dss_average\s*=\s*0\s*,\s*dss_weak\s*=\s*1", src) and "name='tse_dss_view'" in src


# ---- tse_dss_view_plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_plan_paths_and_footprints(nlev):
    seen = set()
    for nf in (1, 2, 5):
        for nk in (1, nlev, nlev + 1):
            for name in dm.LAYOUTS:
                s, _, size = dm.layout(name, E, nf, nk)
                got = dss_view_plan(E, nf, nk, s, nlev=nlev)
                assert got["path"] == dm.expected_path(name, nk, nlev), (name, nf, nk, got)
                assert (got["lo"], got["hi"]) == dm.footprint(name, E, nf, nk), (name, nf, nk, got)
                assert got["hi"] <= size
                seen.add(got["path"])
    assert seen == {0, 1, 2}
    # a negative level stride keeps whole lines (point-fastest) and moves the footprint below the pointer
    got = dss_view_plan(E, 2, nlev, [2 * nlev * 16, nlev * 16, -16, 4, 1], nlev=nlev)
    assert got == dict(path=0, lo=-(nlev - 1) * 16, hi=(E - 1) * 2 * nlev * 16 + nlev * 16 + 16), got
    # level-fastest rows of nlev + 1 interfaces: generic, as the header says
    S = nlev + 1
    assert dss_view_plan(E, 1, nlev + 1, [16 * S, 16 * S, 1, 4 * S, S], nlev=nlev)["path"] == 2
    assert dss_view_plan(E, 1, nlev, [16 * S, 16 * S, 1, 4 * S, S], nlev=nlev)["path"] == 1


def test_plan_refusals_and_unit_axes():
    nlev, nf = 72, 2
    dense = [nf * nlev * 16, nlev * 16, 16, 4, 1]
    with pytest.raises(TseError, match="nf = 0"):
        dss_view_plan(E, 0, nlev, dense)
    with pytest.raises(TseError, match="nk = 0"):
        dss_view_plan(E, nf, 0, dense)
    with pytest.raises(TseError, match="nk = %d" % (nlev + 2)):
        dss_view_plan(E, nf, nlev + 2, dense)
    assert dss_view_plan(E, nf, nlev + 1, [nf * (nlev + 1) * 16, (nlev + 1) * 16, 16, 4, 1])["path"] == 0
    for axis, word in enumerate(("element", "q", "level", "j", "i")):   # a zero stride on an extent above 1, the axis named
        z = list(dense); z[axis] = 0
        with pytest.raises(TseError, match="stride 0 on the %s axis" % word):
            dss_view_plan(E, nf, nlev, z)
    with pytest.raises(TseError, match="overlap itself.*q stride"):    # fields half a field apart
        dss_view_plan(E, nf, nlev, [nf * nlev * 16, nlev * 8, 16, 4, 1])
    with pytest.raises(TseError, match="overlap itself"):              # levels interleaved with the points of a row
        dss_view_plan(E, nf, nlev, [nf * nlev * 16, nlev * 16, 2, 4, 1])
    with pytest.raises(TseError, match="null view"):
        dss_view_plan(E, nf, nlev, None)
    # an axis of extent 1 may carry stride 0: a surface field [e][j][i], one layer field [e][k][j][i]
    assert dss_view_plan(E, 1, 1, [16, 0, 0, 4, 1]) == dict(path=0, lo=0, hi=E * 16)
    assert dss_view_plan(E, 1, nlev, [nlev * 16, 0, 16, 4, 1]) == dict(path=0, lo=0, hi=E * nlev * 16)
    assert dss_view_plan(E, 1, nlev, [nlev * 16, 0, 1, 4 * nlev, nlev])["path"] == 1
    L = _lib.lib()
    assert L.tse_dss_view(None, 1, 1, 0, None, None) != 0 and b"null context" in L.tse_last_error()   # (refused before any device call)


# ---- the model -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[2, 3])
def mesh(request):
    o = po.Oracle(request.param, 1)
    yield o
    o.close()


NF, NK = 2, 5


def test_model_within_the_longdouble_bound(mesh):
    """rspheremp * DSS(spheremp * f): products 1 + 1, a sum of at most four terms 3 -> m = 5 (step_ld: "extra variable m_x + 5"); weak: 4"""
    assert step_ld.has_extended_precision(), np.finfo(np.longdouble)
    o = mesh
    geo = step_ld.Geo(o)
    f = dm.field(o.nelem, NF, NK)
    for mode in dm.MODES:
        t = step_ld.exact(f)
        if mode == "average":
            t = step_ld.mul(geo.g(geo.spheremp, 5), t)
        t = step_ld.mul(geo.g(geo.rspheremp, 5), geo.dss.ld(t))
        assert t.m == (5 if mode == "average" else 4)
        worst, _ = step_ld.ratio(dm.model(o, f, mode), t)
        print("dss_view model ne%d %s: worst error / bound = %.3f" % (o.ne, mode, worst))
        assert worst <= 1.0, (mode, worst)


def _serial(o, f, mode, plant=None):
    """the model spelled out in numpy over step_ld.Dss' contribution lists, with one planted error:
    "corner" the corner contribution (the last of a four-copy node) dropped; "swap" the two edge contributions of a corner point added in
    the other order; "rspheremp" the final product omitted; "fused" spheremp * f carried unrounded into the first addition"""
    d = step_ld.Dss(o)
    sm, rs = np.asarray(o.spheremp)[:, None, None], np.asarray(o.rspheremp)[:, None, None]
    w = sm * f if mode == "average" else f.copy()
    g = d._gather(w)                                                  # [e][16][4][layers]
    cnt = d.count[:, :, None]
    corner = np.zeros((1, 16, 1), dtype=bool); corner[0, [0, 3, 12, 15]] = True
    order = [1, 2, 3]
    y = g[:, :, 0].copy()
    if plant == "fused" and mode == "average":
        a = np.broadcast_to(sm, f.shape).reshape(o.nelem, -1, 16).transpose(0, 2, 1)
        b = np.asarray(f).reshape(o.nelem, -1, 16).transpose(0, 2, 1)
        c = np.where(cnt > 1, g[:, :, 1], 0.0)
        # a * b exactly as hi + lo (Dekker), then one rounding of hi + c with lo folded in: the bits of fma(a, b, c) at all but rare ties
        split = 134217729.0
        ah = a * split; ah = ah - (ah - a); al = a - ah
        bh = b * split; bh = bh - (bh - b); bl = b - bh
        hi = a * b; lo = ((ah * bh - hi) + ah * bl + al * bh) + al * bl
        s = hi + c; bb = s - hi; err = (hi - (s - bb)) + (c - bb)
        y = np.where(cnt > 1, s + (err + lo), y)
        order = [2, 3]
    for c in order:
        use = cnt > c
        if plant == "corner" and c == 3:
            use = use & ~corner
        term = g[:, :, c]
        if plant == "swap" and c in (1, 2):
            term = np.where(corner & (cnt > 2), g[:, :, 3 - c], term)
        y = np.where(use, y + term, y)
    out = d._back(y, f.shape)
    return out if plant == "rspheremp" else rs * out


def test_planted_errors_change_bits(mesh):
    o = mesh
    f = dm.field(o.nelem, NF, NK, seed=1)
    for mode in dm.MODES:
        want = dm.model(o, f, mode)
        assert dm.same(_serial(o, f, mode), want), mode            # the harness itself: Oracle.dss bit for bit
        for plant in ("corner", "swap", "rspheremp", "fused"):
            if plant == "fused" and mode == "weak":
                continue                                            # (no product to fuse)
            got = _serial(o, f, mode, plant)
            ndiff = int((dm.bits(got) != dm.bits(want)).sum())
            print("dss_view planted %s ne%d %s: %d of %d values differ" % (plant, o.ne, mode, ndiff, want.size))
            assert ndiff >= 10, (plant, mode, ndiff)


def test_model_is_continuous_across_edges(mesh):
    """the node identity is read from the mesh's coordinates; a node of two copies adds the same two numbers on both sides (a + b = b + a,
    for spheremp in rspheremp too), so its copies hold equal bits whatever the field"""
    o = mesh
    ids = dm.node_ids(o)
    copies = np.bincount(ids.reshape(-1))
    assert set(copies.tolist()) <= {1, 2, 3, 4} and (copies == 3).sum() == 8          # the cube's corners are nodes of three elements
    assert ids.max() + 1 == 6 * o.ne * o.ne * 9 + 2                                     # unique GLL nodes of the np = 4 cubed sphere
    for f in (dm.own_values(o.nelem), dm.field(o.nelem, NF, NK, seed=2)):
        assert not dm.continuous(o, f, copies=(2,))[0]
        for mode in dm.MODES:
            ok, nbad, n = dm.continuous(o, dm.model(o, f, mode), copies=(2,))
            assert ok and n > 0, (mode, nbad, n)


def test_model_is_continuous(mesh):
    """After the model's DSS all copies of a shared node hold equal bits, at every node, two, three or four elements: every element is
    given its own value beforehand (dss_view_model.own_values: small integers, so no sum depends on the order in which an element adds
    its neighbours), the node identity comes from the mesh's coordinates.  The sums themselves are checked too: every copy holds the
    exact total of its node.  Then the whole model, rspheremp * DSS(spheremp * f) and rspheremp * DSS(f), with a mass matrix that is one
    per node (node_weights).  With the mesh's own rspheremp and with fields of full mantissa width the copies of a node of three or four
    elements differ in the last bits, as they do in the reference (dss_view_model says why); those are held to the longdouble bound
    above and, across edges, to equal bits."""
    o = mesh
    f = dm.own_values(o.nelem)
    assert not dm.continuous(o, f)[0]                                                   # every element its own value beforehand
    d = o.dss(f.reshape(o.nelem, -1, 4, 4).copy()).reshape(f.shape)
    ok, nbad, n = dm.continuous(o, d)
    assert ok and n > 0, (nbad, n)
    want = dm.node_sums(o, f)
    assert dm.same(d, want) and want.max() < 2.0 ** 24
    w = dm.node_weights(o)
    for mode in dm.MODES:
        y = dm.model(o, f, mode, weights=w)
        ok, nbad, n = dm.continuous(o, y)
        assert ok, (mode, nbad, n)
        assert dm.same(y, w[1][:, None, None] * want), mode
