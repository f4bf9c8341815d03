"""-m gpu: tse_stats_view -- the element shares of min, max, sums, integrals and norms of a host's own device arrays through strided views.

The reference of every bit comparison is stats_model.model (tests/test_stats_view_cpu.py holds it to an exact referee within a derived
bound and shows that it sees five planted errors), computed once per (mesh, nf, nk, ref, weight, per_level).
 1 bits          ne2: every layout x nk in {1, 3, nlev, nlev + 1} x nf in {1, 2, 5} x with / without ref and weight, each on a different
                 path (or width) from the field x per_level 0 / 1, on the 72-, the 64- and the 80-level library.  The sums of a slab without a NaN are compared in bits, so is everything else.
 2 independence  permuted elements permute the shares; three emulated ranks give the one-context shares and the same digits;
                 NaN, +inf, -inf and -0.0 planted in known slabs
 3 the library   views inside the library's own "ps_v", "dp3d" and "omega_p" after three DCMIP 1-1 steps; nothing of the context's
                 visible state changes, nor the host's array, padding included; a null and a non-null stream; the refusals, each naming
                 its view (a stream of another device: only where two GPUs are visible)"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import dss_view_model as dm
import stats_model as sm
import view_common as vc
from view_common import FakeArray as _Fake, raw_field as _raw

pytestmark = pytest.mark.gpu
QSIZE = 2


@functools.lru_cache(maxsize=None)
def _oracle(ne):
    return vc.oracle(ne, QSIZE)


def _make(ne, nlev=72, weights=None):
    """weights: (spheremp, rspheremp) in place of the mesh's own"""
    return vc.make_hip(_oracle(ne), QSIZE, nlev, weights=weights)


@functools.lru_cache(maxsize=None)
def _hip(ne, nlev=72):
    """a context of qsize 2 on the oracle's mesh (kept for the session: contexts are small)"""
    return _make(ne, nlev)



# the layouts of dss_view_model -- point-fastest wide (dense) and narrow by its base (dense_odd8: 8 but not 16 bytes aligned), level-fastest
# unpadded (lev0), padded to an even pitch (lev_even) and to an odd one (lev_odd: narrow rows), a generic view (ij) -- and two point-fastest
# layouts that are narrow by ONE ODD STRIDE (stats_layouts: dense_odd_e the element stride, dense_odd_k the level stride)
from stats_layouts import Strided, expected_path, layout   # noqa: E402

LAYOUTS = ("dense", "dense_odd8", "dense_odd_e", "dense_odd_k", "lev0", "lev_even", "lev_odd", "ij")
OTHER = {"dense": "lev_even", "dense_odd8": "ij", "dense_odd_e": "lev0", "dense_odd_k": "lev_odd", "lev0": "dense_odd_k", "lev_even": "ij",
         "lev_odd": "dense_odd_e", "ij": "lev0"}   # another path, or the other width of the same one


@functools.lru_cache(maxsize=None)
def _fields(n, nf, nk):
    """(h, ht, w): a field, a 'true solution' close to it, a positive weight; read-only"""
    h = dm.field(n, nf, nk)
    ht = h + 1e-3 * dm.field(n, nf, nk, seed=1)
    w = 1.0 + np.abs(dm.field(n, 1, nk, seed=2))[:, 0]
    for x in (h, ht, w):
        x.setflags(write=False)
    return h, ht, w


@functools.lru_cache(maxsize=None)
def _want(ne, nf, nk, ref, weight, per_level):
    h, ht, w = _fields(_oracle(ne).nelem, nf, nk)
    out = sm.model(h, _oracle(ne).spheremp, ht if ref else None, w if weight else None, per_level=per_level)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _laid(n, nf, nk, role, name):
    """(Strided, its device copy) of one of _fields in a layout; the device copy is never written"""
    import torch
    x = _fields(n, nf, nk)[role]
    S = Strided(x if role < 2 else x[:, None], name)
    return S, torch.from_numpy(S.host.copy()).cuda()


def _view(S, buf):
    return _Fake(S.shape, S.s, buf.data_ptr() + 8 * S.base)


def _call(h, n, nf, nk, name, ref, weight, per_level, stream=None):
    S, buf = _laid(n, nf, nk, 0, name)
    kw = {}
    if ref:
        R, rbuf = _laid(n, nf, nk, 1, OTHER[name])
        kw.update(ref=_view(R, rbuf))
    if weight:
        W, wbuf = _laid(n, nf, nk, 2, OTHER[OTHER[name]])
        kw.update(weight=_view(W, wbuf), weight_axes="eqkji")
    return h.stats_view(_view(S, buf), "eqkji", per_level=per_level, stream=stream, **kw)


# ---- 1 ----
def _matrix(nlev, nk):
    """every layout x nf x ref x weight x per_level at nk levels on the nlev-level library; the device copies keep their bits"""
    from transport_se_amd.hip_mod import stats_view_plan
    from transport_se_amd import _lib
    ne = 2
    h = _hip(ne, nlev)
    paths, forms = set(), set()
    for nf in (1, 2, 5):
        for name in LAYOUTS:
            names = (name, OTHER[name], OTHER[OTHER[name]])
            lay = [layout(x, h.nelemd, 1 if i == 2 else nf, nk) for i, x in enumerate(names)]
            plans = stats_view_plan(h.nelemd, nf, nk, lay[0][0], lay[1][0], lay[2][0], nlev=nlev)
            assert [p["path"] for p in plans] == [expected_path(x, nk, nlev) for x in names], (name, nf, nk, plans)
            paths.update(p["path"] for p in plans)
            for ref in (False, True):
                for weight in (False, True):
                    for per_level in (False, True):
                        got = _call(h, h.nelemd, nf, nk, name, ref, weight, per_level)
                        want = _want(ne, nf, nk, ref, weight, per_level)
                        assert sm.same(got, want), (nlev, nk, nf, name, ref, weight, per_level, int((sm.bits(got) != sm.bits(want)).sum()))
    assert paths == ({0, 1, 2} if nk == nlev else {0, 2})
    for nf in (1, 2, 5):
        for role in (0, 1, 2):
            for name in LAYOUTS:
                S, buf = _laid(h.nelemd, nf, nk, role, name)
                assert sm.same(buf.cpu().numpy(), S.host), (nf, role, name)


@pytest.mark.parametrize("nk", [1, 3, 72, 73])
def test_bits_of_the_model(nk):
    _matrix(72, nk)


@pytest.mark.parametrize("nlev,nk", [(n, k) for n in (64, 80) for k in (1, 3, n, n + 1)])
def test_bits_of_the_model_at_other_level_counts(nlev, nk):
    _matrix(nlev, nk)


def test_the_odd_strides_are_point_fastest_and_narrow():
    """what the two layouts are there for: path 0, and view_wide says no because of one odd stride alone (the base is 16-byte aligned)"""
    from transport_se_amd.hip_mod import stats_view_plan
    for name, axis in (("dense_odd_e", 0), ("dense_odd_k", 2)):
        for nf, nk in ((2, 72), (5, 73), (1, 3)):
            s_, base, _ = layout(name, 24, nf, nk)
            assert base == 0 and stats_view_plan(24, nf, nk, s_)[0]["path"] == 0
            assert [i for i, x in enumerate(s_) if x % 2 and (24, nf, nk, 4, 4)[i] > 1 and i < 3] == [axis], (name, s_)
            S, buf = _laid(24, nf, nk, 0, name)
            assert buf.data_ptr() % 16 == 0


def test_arrays_without_their_unit_axes_and_the_numbers():
    """a surface field [e][j][i] and a layer field [e][j][i][k] as torch arrays; diagnostics.stats_from_partials on the shares"""
    import torch
    from transport_se_amd import diagnostics as dg
    ne, nlev = 2, 72
    h, o = _hip(ne), _oracle(ne)
    hh, ht, w = _fields(h.nelemd, 1, 1)
    ps = torch.from_numpy(np.array(hh[:, 0, 0])).cuda()
    got = h.stats_view(ps, "eji")
    assert got.shape == (h.nelemd, 1, 16) and sm.same(got, _want(ne, 1, 1, False, False, False))
    hh, ht, w = _fields(h.nelemd, 1, nlev)
    lf = lambda x: torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 1, -1))).cuda()        # [e][k][j][i] -> [e][j][i][k]
    T, Tt, dp = lf(hh[:, 0]), lf(ht[:, 0]), torch.from_numpy(np.array(w)).cuda()
    got = h.stats_view(T, "ejik", ref=Tt, weight=dp, weight_axes="ekji", per_level=True)
    assert got.shape == (h.nelemd, 1, nlev, 16) and sm.same(got, _want(ne, 1, nlev, True, True, True))
    st = dg.stats_from_partials(got, ref=True)
    x = hh[:, 0]
    assert np.array_equal(st["min"][0], x.min((0, 2, 3))) and np.array_equal(st["max"][0], x.max((0, 2, 3))) and not st["nonfinite"].any()
    m = o.spheremp[:, None] * w
    assert np.allclose(st["mean"][0], (m * x).sum((0, 2, 3)) / m.sum((0, 2, 3)), rtol=1e-13, atol=0)
    assert np.allclose(st["l2"][0], np.sqrt((m * (x - ht[:, 0]) ** 2).sum((0, 2, 3)) / (m * ht[:, 0] ** 2).sum((0, 2, 3))), rtol=1e-13, atol=0)


# ---- 2 ----
def test_permuted_elements_permute_the_shares():
    ne, nf, nk = 2, 2, 72
    o = _oracle(ne)
    n = o.nelem
    perm = np.random.default_rng(11).permutation(n)
    assert not np.array_equal(perm, np.arange(n))
    h = _hip(ne)
    hp = _make(ne, weights=(o.spheremp[perm], o.rspheremp[perm]))
    try:
        hh, ht, w = _fields(n, nf, nk)
        import torch
        for per_level in (False, True):
            a = _call(h, n, nf, nk, "lev0", True, True, per_level)
            dev = [torch.from_numpy(np.ascontiguousarray(x[perm])).cuda() for x in (hh, ht, w)]
            b = hp.stats_view(dev[0], "eqkji", ref=dev[1], weight=dev[2], weight_axes="ekji", per_level=per_level)
            assert sm.same(b, a[perm]) and not sm.same(b, a)
    finally:
        hp.close()


def test_three_ranks_give_the_shares_of_one_context():
    from test_gpu_multirank_emulated import _run_ne
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd import diagnostics as dg
    ne, nf, nk = 2, 2, 72
    nelem = 6 * ne * ne
    hh, ht, w = _fields(nelem, nf, nk)
    geo = cm.geometry(ne, cm.topology(ne))

    def body(rank, h, mine, geo_, hv):
        import torch
        dev = [torch.from_numpy(np.ascontiguousarray(x[mine])).cuda() for x in (hh, ht, w)]
        return [h.stats_view(dev[0], "eqkji", ref=dev[1], weight=dev[2], weight_axes="ekji", per_level=pl) for pl in (False, True)]
    (mine1, one), = _run_ne(1, ne=ne, qsize=QSIZE, body=body)
    res = _run_ne(3, ne=ne, qsize=QSIZE, body=body)
    assert all(r is not None for r in res) and sorted(np.concatenate([m for m, _ in res]).tolist()) == list(range(nelem))
    for i, per_level in enumerate((False, True)):
        want = sm.model(hh, geo["spheremp"], ht, w, per_level=per_level)
        full1 = np.empty_like(want); full1[mine1] = one[i]
        full3 = np.empty_like(want)
        for mine, r in res:
            full3[mine] = r[i]
        assert sm.same(full1, want) and sm.same(full3, want)
        a, b = dg.stats_from_partials(one[i], ref=True), dg.stats_from_partials([r[i] for _, r in res], ref=True)
        assert all(sm.same(a[k].astype(np.float64), b[k].astype(np.float64)) for k in a)


def test_special_values():
    import torch
    ne, nf, nk = 2, 2, 3
    h, o = _hip(ne), _oracle(ne)
    hh, ht, w = (np.array(x) for x in _fields(h.nelemd, nf, nk))
    hh[3, 1, 2, 1, 1] = np.nan; hh[5, 0, 0, 0, 0] = np.inf; hh[5, 0, 0, 3, 3] = -np.inf; hh[7, 1, 1, 2, 0] = -0.0; hh[9, 0, 1] = np.nan
    hh[11, 0, 2, 0, 1] = np.inf
    ht[13, 1, 0, 2, 2] = np.nan
    count = np.zeros(hh.shape[:3]); count[3, 1, 2] = 1; count[5, 0, 0] = 2; count[9, 0, 1] = 16; count[11, 0, 2] = 1
    dev = [torch.from_numpy(x).cuda() for x in (hh, ht, w)]
    for layout_axes, moved in (("eqkji", lambda t: t), ("eqjik", lambda t: t.permute(0, 1, 3, 4, 2).contiguous())):
        for ref in (False, True):
            lev = h.stats_view(moved(dev[0]), layout_axes, ref=moved(dev[1]) if ref else None, per_level=True)
            el = h.stats_view(moved(dev[0]), layout_axes, ref=moved(dev[1]) if ref else None)
            want = sm.model(hh, o.spheremp, ht if ref else None, per_level=True)
            assert sm.same_or_both_nan(lev, want) and sm.same_or_both_nan(el, sm.element_shares(want))
            assert np.array_equal(lev[..., 7], count) and np.array_equal(el[..., 7], count.sum(2))
            x = hh.reshape(hh.shape[:3] + (16,))
            assert sm.same(lev[3, 1, 2, :2], [np.nanmin(x[3, 1, 2]), np.nanmax(x[3, 1, 2])])                 # the NaN is skipped
            assert sm.same(lev[9, 0, 1, [0, 1, 6]], [np.inf, -np.inf, 0.0])                                    # a slab of NaNs
            assert sm.same(lev[5, 0, 0, [0, 1, 6]], [-np.inf, np.inf, np.inf]) and sm.same(lev[11, 0, 2, [1, 2, 3]], [np.inf] * 3)
            nan = np.isnan(lev[..., [2, 3, 4, 5]]).any(-1)
            only = np.zeros(hh.shape[:3], bool); only[3, 1, 2] = only[9, 0, 1] = only[5, 0, 0] = True        # (inf - inf, too)
            assert np.array_equal(nan, only)
            assert sm.same(lev[7, 1, 1, 2], want[7, 1, 1, 2]) and lev[7, 1, 1, 7] == 0                          # -0.0 is a finite value
            if ref:
                nanr = np.isnan(lev[..., 8:12]).any(-1)                                                         # h or ht NaN; |inf - ht| stays inf
                onlyr = np.zeros(hh.shape[:3], bool); onlyr[3, 1, 2] = onlyr[9, 0, 1] = onlyr[13, 1, 0] = True
                assert np.array_equal(nanr, onlyr), np.argwhere(nanr != onlyr)
                assert lev[13, 1, 0, 13] == np.nanmax(np.abs(ht[13, 1, 0])) and lev[13, 1, 0, 7] == 0


# ---- 3 ----
LIB_FIELDS = ("qdp1", "qdp2", "dp", "divdp", "divdp_proj", "dp3d", "ps_v", "omega_p", "eta_dot_dpdn", "qmin", "qmax")
GROUPS = ("dss", "view", "level", "fieldremap", "fielddss", "fieldlap", "fieldvlap", "fieldop", "remap", "advance", "minmax", "norms", "stateq")


def test_the_library_s_own_fields_and_untouched_state():
    from gpu_common import elem_from_oracle
    from transport_se_amd import diagnostics as dg
    ne, nlev, dt = 2, 72, 1800.0
    o = _oracle(ne)
    h = _make(ne)
    try:
        h.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm)
        h.dcmip_set_initial()
        assert h.prim_run_subcycle(dt, 1, 0) == 3
        elem = elem_from_oracle(o)
        h.get_derived(elem)
        before = {k: _raw(h, k) for k in LIB_FIELDS}
        mm = h.get_qminmax()
        h.timing(True)
        E, plane = h.nelemd, nlev * 16
        ps_p, n = h.device_ptr("ps_v"); assert n == E * 16 * 8
        dp_p, n = h.device_ptr("dp3d"); assert n == E * plane * 8
        om_p, _ = h.device_ptr("omega_p")
        ps = _Fake((E, 4, 4), [16, 4, 1], ps_p)
        dp = _Fake((E, nlev, 4, 4), [plane, 16, 4, 1], dp_p)
        om = _Fake((E, nlev, 4, 4), [plane, 16, 4, 1], om_p)
        got = h.stats_view(ps, "eji")
        assert sm.same(got, sm.model(elem["ps_v"][:, None, None], o.spheremp)) and float(got[..., 0].min()) > 9.0e4
        M = dg.stats_from_partials(got)["integral"][0]
        Mh = math.fsum((o.spheremp * elem["ps_v"]).ravel().tolist()) / (4 * math.pi)               # the same products, added exactly
        assert abs(M - Mh) <= 8 * sm.U * Mh, (M, Mh)                                                # (4 additions of the tree, fsum, the division)
        print("\n".join(dg.printstate_field_lines([("ps", dg.stats_from_partials(got))], mass=M)))
        for per_level in (False, True):
            got = h.stats_view(dp, "ekji", per_level=per_level)
            assert sm.same(got, sm.model(elem["dp3d"][:, None], o.spheremp, per_level=per_level))
            got = h.stats_view(om, "ekji", ref=dp, weight=dp, per_level=per_level)                    # the views may overlap each other
            assert sm.same(got, sm.model(elem["omega_p"][:, None], o.spheremp, elem["dp3d"][:, None], elem["dp3d"], per_level=per_level))
        assert h.kernel_time("fieldstats")[1] == 5 and h.kernel_time("fieldstats")[0] > 0.0
        for g in GROUPS:
            assert h.kernel_time(g)[1] == 0, g
        h.timing(False)
        for k in LIB_FIELDS:
            assert dm.same(_raw(h, k), before[k]), k
        assert all(dm.same(a, b) for a, b in zip(h.get_qminmax(), mm))
        part, nbytes = h.device_ptr("stats_partials")
        assert part and nbytes == E * nlev * 16 * 8
        from transport_se_amd.hip_mod import TseError
        with pytest.raises(TseError, match=r"\(field\).*partials buffer"):
            h.stats_view(_Fake((E, nlev, 4, 4), [plane, 16, 4, 1], part), "ekji")
    finally:
        h.close()


def test_streams_and_refusals():
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    ne, nlev, nf = 2, 72, 2
    h = _hip(ne)
    hh, ht, w = _fields(h.nelemd, nf, nlev)
    E, plane = h.nelemd, nlev * 16
    dense = [nf * plane, plane, 16, 4, 1]
    wdense = [plane, 0, 16, 4, 1]
    buf, wbuf = torch.from_numpy(np.array(hh)).cuda(), torch.from_numpy(np.array(w)).cuda()
    keep = buf.clone()
    host = np.array(hh)
    want = _want(ne, nf, nlev, False, False, False)
    # a null and a non-null stream
    s = torch.cuda.Stream()
    made = torch.zeros_like(buf)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        made.copy_(buf, non_blocking=True)
        got = h.stats_view(made, "eqkji", stream=s)                       # waits for the stream; complete on return
        made.zero_()
    assert sm.same(got, want) and sm.same(h.stats_view(buf, "eqkji"), want)
    torch.cuda.synchronize()
    h.timing(True)

    def view(strides, ptr):
        return _lib.View(ptr, (C.c_longlong * 5)(*strides))
    raw = vc.RawAllocation(hh.size * 8, fill=host)
    beyond = raw.beyond
    fv = view(dense, buf.data_ptr())
    out = np.zeros((E, nf, 16))
    cases = [
        ("device", lambda: h.stats_view(_Fake(hh.shape, dense, host.ctypes.data), "eqkji")),
        (r"\(ref\).*device", lambda: h.stats_view(buf, "eqkji", ref=_Fake(hh.shape, dense, host.ctypes.data))),
        (r"\(field\).*outside its allocation", lambda: h.stats_view(_Fake(hh.shape, dense, beyond), "eqkji")),
        (r"\(weight\).*outside its allocation", lambda: h.stats_view(buf, "eqkji", weight=_Fake(w.shape, [plane, 16, 4, 1], raw.end - w.nbytes + 8),
                                                        weight_axes="ekji")),
        ("per_level=2", lambda: h._chk(h.L.tse_stats_view(h.h, nf, nlev, 2, C.byref(fv), None, None, None, out.ctypes.data))),
        ("null out", lambda: h._chk(h.L.tse_stats_view(h.h, nf, nlev, 0, C.byref(fv), None, None, None, None))),
        ("null view", lambda: h._chk(h.L.tse_stats_view(h.h, nf, nlev, 0, None, None, None, None, out.ctypes.data))),
        ("nf = 0", lambda: h.stats_view(fv, None, nf=0, nk=nlev)),
        ("nk = %d" % (nlev + 2), lambda: h.stats_view(fv, None, nf=1, nk=nlev + 2)),
        ("stride 0 on the j axis", lambda: h.stats_view(view([nf * plane, plane, 16, 0, 1], buf.data_ptr()), None, nf=nf, nk=nlev)),
        (r"overlap itself.*\(ref\)", lambda: h.stats_view(fv, None, ref=view([nf * plane, plane // 2, 16, 4, 1], buf.data_ptr()), nf=nf, nk=nlev)),
        ("null view pointer", lambda: h.stats_view(view(dense, None), None, nf=nf, nk=nlev)),
        (r"\(weight\).*not 8-byte aligned", lambda: h.stats_view(fv, None, weight=view(wdense, wbuf.data_ptr() + 4), nf=nf, nk=nlev)),
        ("ref has 1 fields", lambda: h.stats_view(buf, "eqkji", ref=wbuf, ref_axes="ekji")),
        ("one field of 72 is needed", lambda: h.stats_view(buf, "eqkji", weight=buf, weight_axes="eqkji")),
    ]
    for text, call in cases:
        with pytest.raises(TseError, match=text):
            call()
        assert h.kernel_time("fieldstats")[1] == 0, text
    # a stream that is being captured
    torch.cuda.synchronize()
    with vc.capturing(s):
        with pytest.raises(TseError, match="captured"):
            h.stats_view(buf, "eqkji", stream=s)
    assert h.kernel_time("fieldstats")[1] == 0
    assert torch.equal(buf.view(torch.int64), keep.view(torch.int64))
    # the view that fits its allocation exactly is served
    assert sm.same(h.stats_view(_Fake(hh.shape, dense, raw.ptr), "eqkji"), want) and h.kernel_time("fieldstats")[1] == 1
    h.timing(False)
    raw.free()


def test_a_stream_of_another_device_is_refused():
    """the one refusal that needs a second GPU"""
    import torch
    from transport_se_amd.hip_mod import TseError
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs (%d visible)" % torch.cuda.device_count())
    ne = 2
    h = _hip(ne)
    hh, _, _ = _fields(h.nelemd, 2, 3)
    buf = torch.from_numpy(np.array(hh)).cuda()
    other = torch.cuda.Stream(device=1)
    h.timing(True)
    with pytest.raises(TseError, match="belongs to device 1"):
        h.stats_view(buf, "eqkji", stream=other)
    assert h.kernel_time("fieldstats")[1] == 0
    h.timing(False)
