"""-m gpu: tse_column_view -- interface and mid-point pressure, hydrostatic geopotential and omega / p of a host's own device arrays
through strided views, on the ne2 mesh (24 elements).

The reference of every bit comparison is column_model.model (tests/test_column_cpu.py holds it to a longdouble referee within derived
bounds, ties it to the physics by four identities and shows that it sees six planted errors), computed once per (nlev, op, p given).
 1 bits          every op x every layout of stats_layouts as out x the inputs each in another layout (point-fastest wide and narrow,
                 level-fastest unpadded, padded even and odd, generic) x p given / formed, on the 72-, 64- and 80-level library; the
                 padding of out keeps its payload; PHI and OMEGA without p are PMID followed by the op with that p; phis with level
                 stride 0, as the slice of a larger array and as one level of a point-fastest one
 2 the bound     the device under column_model.bound against the referee on the CPU test's input family
 3 independence  permuted elements permute the result; one changed column changes that column alone
 4 the library   dp = "dp3d", b = "ps_v" / "divdp" inside the library; out inside the library refused; nothing visible changes
 5 streams and refusals, and the sequence column_view("pmid") -> sphere_op_view("gradient") on one stream"""
import ctypes as C
import functools

import numpy as np
import pytest

import column_model as cm
import dss_view_model as dm
import view_common as vc
from stats_layouts import Strided, layout
from view_common import FakeArray as _Fake, raw_field as _raw

pytestmark = pytest.mark.gpu
QSIZE = 2
NE = 2
LAYOUTS = ("dense", "dense_odd8", "dense_odd_e", "dense_odd_k", "lev0", "lev_even", "lev_odd", "ij")
INPUTS = ("dense", "lev0", "lev_even", "ij", "lev_odd", "dense_odd_k")     # role r of out layout i takes INPUTS[(i + r) % 6]: mixed pairs
ROLES = ("dp", "p", "tv", "phis", "vgrad_p", "divdp")
SENTINEL = -7.25e33


@functools.lru_cache(maxsize=None)
def _oracle(ne):
    return vc.oracle(ne, QSIZE)


def _make(ne, nlev=72):
    return vc.make_hip(_oracle(ne), QSIZE, nlev)


@functools.lru_cache(maxsize=None)
def _hip(ne, nlev=72):
    """a context of qsize 2 on the oracle's mesh (kept for the session: contexts are small)"""
    return _make(ne, nlev)


@functools.lru_cache(maxsize=None)
def _fields(nlev, seed=0):
    """the CPU test's family on the mesh's columns, as [E][1][nk][4][4] arrays (phis [E][1][1][4][4]); p: a pressure that is no prefix
    sum.  Read-only."""
    E = _oracle(NE).nelem
    f = cm.family(nlev, E * 16, seed=seed)
    out = dict(ptop=f["ptop"], rgas=f["rgas"])
    for k in ("dp", "tv", "vgrad_p", "divdp"):
        out[k] = cm.from_cols(f[k].reshape(nlev, E, 4, 4))
    out["phis"] = np.ascontiguousarray(f["phis"].reshape(E, 1, 1, 4, 4))
    out["p"] = cm.from_cols(cm.pmid(f["dp"], f["ptop"]).reshape(nlev, E, 4, 4) * (1.0 + 1e-3 * np.sin(np.arange(nlev))[:, None, None, None]))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _model_views(op, f, pgiven):
    c = {k: cm.to_cols(v) for k, v in f.items() if isinstance(v, np.ndarray)}
    return cm.views_of(op, c, p=c["p"] if pgiven else None)


@functools.lru_cache(maxsize=None)
def _want(nlev, op, pgiven, seed=0):
    f = _fields(nlev, seed)
    out = cm.from_cols(cm.model(op, f["ptop"], f["rgas"], **_model_views(op, f, pgiven)))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _laid(nlev, role, name, seed=0):
    """(Strided, its device copy) of one input in a layout; the device copy is never written"""
    import torch
    S = Strided(_fields(nlev, seed)[role], name)
    return S, torch.from_numpy(S.host.copy()).cuda()


def _view(S, buf):
    from transport_se_amd import _lib
    return _lib.View(buf.data_ptr() + 8 * S.base, (C.c_longlong * 5)(*S.s))


def _inputs(nlev, op, pgiven, i, seed=0):
    """the keyword views of HipMod.column_view for one op, input role r in the layout INPUTS[(i + r) % 6]"""
    pick = lambda r: _view(*_laid(nlev, ROLES[r], INPUTS[(i + r) % len(INPUTS)], seed))
    if op in ("pint", "pmid"):
        return dict(dp=pick(0))
    if op == "phi":
        S, buf = _laid(nlev, "phis", ("dense", "ij", "dense_odd8")[i % 3], seed)
        return dict(dp=pick(0), p=pick(1) if pgiven else None, a=pick(2), b=_view(S, buf))
    return dict(dp=None if pgiven else pick(0), p=pick(1) if pgiven else None, a=pick(4), b=pick(5))


def _run(h, op, pgiven, name, i, seed=0, stream=None, **over):
    """one call into a fresh out array in the layout `name` -> the result; every gap of out keeps its bits"""
    import torch
    nlev = h.nlev
    f = _fields(nlev, seed)
    nko = nlev + 1 if op == "pint" else nlev
    T = Strided(np.full((h.nelemd, 1, nko, 4, 4), SENTINEL), name)
    res = torch.from_numpy(T.host.copy()).cuda()
    kw = _inputs(nlev, op, pgiven, i, seed)
    kw.update(over)
    h.column_view(op, out=_view(T, res), ptop=f["ptop"], rgas=f["rgas"], stream=stream, **kw)
    if stream is not None:
        torch.cuda.synchronize()
    got, gaps = T.read(res.cpu().numpy())
    assert gaps, "bytes outside the out view changed (%s, %s)" % (op, name)
    return got


CASES = (("pint", False), ("pmid", False), ("phi", False), ("phi", True), ("omega", False), ("omega", True))


# ---- 1 ----
@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_bits_of_the_model(nlev):
    from transport_se_amd.hip_mod import dss_view_plan
    h = _hip(NE, nlev)
    paths = set()
    for op, pgiven in CASES:
        nko = nlev + 1 if op == "pint" else nlev
        for i, name in enumerate(LAYOUTS):
            got = _run(h, op, pgiven, name, i)
            want = _want(nlev, op, pgiven)
            assert cm.same(got, want), (nlev, op, pgiven, name, int((cm.bits(got) != cm.bits(want)).sum()))
            paths.add((op, dss_view_plan(h.nelemd, 1, nko, layout(name, h.nelemd, 1, nko)[0], nlev=nlev)["path"]))
    assert {p for o, p in paths if o == "pint"} == {0, 2} and {p for o, p in paths if o == "phi"} == {0, 1, 2}
    for key in _input_keys(nlev):                           # the inputs keep their bits
        S, buf = _laid(*key)
        assert cm.same(buf.cpu().numpy(), S.host), key


def _input_keys(nlev):
    """the arguments of _laid that _inputs picks over CASES and LAYOUTS"""
    keys = set()
    for i in range(len(LAYOUTS)):
        for r, role in enumerate(ROLES):
            if role != "phis":
                keys.add((nlev, role, INPUTS[(i + r) % len(INPUTS)], 0))
        keys.add((nlev, "phis", ("dense", "ij", "dense_odd8")[i % 3], 0))
    return sorted(keys)


@pytest.mark.parametrize("op", ["phi", "omega"])
def test_without_p_is_pmid_and_then_the_op(op):
    """the pressure formed in the kernel has PMID's roundings: two calls through memory give the same bits as the fused one"""
    import torch
    for nlev in (72, 80):
        h = _hip(NE, nlev)
        f = _fields(nlev)
        for i, name in enumerate(("dense", "lev_even", "ij")):
            fused = _run(h, op, False, name, i)
            p = torch.full((h.nelemd, 4, 4, nlev), SENTINEL, dtype=torch.float64, device="cuda")        # level-fastest, as E3SM's GPU layouts
            kw = _inputs(nlev, op, False, i)
            h.column_view("pmid", dp=kw["dp"], out=p, out_axes="ejik", ptop=f["ptop"])
            assert cm.same(p.cpu().numpy().transpose(0, 3, 1, 2)[:, None], _want(nlev, "pmid", False))
            two = _run(h, op, True, name, i, dp=kw["dp"] if op == "phi" else None,
                       p=_Fake((h.nelemd, 4, 4, nlev), [16 * nlev, 4 * nlev, nlev, 1], p.data_ptr()), p_axes="ejik")
            assert cm.same(two, fused) and cm.same(fused, _want(nlev, op, False)), (nlev, op, name)


def test_surface_views_of_phis():
    """phis [e][j][i] (level stride 0), the bottom level of a larger level-fastest array with the level stride left at 1, and one level of
    a point-fastest array"""
    import torch
    from transport_se_amd import _lib
    nlev = 72
    h = _hip(NE, nlev)
    E = h.nelemd
    f = _fields(nlev)
    phis = f["phis"][:, 0, 0]
    want = _want(nlev, "phi", False)
    flat = torch.from_numpy(np.array(phis)).cuda()
    got = _run(h, "phi", False, "lev0", 1, b=flat, b_axes="eji")
    assert cm.same(got, want)
    S = nlev + 3
    big = np.full((E, 4, 4, S), SENTINEL); big[..., S - 1] = phis
    bigd = torch.from_numpy(big).cuda()
    for lev_stride in (1, 0):
        v = _lib.View(bigd.data_ptr() + 8 * (S - 1), (C.c_longlong * 5)(16 * S, 0, lev_stride, 4 * S, S))
        assert cm.same(_run(h, "phi", False, "dense", 2, b=v), want)
    pf = np.full((E, 5, 4, 4), SENTINEL); pf[:, 3] = phis
    pfd = torch.from_numpy(pf).cuda()
    assert cm.same(_run(h, "phi", True, "ij", 3, b=_Fake((E, 1, 4, 4), [80, 16, 4, 1], pfd.data_ptr() + 8 * 48), b_axes="ekji"), _want(nlev, "phi", True))
    assert cm.same(bigd.cpu().numpy(), big) and cm.same(pfd.cpu().numpy(), pf)


# ---- 2 ----
def test_the_device_lies_under_the_bound():
    nlev = 72
    h = _hip(NE, nlev)
    worst = {}
    for seed in (1, 2, 3):
        f = _fields(nlev, seed)
        for op, pgiven in CASES:
            got = cm.to_cols(_run(h, op, pgiven, "lev_even" if op != "pint" else "dense", seed, seed=seed))
            views = _model_views(op, f, pgiven)
            ref = cm.referee(op, f["ptop"], f["rgas"], **views)
            bnd = cm.bound(op, f["ptop"], f["rgas"], **views)
            err = np.abs(got.astype(np.longdouble) - ref)
            assert (bnd[err > 0] > 0).all()
            key = op + ("(p)" if pgiven else "")
            worst[key] = max(worst.get(key, 0.0), float(np.max(np.where(err > 0, err / np.where(bnd > 0, bnd, 1), 0))))
    for key, r in worst.items():
        print("tse_column_view: worst |device - referee| / bound, %-9s %.4f" % (key, r))
    assert all(0 < r < 1 for r in worst.values()), worst


# ---- 3 ----
def test_permuted_elements_and_one_changed_column():
    import torch
    nlev = 72
    h = _hip(NE, nlev)
    E = h.nelemd
    f = _fields(nlev)
    perm = np.random.default_rng(5).permutation(E)
    assert not np.array_equal(perm, np.arange(E))
    dev = lambda x: torch.from_numpy(np.array(x)).cuda()                              # (a copy: the shared fields are read-only)
    lf = lambda x: dev(np.moveaxis(np.asarray(x)[:, 0], 1, -1))                      # [e][j][i][k]

    def call(op, g, level_fastest):
        mk, ax = (lf, "ejik") if level_fastest else (lambda x: dev(np.asarray(x)[:, 0]), "ekji")
        nko = nlev + 1 if op == "pint" else nlev
        out = torch.full((E, nko, 4, 4), SENTINEL, dtype=torch.float64, device="cuda")
        kw = dict(dp=mk(g["dp"]), dp_axes=ax, out=out, out_axes="ekji", ptop=f["ptop"], rgas=f["rgas"])
        if op == "phi":
            kw.update(a=mk(g["tv"]), b=dev(g["phis"][:, 0, 0]), b_axes="eji")
        if op == "omega":
            kw.update(a=mk(g["vgrad_p"]), b=mk(g["divdp"]))
        h.column_view(op, **kw)
        return out.cpu().numpy()[:, None]

    arrays = ("dp", "tv", "phis", "vgrad_p", "divdp")
    for op in cm.OPS:
        for level_fastest in (False, True):
            base = call(op, f, level_fastest)
            assert cm.same(base, _want(nlev, op, False))
            moved = call(op, {k: f[k][perm] for k in arrays}, level_fastest)
            assert cm.same(moved, base[perm]) and not cm.same(moved, base)
            g = {k: np.array(f[k]) for k in arrays}
            e, j, i = 5, 2, 1
            for k in arrays:
                g[k][e, 0, :, j, i] *= 1.03125
            changed = cm.bits(call(op, g, level_fastest)) != cm.bits(base)
            only = np.zeros_like(changed); only[e, 0, :, j, i] = True
            assert not (changed & ~only).any(), (op, level_fastest, np.argwhere(changed & ~only)[:4])
            assert changed[e, 0, 1:, j, i].all(), (op, level_fastest)               # (pi[0] = ptop does not move)


# ---- 4 ----
LIB_FIELDS = ("qdp1", "qdp2", "dp", "divdp", "divdp_proj", "dp3d", "ps_v", "omega_p", "eta_dot_dpdn", "qmin", "qmax")
GROUPS = ("dss", "view", "level", "fieldremap", "fielddss", "fieldlap", "fieldvlap", "fieldop", "fieldstats", "remap", "advance", "minmax", "norms", "stateq")


def test_the_library_s_own_fields_and_untouched_state():
    import torch
    from gpu_common import elem_from_oracle
    from transport_se_amd.hip_mod import TseError
    nlev, dt = 72, 1800.0
    o = _oracle(NE)
    h = _make(NE)
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
        lib = lambda name: _Fake((E, nlev, 4, 4), [plane, 16, 4, 1], h.device_ptr(name)[0])
        ps = _Fake((E, 4, 4), [16, 4, 1], h.device_ptr("ps_v")[0])
        f = _fields(nlev)
        tv = torch.from_numpy(np.array(f["tv"][:, 0])).cuda()
        vg = torch.from_numpy(np.array(f["vgrad_p"][:, 0])).cuda()
        out = torch.full((E, nlev, 4, 4), SENTINEL, dtype=torch.float64, device="cuda")
        ptop, rgas = float(o.hyai[0]) * 1.0e5, f["rgas"]
        col = lambda x: np.moveaxis(np.asarray(x), 1, 0)
        dp3d, div = col(elem["dp3d"]), col(_raw(h, "divdp").reshape(E, nlev, 4, 4))
        h.column_view("pmid", dp=lib("dp3d"), out=out, ptop=ptop)
        assert cm.same(col(out.cpu().numpy()), cm.model("pmid", ptop, rgas, dp=dp3d))
        h.column_view("phi", dp=lib("dp3d"), a=tv, b=ps, b_axes="eji", out=out, ptop=ptop, rgas=rgas)
        assert cm.same(col(out.cpu().numpy()), cm.model("phi", ptop, rgas, dp=dp3d, a=col(f["tv"][:, 0]), b=elem["ps_v"]))
        h.column_view("omega", dp=lib("dp3d"), a=vg, b=lib("divdp"), out=out, ptop=ptop)
        assert cm.same(col(out.cpu().numpy()), cm.model("omega", ptop, rgas, dp=dp3d, a=col(f["vgrad_p"][:, 0]), b=div))
        assert h.kernel_time("fieldcol")[1] == 3 and h.kernel_time("fieldcol")[0] > 0.0
        for name in ("dp3d", "omega_p", "divdp", "dp", "qdp1", "qdp2", "eta_dot_dpdn"):
            with pytest.raises(TseError, match="out: .*lies inside an allocation of the library"):
                h.column_view("pmid", dp=tv, out=lib(name), ptop=ptop)
        assert h.kernel_time("fieldcol")[1] == 3
        for g in GROUPS:
            assert h.kernel_time(g)[1] == 0, g
        h.timing(False)
        for k in LIB_FIELDS:
            assert dm.same(_raw(h, k), before[k]), k
        assert all(dm.same(a, b) for a, b in zip(h.get_qminmax(), mm))
    finally:
        h.close()


# ---- 5 ----
def test_streams_and_refusals():
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    nlev = 72
    h = _hip(NE, nlev)
    E, plane = h.nelemd, nlev * 16
    f = _fields(nlev)
    ptop, rgas = f["ptop"], f["rgas"]
    host = np.array(f["dp"][:, 0])
    buf = torch.from_numpy(host).cuda()
    tv = torch.from_numpy(np.array(f["tv"][:, 0])).cuda()
    phis = torch.from_numpy(np.array(f["phis"][:, 0, 0])).cuda()
    keep = buf.clone()
    want = _want(nlev, "pmid", False)[:, 0]
    # a side stream orders producer and consumer without host synchronisation
    s = torch.cuda.Stream()
    made, out = torch.zeros_like(buf), torch.full_like(buf, SENTINEL)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        made.copy_(buf, non_blocking=True)
        h.column_view("pmid", dp=made, out=out, ptop=ptop, stream=s)
        took = out.clone()
        made.zero_(); out.zero_()
    s.synchronize()
    assert cm.same(took.cpu().numpy(), want)
    h.column_view("pmid", dp=buf, out=out, ptop=ptop)                                   # no stream: complete on return
    assert cm.same(out.cpu().numpy(), want)
    torch.cuda.synchronize()
    h.timing(True)

    def view(strides, ptr):
        return _lib.View(ptr, (C.c_longlong * 5)(*strides))
    raw = vc.RawAllocation(host.size * 8)
    beyond = raw.beyond
    dense, surf = [plane, 0, 16, 4, 1], [16, 0, 0, 4, 1]
    vd, vo, vt, vs = view(dense, buf.data_ptr()), view(dense, out.data_ptr()), view(dense, tv.data_ptr()), view(surf, phis.data_ptr())
    rawcall = lambda op, ptop_, rgas_, *v: h._chk(h.L.tse_column_view(h.h, op, ptop_, rgas_, *[None if x is None else C.byref(x) for x in v], None))
    nan, inf = float("nan"), float("inf")
    cases = [
        ("op=4", lambda: rawcall(4, ptop, rgas, vd, None, None, None, vo)),
        ("op=-1", lambda: rawcall(-1, ptop, rgas, vd, None, None, None, vo)),
        ("unknown op", lambda: h.column_view("pmax", dp=buf, out=out, ptop=ptop)),
        ("ptop = nan", lambda: rawcall(1, nan, rgas, vd, None, None, None, vo)),
        ("ptop = inf", lambda: rawcall(1, inf, rgas, vd, None, None, None, vo)),
        ("ptop = -1", lambda: rawcall(1, -1.0, rgas, vd, None, None, None, vo)),
        ("rgas = nan", lambda: rawcall(2, ptop, nan, vd, None, vt, vs, vo)),
        ("rgas = -inf", lambda: rawcall(2, ptop, -inf, vd, None, vt, vs, vo)),
        ("TSE_COL_PMID needs the view dp", lambda: rawcall(1, ptop, rgas, None, None, None, None, vo)),
        ("TSE_COL_PMID needs the view out", lambda: rawcall(1, ptop, rgas, vd, None, None, None, None)),
        ("TSE_COL_PINT takes no view p", lambda: rawcall(0, ptop, rgas, vd, vd, None, None, vo)),
        ("TSE_COL_PHI needs the view b", lambda: rawcall(2, ptop, rgas, vd, None, vt, None, vo)),
        ("TSE_COL_PHI needs the view a", lambda: rawcall(2, ptop, rgas, vd, None, None, vs, vo)),
        ("TSE_COL_OMEGA needs the view dp when p is null", lambda: rawcall(3, ptop, rgas, None, None, vt, vt, vo)),
        ("TSE_COL_OMEGA takes no view dp beside p", lambda: rawcall(3, ptop, rgas, vd, vd, vt, vt, vo)),
        (r"\(dp\).*device", lambda: h.column_view("pmid", dp=_Fake(host.shape, dense[:1] + dense[2:], host.ctypes.data), out=out, ptop=ptop)),
        (r"tse_column_view: .*device", lambda: h.column_view("pmid", dp=buf, out=_Fake(host.shape, dense[:1] + dense[2:], host.ctypes.data), ptop=ptop)),
        (r"\(a\).*outside its allocation", lambda: h.column_view("phi", dp=buf, a=_Fake(host.shape, dense[:1] + dense[2:], beyond), b=phis, out=out, ptop=ptop, rgas=rgas)),
        (r"tse_column_view: the view reaches.*outside its allocation", lambda: h.column_view("pmid", dp=buf, out=_Fake(host.shape, dense[:1] + dense[2:], beyond), ptop=ptop)),
        (r"\(b\).*not 8-byte aligned", lambda: rawcall(2, ptop, rgas, vd, None, vt, view(surf, phis.data_ptr() + 4), vo)),
        ("null view pointer", lambda: rawcall(1, ptop, rgas, view(dense, None), None, None, None, vo)),
        (r"stride 0 on the j axis.*\(out\)", lambda: rawcall(1, ptop, rgas, vd, None, None, None, view([plane, 0, 16, 0, 1], out.data_ptr()))),
        (r"out \[.*overlaps dp \[", lambda: rawcall(1, ptop, rgas, vd, None, None, None, vd)),
        (r"out \[.*overlaps a \[", lambda: rawcall(2, ptop, rgas, vd, None, vt, vs, view(dense, tv.data_ptr()))),
        (r"out \[.*overlaps b \[", lambda: rawcall(3, ptop, rgas, vd, None, vt, vo, vo)),
        ("out has 72 levels, pint wants 73", lambda: h.column_view("pint", dp=buf, out=out, ptop=ptop)),
        ("b has 72 levels, phi wants 1", lambda: h.column_view("phi", dp=buf, a=tv, b=tv, b_axes="ekji", out=out, ptop=ptop, rgas=rgas)),
    ]
    for text, call in cases:
        with pytest.raises(TseError, match=text):
            call()
        assert h.kernel_time("fieldcol")[1] == 0, text
    # a stream that is being captured
    torch.cuda.synchronize()
    with vc.capturing(s):
        with pytest.raises(TseError, match="captured"):
            h.column_view("pmid", dp=buf, out=out, ptop=ptop, stream=s)
    assert h.kernel_time("fieldcol")[1] == 0
    assert torch.equal(buf.view(torch.int64), keep.view(torch.int64))
    # out that fits its allocation exactly is served
    h.column_view("pmid", dp=buf, out=_Fake(host.shape, dense[:1] + dense[2:], raw.ptr), ptop=ptop)
    h.synchronize()
    back = raw.read(host.shape)
    assert cm.same(back, want) and h.kernel_time("fieldcol")[1] == 1
    h.timing(False)
    raw.free()


def _true_fma(a, b, c):
    """round(a * b + c) with one rounding, in fp64 operations alone (Boldo and Melquiond, 'Emulation of a FMA and correctly rounded sums:
    proved algorithms using rounding to odd', 2008): the exact product and the exact sum as pairs, the low parts added with rounding to
    odd, one final addition.  No overflow or underflow at the magnitudes of this test."""
    a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (a, b, c)))

    def split(x):
        t = 134217729.0 * x
        hi = t - (t - x)
        return hi, x - hi

    def two_sum(x, y):
        s = x + y
        bb = s - x
        return s, (x - (s - bb)) + (y - bb)
    uh = a * b
    ah, al = split(a)
    bh, bl = split(b)
    ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl
    th, tl = two_sum(c, uh)
    vh, vl = two_sum(tl, ul)
    # to odd: where the sum was inexact and the last bit of vh is even, one step towards the discarded part
    even = (vh.view(np.uint64) & np.uint64(1)) == 0
    v = np.where((vl != 0) & even, np.nextafter(vh, np.where(vl > 0, np.inf, -np.inf)), vh)
    return th + v


def test_the_true_fma_of_this_file():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(4000), rng.standard_normal(4000)
    c = -a * b * (1.0 + rng.integers(-4, 5, 4000) * 2.0 ** -52)        # heavy cancellation: the low part decides
    c[::2] = rng.standard_normal(2000)
    got = _true_fma(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        assert g == float(exact), (x, y, z)                            # (float(Fraction) rounds correctly)


def test_pressure_and_then_its_gradient_on_one_stream():
    """column_view("pmid") -> sphere_op_view("gradient") on the result, both on a side stream with nothing between them: the gradient of
    the model's p in the device's order of operations (sphere_ops_model.device_order, its fused multiply-adds true ones), bit for bit"""
    import torch
    import sphere_ops_model as som
    from vlaplace_model import host_fields
    nlev = 72
    h = _hip(NE, nlev)
    o = _oracle(NE)
    f = _fields(nlev)
    E = h.nelemd
    dp = torch.from_numpy(np.moveaxis(np.array(f["dp"][:, 0]), 1, -1).copy()).cuda()                 # dp3d [e][j][i][k]
    p = torch.full((E, 4, 4, nlev), SENTINEL, dtype=torch.float64, device="cuda")
    grad = torch.full((E, 2, nlev, 4, 4), SENTINEL, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    h.column_view("pmid", dp=dp, dp_axes="ejik", out=p, ptop=f["ptop"], stream=s)
    h.sphere_op_view(p, "ejik", grad, "eqkji", op="gradient", stream=s)
    s.synchronize()
    pm = _want(nlev, "pmid", False)
    assert cm.same(p.cpu().numpy().transpose(0, 3, 1, 2)[:, None], pm)
    # the same gradient of the model's p from memory: the two entries compose
    pd = torch.from_numpy(np.array(pm)).cuda()
    alone = torch.full_like(grad, SENTINEL)
    h.sphere_op_view(pd, "eqkji", alone, op="gradient")
    assert cm.same(grad.cpu().numpy(), alone.cpu().numpy())
    keep = som._fma
    som._fma = _true_fma
    try:
        want = som.device_order(o, host_fields(o)[0], "gradient", pm)
    finally:
        som._fma = keep
    got = grad.cpu().numpy()
    assert cm.same(got, want), int((cm.bits(got) != cm.bits(want)).sum())
