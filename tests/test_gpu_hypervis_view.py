"""-m gpu: tse_hypervis_view -- one hyperviscosity sub-step of a host's own scalars and wind in one call, in place or into out views.

The reference of every bit comparison is the loop the call replaces, on the dense layout of the same device: biharmonic_view /
vlaplace_view (order 2) -> the product with the field's factor in numpy float64 -> dss_view(mode="weak") -> the addition in numpy
float64; computed once per (mesh, nf, wind, nk) and shared.  What the numbers are is held by the bound against the reference's fixture.
 1 bits          ne2 / ne3, (nf, wind) in (3, yes), (1, no), (0, yes), nk in 1, 3, nlev, nlev + 1, in place and with out views, s and v in
                 layouts of every path independently; payload-filled gaps keep every bit, with out views s and v keep every bit
 2 fixture       the reference's ne2 fixture on the device under hypervis_model's bound
 3 independence  a level alone has the bits it has among nlev
 4 coefficients  a zero factor leaves its field; a factor times 2^+-k scales that field's tendency exactly
 5 untouched     the library's fields and timer groups, at most 5 launches per call, a second call allocates nothing
 6 levels        the 64- and 80-level libraries on the level-fastest path
 7 stream        producer -> hypervis_view -> consumer on one side stream; a stream under capture is refused
 8 ranks         3 contexts on one GPU through the callback exchange == one context, bit for bit; two exchanges per call
 9 refusals      nothing launched, the arrays unchanged"""
import ctypes as C
import functools

import numpy as np
import pytest

import biharmonic_model as bm
import dss_view_model as dm
import hypervis_model as hm
import view_common as vc
import vlaplace_model as vm
from view_common import FakeArray as _Fake, raw_field as _raw

pytestmark = pytest.mark.gpu
QSIZE = 2
SENTINEL = -7.25
COEF = (-3.1e21, -1.7e21, -2.3e21, -7.3e20)   # three scalar fields and the wind: distinct, no powers of two
NU = 2.5
COMBOS = ((3, True), (1, False), (0, True))


def _coef(nf, wind=True):
    return COEF[:nf] + ((COEF[3],) if wind else ())


def launches(nf, wind):
    return (2 if nf else 0) + (2 if wind else 0) + 1


@functools.lru_cache(maxsize=None)
def _oracle(ne):
    return vc.oracle(ne, QSIZE)


@functools.lru_cache(maxsize=None)
def _host(ne):
    return vm.host_fields(_oracle(ne))


def _make(ne, nlev=72, setup=True):
    return vc.make_hip(_oracle(ne), QSIZE, nlev, setup=_host(ne) if setup else None)


@functools.lru_cache(maxsize=None)
def _hip(ne, nlev=72):
    return _make(ne, nlev)


def compose(h, s, v, coef, nu=NU):
    """the loop the call replaces on dense arrays -> (s + ds, v + dv, ds, dv); None for an absent half"""
    import torch
    out = {}
    nf = 0 if s is None else s.shape[1]
    for key, x in (("s", s), ("v", v)):
        if x is None:
            out[key] = (None, None)
            continue
        t = torch.from_numpy(np.array(x)).cuda()
        if key == "s":
            h.biharmonic_view(t, "eqkji", order=2)
            fac = np.asarray(coef[:nf], dtype=np.float64).reshape(1, nf, 1, 1, 1)
        else:
            h.vlaplace_view(t, "eqkji", order=2, nu_ratio=nu)
            fac = np.float64(coef[nf])
        t = torch.from_numpy(np.ascontiguousarray(fac * t.cpu().numpy())).cuda()     # host_scale: one product
        h.dss_view(t, "eqkji", mode="weak")
        d = t.cpu().numpy()
        out[key] = (x + d, d)                                                        # host_add: one addition
    return out["s"][0], out["v"][0], out["s"][1], out["v"][1]


def _fields(n, nf, wind, nk, seed=0):
    s = bm.random_field(n, nf, nk, seed) if nf else None
    v = vm.random_field(n, nk, seed) if wind else None
    return s, v


@functools.lru_cache(maxsize=None)
def _case(ne, nf, wind, nk, nlev=72, seed=0):
    """(s, v, the composition's four results), shared and read-only"""
    h = _hip(ne, nlev)
    s, v = _fields(h.nelemd, nf, wind, nk, seed)
    want = compose(h, s, v, _coef(nf, wind))
    for a in (s, v) + want:
        if a is not None:
            a.setflags(write=False)
    return s, v, want


class _Side:
    """one operand on the device through a layout: the input x (or None), and with out_name a sentinel-filled out array"""
    def __init__(self, x, name, out_name):
        import torch
        self.x = x
        if x is None:
            self.vin = self.vout = None
            return
        self.S = dm.Strided(x, name)
        self.buf = torch.from_numpy(self.S.host.copy()).cuda()
        self.vin = _Fake(self.S.shape, self.S.s, self.buf.data_ptr() + 8 * self.S.base)
        self.vout = None
        if out_name is not None:
            self.T = dm.Strided(np.full(x.shape, SENTINEL), out_name)
            self.res = torch.from_numpy(self.T.host.copy()).cuda()
            self.vout = _Fake(self.T.shape, self.T.s, self.res.data_ptr() + 8 * self.T.base)

    def result(self, what):
        if self.x is None:
            return None
        if self.vout is None:
            got, gaps = self.S.read(self.buf.cpu().numpy())
        else:
            got, gaps = self.T.read(self.res.cpu().numpy())
            assert np.array_equal(dm.bits(self.buf.cpu().numpy()), dm.bits(self.S.host)), "%s changed" % what
        assert gaps, "bytes outside the view of %s changed" % what
        return got


def _run(h, s, v, sname, vname, coef, out=None, stream=None, nu=NU):
    """hypervis_view of host arrays through layouts, in place (out None) or into out arrays in the layouts out = (s_out, v_out) ->
    (s result, v result): the new state in place, the tendencies with out views"""
    import torch
    a = _Side(s, sname, None if out is None else out[0])
    b = _Side(v, vname, None if out is None else out[1])
    h.hypervis_view(a.vin, "eqkji", b.vin, "eqkji", coef=coef, nu_ratio=nu, s_out=a.vout, v_out=b.vout, stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    return a.result("s"), b.result("v")


def _same(a, b):
    return (a is None and b is None) or dm.same(a, b)


# ---- 1 ----
@pytest.mark.parametrize("ne", [2, 3])
def test_bits_of_the_composition(ne):
    from transport_se_amd.hip_mod import hypervis_view_plan
    h, nlev = _hip(ne), 72
    L = dm.LAYOUTS
    assert "lev_odd" in L and "lev_odd8" in L and "dense_odd8" in L
    for nf, wind in COMBOS:
        pairs = set()
        for nk in (1, 3, nlev, nlev + 1):
            s, v, (ws, wv, wds, wdv) = _case(ne, nf, wind, nk)
            for x, w in ((s, ws), (v, wv)):
                assert x is None or (not dm.same(x, w) and np.isfinite(w).all())
            for i, sname in enumerate(L):
                for shift in (3, 0, 5) if nk == nlev else (3,):      # (at nk == nlev the three shifts meet every pair of paths)
                    vname = L[(i + shift) % len(L)]
                    outs = (L[(i + 5) % len(L)], L[(i + 6) % len(L)])
                    plan = hypervis_view_plan(h.nelemd, nf, nk, dm.layout(sname, h.nelemd, nf, nk)[0] if nf else None,
                                              dm.layout(vname, h.nelemd, 2, nk)[0] if wind else None)
                    ps = plan["s"]["path"] if nf else None
                    pv = plan["v"]["path"] if wind else None
                    assert ps == (dm.expected_path(sname, nk, nlev) if nf else None) and pv == (dm.expected_path(vname, nk, nlev) if wind else None)
                    pairs.add((ps, pv))
                    gs, gv = _run(h, s, v, sname, vname, _coef(nf, wind))
                    assert _same(gs, ws) and _same(gv, wv), (ne, nf, wind, nk, sname, vname, "in place")
                    gs, gv = _run(h, s, v, sname, vname, _coef(nf, wind), out=outs)
                    assert _same(gs, wds) and _same(gv, wdv), (ne, nf, wind, nk, sname, vname, outs)
        want = {(a if nf else None, b if wind else None) for a in range(3) for b in range(3)}
        assert pairs >= want, (nf, wind, want - pairs)


# ---- 2 ----
def test_reference_fixture_on_the_device(gold):
    """the ne2 fixture of the reference's Fortran: the device under bound(N, A) of hypervis_model against the longdouble chain (ratio <= 1),
    every nu_ratio of the fixture.  Measured on the MI355X, worst error / bound: 0.018 for the scalars, 0.013 for the wind."""
    import elem_ops_ld as ld
    import fieldops_ref as fr
    from conftest import record_margin
    from transport_se_amd.hip_mod import HipMod
    assert ld.has_extended_precision(), np.finfo(np.longdouble)
    st, fx = gold("ref_ne2_static.npz"), gold("ref_ne2_fieldops.npz")
    st = {k: st[k] for k in st.files}
    fx = {k: fx[k] for k in fx.files}
    elem = dict(Dinv=st["Dinv"], metdet=st["metdet"], rmetdet=st["rmetdet"], spheremp=st["spheremp"], rspheremp=st["rspheremp"],
                putmapP=st["putmap"].astype(np.int32), getmapP=st["getmap"].astype(np.int32), reverse=st["reverse"].astype(np.int32))
    hip = HipMod(elem, st["Dvv"], (st["hyai"], st["hybi"], float(st["ps0"])), 3, 1e19, device=0)
    o = fr.mesh(st)
    try:
        geo = (st["D"], fx["metinv"], st["mp"])
        hip.vector_setup(*geo)
        s = np.ascontiguousarray(np.concatenate([fx["s"], fx["dss_average"]], axis=1))
        v = np.ascontiguousarray(fx["v"])
        assert s.shape == (24, 2, 3, 4, 4) and v.shape == (24, 2, 3, 4, 4)
        coef = (COEF[0], COEF[1], COEF[3])
        for nu in fx["nu_ratio"]:
            (rs, As), (rv, Av) = hm.longdouble(o, geo, s, v, coef, float(nu))
            for sname, vname in (("dense", "lev_even"), ("lev_even", "ij")):
                gs, gv = _run(hip, s, v, sname, vname, coef, nu=float(nu))
                for key, got, ref, A, wind in (("scalars", gs, rs, As, False), ("wind", gv, rv, Av, True)):
                    worst = float(hm.ratio(got, ref, A, wind).max())
                    print("hypervis_view fixture nu_ratio %.1f %s (%s, %s): worst error / bound(%d, A) = %.3f" % (nu, key, sname, vname, hm.steps(wind), worst))
                    record_margin("hypervis_view %s vs longdouble chain / bound(%d, A)" % (key, hm.steps(wind)), worst, 1.0)
                    assert worst <= 1.0, (nu, key, sname, vname, worst)
    finally:
        hip.close(); o.close()


# ---- 3 ----
def test_levels_are_independent():
    ne, nlev = 3, 72
    h = _hip(ne)
    s, v, (ws, wv, _, _) = _case(ne, 3, True, nlev)
    for sname, vname, out in (("dense", "lev0", None), ("lev0", "dense", None), ("ij", "epad", ("dense", "lev_even"))):
        bs, bv = _run(h, s, v, sname, vname, COEF, out=out)
        if out is None:
            assert dm.same(bs, ws) and dm.same(bv, wv)
        for k in (0, 37, nlev - 1):
            gs, gv = _run(h, np.ascontiguousarray(s[:, :, k:k + 1]), np.ascontiguousarray(v[:, :, k:k + 1]), sname, vname, COEF, out=out)
            assert dm.same(gs[:, :, 0], bs[:, :, k]) and dm.same(gv[:, :, 0], bv[:, :, k]), (sname, vname, k)


# ---- 4 ----
def test_coefficients():
    ne, nk = 2, 5
    h = _hip(ne)
    s, v = _fields(h.nelemd, 3, True, nk, seed=4)
    for sname, vname in (("dense", "lev_even"), ("ij", "dense_odd8")):
        base_s, base_v = _run(h, s, v, sname, vname, COEF)
        ds, dv = _run(h, s, v, sname, vname, COEF, out=("dense", "dense"))
        assert not dm.same(base_s, s) and not dm.same(base_v, v)
        # a zero factor: that field keeps every bit, the others are what they were
        for f in range(4):
            c = list(COEF); c[f] = 0.0
            gs, gv = _run(h, s, v, sname, vname, c)
            for g in range(3):
                assert dm.same(gs[:, g], s[:, g] if g == f else base_s[:, g]), (f, g)
            assert dm.same(gv, v if f == 3 else base_v), f
        # a factor times 2^+-k: that field's tendency times the same power, exactly
        for f, p in ((0, 7), (1, -9), (2, 30), (3, -30)):
            c = list(COEF); c[f] = float(np.ldexp(COEF[f], p))
            gs, gv = _run(h, s, v, sname, vname, c, out=("dense", "dense"))
            for g in range(3):
                assert dm.same(gs[:, g], np.ldexp(ds[:, g], p) if g == f else ds[:, g]), (f, g, p)
            assert dm.same(gv, np.ldexp(dv, p) if f == 3 else dv), (f, p)


# ---- 5 ----
LIB_FIELDS = ("qdp1", "qdp2", "dp", "q", "divdp", "divdp_proj", "dp3d", "ps_v", "qmin", "qmax")
GROUPS = ("dss", "lap", "view", "level", "fielddss", "fieldlap", "fieldvlap", "fieldop", "fieldremap", "fieldstats", "fieldcol", "remap", "advance", "minmax",
          "forcing", "stateq")


def test_the_library_is_untouched():
    ne, nlev, dt = 2, 72, 1800.0
    o = _oracle(ne)
    h, twin = _make(ne), _make(ne)
    try:
        for x in (h, twin):
            x.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm)
            x.dcmip_set_initial()
            x.dcmip_step_inputs(0, dt); x.advec_tracers_remap_rk2(dt, 1, 2)
            x.state_q(2)
        # the references first (they use the other entries' groups), then the timers on
        cases = [(nf, wind, nk, sname, vname, out, _case(ne, nf, wind, nk))
                 for nf, wind, nk, sname, vname, out in ((3, True, nlev, "lev0", "dense", None), (3, True, nlev, "dense", "ij", ("lev_even", "dense")),
                                                         (1, False, nlev, "epad", None, None), (0, True, 3, None, "lev_odd", None),
                                                         (3, True, nlev + 1, "dense", "dense", None), (3, True, nlev, "ij", "lev0", None))]
        before = {k: _raw(h, k) for k in LIB_FIELDS}
        assert h.device_ptr("view_stage") == (None, 0) and h.device_ptr("hypervis_stage") == (None, 0)
        h.timing(True)
        assert h.kernel_time("fieldhv") == (0.0, 0)
        total, stages = 0, []
        for nf, wind, nk, sname, vname, out, (s, v, (ws, wv, wds, wdv)) in cases:
            gs, gv = _run(h, s, v, sname, vname, _coef(nf, wind), out=out)
            assert _same(gs, ws if out is None else wds) and _same(gv, wv if out is None else wdv), (nf, wind, nk, sname, vname)
            total += launches(nf, wind)
            assert launches(nf, wind) <= 5 and h.kernel_time("fieldhv")[1] == total
            stages.append((h.device_ptr("view_stage"), h.device_ptr("hypervis_stage")))
        assert h.kernel_time("fieldhv")[0] > 0.0
        # layers per call: 360, 360, 72, 6 (smaller: reused), 365 (grows once), 360: a steady-state call allocates nothing
        assert stages[0] == stages[1] == stages[2] == stages[3] and stages[0][0][1] == stages[0][1][1] == h.nelemd * 360 * 128
        assert stages[4] == stages[5] and stages[4][0][1] == stages[4][1][1] == h.nelemd * 365 * 128
        for g in GROUPS:
            assert h.kernel_time(g)[1] == 0, g
        assert all(n == 0 for _, n in h.comm_times().values())
        h.timing(False)
        for k in LIB_FIELDS:
            assert dm.same(_raw(h, k), before[k]), k
        # the other view entries after it still give their own bits (the staging field is shared)
        s, v, (ws, wv, _, _) = _case(ne, 3, True, nlev)
        assert all(_same(a, b) for a, b in zip(compose(h, s, v, COEF), _case(ne, 3, True, nlev)[2]))
        for x in (h, twin):                                                      # the cached bounds survive: the next step is the twin's
            x.dcmip_step_inputs(1, dt); x.advec_tracers_remap_rk2(dt, 2, 1)
        shape = (h.nelemd, QSIZE, nlev, 4, 4)
        assert dm.same(h.fetch("qdp1", shape), twin.fetch("qdp1", shape))
        assert all(dm.same(a, b) for a, b in zip(h.get_qminmax(), twin.get_qminmax()))
    finally:
        h.close(); twin.close()


# ---- 6 ----
@pytest.mark.parametrize("nlev", [64, 80])
def test_other_level_counts(nlev):
    from transport_se_amd.hip_mod import hypervis_view_plan
    ne = 2
    h = _hip(ne, nlev)
    s, v, (ws, wv, wds, wdv) = _case(ne, 3, True, nlev, nlev)
    for sname, vname, out in (("lev0", "lev_odd", None), ("lev_odd8", "lev0", None), ("epad", "lev_even", ("lev_odd", "lev_odd8")), ("lev_even", "ij", ("lev0", "dense"))):
        plan = hypervis_view_plan(h.nelemd, 3, nlev, dm.layout(sname, h.nelemd, 3, nlev)[0], dm.layout(vname, h.nelemd, 2, nlev)[0], nlev=nlev)
        assert 1 in (plan["s"]["path"], plan["v"]["path"]), plan
        gs, gv = _run(h, s, v, sname, vname, COEF, out=out)
        assert dm.same(gs, ws if out is None else wds) and dm.same(gv, wv if out is None else wdv), (nlev, sname, vname, out)


# ---- 7 ----
def test_stream_order_and_capture():
    import torch
    from transport_se_amd.hip_mod import TseError
    ne, nlev = 3, 72
    h = _hip(ne)
    s, v, _ = _case(ne, 3, True, nlev)
    lev = lambda f: np.ascontiguousarray(np.moveaxis(f.reshape(f.shape[:3] + (16,)), 2, -1)).reshape(f.shape[0], f.shape[1], 4, 4, nlev)   # [e][q][j][i][k]
    xs, xv = (lev(s) - 1.0) / 2.0, (lev(v) - 1.0) / 2.0
    made = [x * 2.0 + 1.0 for x in (xs, xv)]                                   # what the device will hold: the host knows its bits
    ref = [torch.from_numpy(m.copy()).cuda() for m in made]
    h.hypervis_view(ref[0], "eqjik", ref[1], "eqjik", coef=COEF, nu_ratio=NU)  # stream=None: complete on return
    want = [r.cpu().numpy() for r in ref]
    assert not dm.same(want[0], made[0]) and not dm.same(want[1], made[1])
    st = torch.cuda.Stream()
    pinned = [torch.from_numpy(x).pin_memory() for x in (xs, xv)]
    field = [torch.zeros(p.shape, dtype=torch.float64, device="cuda") for p in pinned]
    out = [torch.zeros(p.shape, dtype=torch.float64, device="cuda") for p in pinned]
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for f, p in zip(field, pinned):
            f.copy_(p, non_blocking=True)
            f.mul_(2.0); f.add_(1.0)                                           # the producer
        h.hypervis_view(field[0], "eqjik", field[1], "eqjik", coef=COEF, nu_ratio=NU, stream=st)
        for o_, f in zip(out, field):
            o_.copy_(f, non_blocking=True)                                     # the consumer
            f.zero_()                                                          # the caller reuses its arrays at once
    torch.cuda.synchronize()
    assert dm.same(out[0].cpu().numpy(), want[0]) and dm.same(out[1].cpu().numpy(), want[1])
    assert not field[0].any().item() and not field[1].any().item()
    # a stream that is being captured
    h.timing(True)
    keep = [r.clone() for r in ref]
    torch.cuda.synchronize()
    with vc.capturing(st):
        with pytest.raises(TseError, match="captured"):
            h.hypervis_view(ref[0], "eqjik", ref[1], "eqjik", coef=COEF, stream=st)
    assert h.kernel_time("fieldhv")[1] == 0
    h.timing(False)
    assert all(torch.equal(r.view(torch.int64), k.view(torch.int64)) for r, k in zip(ref, keep))


# ---- 8 ----
RANK_CASES = ((72, "dense"), (73, "lev_odd"), (72, "lev0"), (1, "dense"))


def _rank_body(ne):
    from transport_se_amd import cube_mesh as cm
    nelem = 6 * ne * ne

    def body(rank, h, mine, geo, hv):
        out = {}
        h.vector_setup(geo["D"][mine], cm.metinv(geo["D"])[mine], geo["mp"][mine])
        h.comm_timing(True)
        done = 0
        for nk, name in RANK_CASES:
            s, v = _fields(nelem, 3, True, nk, seed=7)
            for mode in (None, ("dense", name)):
                out[(nk, name, mode is None)] = _run(h, s[mine], v[mine], name, "dense" if name != "dense" else "lev_even", COEF, out=mode)
                done += 1
                out[("exchanges", done)] = h.comm_times()["comm_exchange_q"][1]
        h.comm_timing(False)
        return out
    return body


@pytest.mark.parametrize("ne", [3, 4])
def test_ranks_give_the_bits_of_one_context(ne):
    from test_gpu_multirank_emulated import _run_ne
    nelem = 6 * ne * ne
    (mine1, one), = _run_ne(1, ne=ne, body=_rank_body(ne))
    assert np.array_equal(np.sort(mine1), np.arange(nelem))
    ncalls = 2 * len(RANK_CASES)
    assert all(one.pop(("exchanges", i)) == 0 for i in range(1, ncalls + 1))
    full = {}
    for key, (gs, gv) in one.items():
        fs, fv = np.empty_like(gs), np.empty_like(gv)
        fs[mine1] = gs; fv[mine1] = gv
        full[key] = (fs, fv)
    res = _run_ne(3, ne=ne, body=_rank_body(ne))
    assert all(r is not None for r in res)
    for mine, r in res:
        for i in range(1, ncalls + 1):
            assert r[("exchanges", i)] == 2 * i, (i, r[("exchanges", i)])       # halo_exchange exactly twice per call
    for key, want in full.items():
        for j in range(2):
            got = np.empty_like(want[j])
            for mine, r in res:
                got[mine] = r[key][j]
            assert dm.same(got, want[j]), (ne, key, "sv"[j], int((dm.bits(got) != dm.bits(want[j])).sum()))


# ---- 9 ----
def test_refusals_launch_nothing():
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    ne, nlev, nf = 2, 72, 3
    h = _hip(ne)
    s, v, (ws, wv, wds, wdv) = _case(ne, nf, True, nlev)
    E, plane = h.nelemd, nlev * 16
    ds_, dv_ = [nf * plane, plane, 16, 4, 1], [2 * plane, plane, 16, 4, 1]
    big = torch.full((s.size + v.size + 64,), SENTINEL, dtype=torch.float64, device="cuda")   # s, then v right behind it, then room
    big[:s.size] = torch.from_numpy(np.array(s)).reshape(-1).cuda()
    big[s.size:s.size + v.size] = torch.from_numpy(np.array(v)).reshape(-1).cuda()
    ts, tv = big[:s.size].view(s.shape), big[s.size:s.size + v.size].view(v.shape)
    os_ = torch.full(s.shape, SENTINEL, dtype=torch.float64, device="cuda")
    ov_ = torch.full(v.shape, SENTINEL, dtype=torch.float64, device="cuda")
    keep, keep_os, keep_ov = big.clone(), os_.clone(), ov_.clone()
    host = np.array(s)

    def view(strides, ptr):
        return _lib.View(ptr, (C.c_longlong * 5)(*strides))
    ps, pv = ts.data_ptr(), tv.data_ptr()
    VS, VV = view(ds_, ps), view(dv_, pv)
    hv = lambda **kw: h.hypervis_view(**dict(dict(s=ts, s_axes="eqkji", v=tv, v_axes="eqkji", coef=COEF), **kw))
    # before vector_setup: a context of its own
    bare = _make(ne, setup=False)
    try:
        bare.timing(True)
        with pytest.raises(TseError, match="tse_vector_setup first"):
            bare.hypervis_view(ts, "eqkji", tv, "eqkji", coef=COEF)
        assert bare.kernel_time("fieldhv")[1] == 0 and bare.device_ptr("hypervis_stage") == (None, 0)
        assert torch.equal(big.view(torch.int64), keep.view(torch.int64))
        bare.hypervis_view(ts, "eqkji", coef=COEF[:3], s_out=os_)                # ... the scalars alone need none
        assert dm.same(os_.cpu().numpy(), wds) and bare.kernel_time("fieldhv")[1] == launches(3, False)
        os_.copy_(keep_os)
    finally:
        bare.close()
    q1, nbytes = h.device_ptr("qdp1")
    libview = _Fake((E, QSIZE, nlev, 4, 4), [QSIZE * plane, plane, 16, 4, 1], q1)
    h.hypervis_view(os_, "eqkji", ov_, "eqkji", coef=COEF)                       # (the staging fields exist from here on)
    os_.copy_(keep_os); ov_.copy_(keep_ov)
    h.timing(True)
    st1, _ = h.device_ptr("view_stage")
    st2, st2bytes = h.device_ptr("hypervis_stage")
    assert st1 and st2 and st2bytes >= (s.size + v.size) * 8
    nan, inf = float("nan"), float("inf")
    cases = [
        ("device", lambda: hv(s=_Fake(s.shape, ds_, host.ctypes.data))),
        ("device", lambda: hv(s_out=_Fake(s.shape, ds_, host.ctypes.data), v_out=ov_)),
        ("s: .* allocation of the library", lambda: h.hypervis_view(libview, "eqkji", coef=COEF[:2], s_out=os_[:, :2])),
        ("v_out: .* allocation of the library", lambda: hv(s_out=os_, v_out=libview)),
        ("s_out: .* allocation of the library", lambda: hv(s_out=_Fake(s.shape, ds_, st2), v_out=ov_)),      # the second staging field itself
        ("v_out: .* allocation of the library", lambda: hv(s_out=os_, v_out=_Fake(v.shape, dv_, st1))),      # the first
        ("nu_ratio = nan", lambda: hv(nu_ratio=nan)),
        ("nu_ratio = inf", lambda: hv(nu_ratio=inf)),
        (r"coef\[1\] = nan", lambda: hv(coef=(COEF[0], nan, COEF[2], COEF[3]))),
        (r"coef\[3\] = -inf.*wind", lambda: hv(coef=COEF[:3] + (-inf,))),
        ("factors in coef", lambda: hv(coef=COEF[:2])),
        ("nk = 0", lambda: h.hypervis_view(VS, None, VV, None, coef=COEF, nf=nf, nk=0)),
        ("nk = %d" % (nlev + 2), lambda: h.hypervis_view(VS, None, VV, None, coef=COEF, nf=nf, nk=nlev + 2)),
        ("nf = 65", lambda: h.hypervis_view(VS, None, VV, None, coef=[1.5] * 66, nf=65, nk=1)),
        ("extent 3, not 2", lambda: hv(v=ts)),
        ("neither s nor v", lambda: h.hypervis_view(coef=COEF)),
        ("v has 5 levels, s has", lambda: hv(v=tv[:, :, :5])),
        ("s_out is given and s is not", lambda: h.hypervis_view(v=tv, v_axes="eqkji", coef=COEF[3:], s_out=os_, v_out=ov_)),
        ("v is given and v_out is not", lambda: hv(s_out=os_)),
        ("s is given and s_out is not", lambda: hv(v_out=ov_)),
        ("out has 2 fields", lambda: hv(s_out=os_[:, :2], v_out=ov_)),
        (r"stride 0 on the j axis.*\(s\)", lambda: h.hypervis_view(view([nf * plane, plane, 16, 0, 1], ps), None, VV, None, coef=COEF, nf=nf, nk=nlev)),
        (r"stride 0 on the q axis.*\(v_out\)", lambda: h.hypervis_view(VS, None, VV, None, coef=COEF, nf=nf, nk=nlev, s_out=view(ds_, os_.data_ptr()),
                                                                       v_out=view([2 * plane, 0, 16, 4, 1], ov_.data_ptr()))),
        (r"overlap itself.*\(v\)", lambda: h.hypervis_view(VS, None, view([2 * plane, plane // 2, 16, 4, 1], pv), None, coef=COEF, nf=nf, nk=nlev)),
        ("v .* overlaps s ", lambda: h.hypervis_view(VS, None, view(dv_, pv - 8), None, coef=COEF, nf=nf, nk=nlev)),        # one double shared
        ("s_out .* overlaps s ", lambda: h.hypervis_view(VS, None, VV, None, coef=COEF, nf=nf, nk=nlev, s_out=view(ds_, ps + 8 * 16), v_out=view(dv_, ov_.data_ptr()))),
        ("v_out .* overlaps v ", lambda: h.hypervis_view(VS, None, VV, None, coef=COEF, nf=nf, nk=nlev, s_out=view(ds_, os_.data_ptr()), v_out=VV)),
        ("v_out .* overlaps s_out ", lambda: h.hypervis_view(VS, None, VV, None, coef=COEF, nf=nf, nk=nlev, s_out=view(ds_, os_.data_ptr()),
                                                             v_out=view(dv_, os_.data_ptr() + 8 * plane))),
        ("null view pointer", lambda: h.hypervis_view(view(ds_, None), None, VV, None, coef=COEF, nf=nf, nk=nlev)),
        ("not 8-byte aligned", lambda: h.hypervis_view(VS, None, view(dv_, pv + 4), None, coef=COEF, nf=nf, nk=nlev)),
    ]
    for text, call in cases:
        print("hypervis_view refusal:", text)
        with pytest.raises(TseError, match=text):
            call()
        assert h.kernel_time("fieldhv")[1] == 0, text
        assert torch.equal(big.view(torch.int64), keep.view(torch.int64)), text
        assert torch.equal(os_.view(torch.int64), keep_os.view(torch.int64)) and torch.equal(ov_.view(torch.int64), keep_ov.view(torch.int64)), text
    L = h.L
    c3 = (C.c_double * 4)(*COEF)
    assert L.tse_hypervis_view(h.h, nf, nlev, None, 1.0, C.byref(VS), C.byref(VV), None, None, None) != 0 and b"null coef" in L.tse_last_error()
    assert L.tse_hypervis_view(h.h, nf, nlev, c3, 1.0, None, None, None, None, None) != 0 and b"needs the view s" in L.tse_last_error()
    assert L.tse_hypervis_view(h.h, 0, nlev, c3, 1.0, None, None, None, None, None) != 0 and b"nothing to do" in L.tse_last_error()
    assert h.kernel_time("fieldhv")[1] == 0
    # good calls afterwards: v touches the end of s (they lie behind one another), with out views, then in place
    h.hypervis_view(VS, None, VV, None, coef=COEF, nu_ratio=NU, nf=nf, nk=nlev, s_out=view(ds_, os_.data_ptr()), v_out=view(dv_, ov_.data_ptr()))
    assert h.kernel_time("fieldhv")[1] == 5
    assert dm.same(os_.cpu().numpy(), wds) and dm.same(ov_.cpu().numpy(), wdv) and torch.equal(big.view(torch.int64), keep.view(torch.int64))
    hv(nu_ratio=NU)
    assert h.kernel_time("fieldhv")[1] == 10 and dm.same(ts.cpu().numpy(), ws) and dm.same(tv.cpu().numpy(), wv)
    assert torch.equal(big[s.size + v.size:], keep[s.size + v.size:])
    h.timing(False)
