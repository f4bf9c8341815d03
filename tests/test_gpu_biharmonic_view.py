"""-m gpu: tse_biharmonic_view -- the weak Laplacian (order 1) and the weak biharmonic (order 2) of a host's own device arrays through
strided views, in place or into a second view.

The reference of every bit comparison is the composition of the entries the library had before: HipMod.laplace_sphere_wk on every layer,
HipMod.dss_view(mode="weak"), HipMod.laplace_sphere_wk on every layer -- computed once per (mesh, nf, nk, order) and shared.
 1 bits        both orders, ne2 / ne3, (nf, nk) in (2, nlev), (1, nlev + 1), (3, 1), (1, 2): `in` in every layout, `out` in place and a
               separate array in a layout of each other path; NaN-filled gaps keep every bit, a separate `in` keeps every bit
 2 bound       the device result under biharmonic_model's bound(19, A) / bound(42, A) against the longdouble chain
 3 linearity   the input times 2^+-200 gives the output times the same power, bit for bit
 4 layers      a permutation of the layers permutes the output; a layer alone has the bits it has among 2 * nlev
 5 levels      the 64- and 80-level libraries on the level-fastest path
 6 untouched   the library's fields and timer groups, the launch count, the shared staging buffer, an interleaved dss_view
 7 stream      producer -> biharmonic_view -> consumer on one side stream; a stream under capture is refused
 8 ranks       2 and 3 contexts on one GPU through the callback exchange == one context, bit for bit; order 1 exchanges nothing
 9 refusals    nothing launched, the arrays unchanged"""
import ctypes as C
import functools

import numpy as np
import pytest

import biharmonic_model as bm
import dss_view_model as dm
import view_common as vc
from view_common import FakeArray as _Fake, raw_field as _raw

pytestmark = pytest.mark.gpu
QSIZE = 2
LAUNCHES = 2   # per call, either order: k_lap_view_stage and k_lap_view_out
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def _oracle(ne):
    return vc.oracle(ne, QSIZE)


def _make(ne, nlev=72):
    return vc.make_hip(_oracle(ne), QSIZE, nlev)


@functools.lru_cache(maxsize=None)
def _hip(ne, nlev=72):
    """a context of qsize 2 on the oracle's mesh (kept for the session: contexts are small)"""
    return _make(ne, nlev)


def compose(h, f, order):
    """the entries the library had before, one after the other: f[n][nf][nk][4][4] -> the same shape"""
    import torch
    f = np.asarray(f)
    n = f.shape[0]

    def lap(x):
        x = x.reshape(n, -1, 4, 4)
        return np.stack([h.laplace_sphere_wk(np.ascontiguousarray(x[:, l])) for l in range(x.shape[1])], axis=1).reshape(f.shape)
    w = lap(f)
    if order == 2:
        t = torch.from_numpy(w).cuda()
        h.dss_view(t, "eqkji", mode="weak")
        w = lap(t.cpu().numpy())
    return w


@functools.lru_cache(maxsize=None)
def _case(ne, nf, nk, order, nlev=72, seed=0):
    """(field, the composition's result), shared and read-only"""
    h = _hip(ne, nlev)
    f = bm.random_field(h.nelemd, nf, nk, seed)
    want = compose(h, f, order)
    f.setflags(write=False); want.setflags(write=False)
    return f, want


def _run(h, f, name, order, out_name=None, stream=None):
    """biharmonic_view of a host array through a layout, in place (out_name None) or into a second array -> the result; every gap keeps
    its bits, and with a separate out the whole of `in` does"""
    import torch
    S = dm.Strided(f, name)
    buf = torch.from_numpy(S.host.copy()).cuda()
    vin = _Fake(S.shape, S.s, buf.data_ptr() + 8 * S.base)
    if out_name is None:
        h.biharmonic_view(vin, "eqkji", order=order, stream=stream)
        T, res = S, buf
    else:
        T = dm.Strided(np.full(f.shape, SENTINEL), out_name)
        res = torch.from_numpy(T.host.copy()).cuda()
        h.biharmonic_view(vin, "eqkji", out=_Fake(T.shape, T.s, res.data_ptr() + 8 * T.base), order=order, stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    got, gaps = T.read(res.cpu().numpy())
    assert gaps, "bytes outside the out view changed (%s -> %s)" % (name, out_name)
    if out_name is not None:
        assert np.array_equal(dm.bits(buf.cpu().numpy()), dm.bits(S.host)), "in changed (%s -> %s)" % (name, out_name)
    return got


# ---- 1 ----
OUT_REPS = ("epad", "lev_even", "ij")        # a layout of each path at nk == nlev (a level-fastest one of another depth is generic)
OUT_ODD = ("dense_odd8", "lev_odd8")         # the 8-byte accesses on the out side


@pytest.mark.parametrize("order", bm.ORDERS)
@pytest.mark.parametrize("ne", [2, 3])
def test_bits_of_the_composition(ne, order):
    from transport_se_amd.hip_mod import biharmonic_view_plan
    h, nlev = _hip(ne), 72
    pairs = set()
    for nf, nk in ((2, nlev), (1, nlev + 1), (3, 1), (1, 2)):
        f, want = _case(ne, nf, nk, order)
        assert not dm.same(f, want)
        for i, name in enumerate(dm.LAYOUTS):
            pin = dm.expected_path(name, nk, nlev)
            outs = [None] + [r for r in OUT_REPS if dm.expected_path(r, nk, nlev) != pin] + [OUT_ODD[i % 2]]
            for out_name in outs:
                pout = pin if out_name is None else dm.expected_path(out_name, nk, nlev)
                plan = biharmonic_view_plan(h.nelemd, nf, nk, dm.layout(name, h.nelemd, nf, nk)[0],
                                            None if out_name is None else dm.layout(out_name, h.nelemd, nf, nk)[0])
                assert [p["path"] for p in plan] == [pin, pout], (name, out_name, plan)
                pairs.add((pin, pout))
                got = _run(h, f, name, order, out_name)
                assert dm.same(got, want), (ne, order, nf, nk, name, out_name, int((dm.bits(got) != dm.bits(want)).sum()))
    assert pairs == {(a, b) for a in range(3) for b in range(3)}, pairs
    if order == 2:
        assert not dm.same(_case(ne, 2, nlev, 1)[1], _case(ne, 2, nlev, 2)[1])


def test_a_surface_field_and_a_layer_field_without_their_unit_axes():
    """a missing q or k letter: extent 1 and stride 0; out in other axes than in"""
    import torch
    ne, nlev = 2, 72
    h = _hip(ne)
    f, want = _case(ne, 1, 1, 2)
    ps = torch.from_numpy(np.array(f[:, 0, 0])).cuda()                        # [e][j][i]
    h.biharmonic_view(ps, "eji")
    assert dm.same(ps.cpu().numpy(), want[:, 0, 0])
    f, want = _case(ne, 1, nlev, 2)
    T = torch.from_numpy(np.ascontiguousarray(np.moveaxis(f[:, 0], 1, -1))).cuda()   # [e][j][i][k]
    out = torch.full((h.nelemd, nlev, 4, 4), SENTINEL, dtype=torch.float64, device="cuda")   # [e][k][j][i]
    h.biharmonic_view(T, "ejik", out=out, out_axes="ekji", order="biharmonic")
    assert dm.same(out.cpu().numpy(), want[:, 0])
    h.biharmonic_view(T, "ejik", order="laplace")
    assert dm.same(np.ascontiguousarray(np.moveaxis(T.cpu().numpy(), -1, 1)), _case(ne, 1, nlev, 1)[1][:, 0])


# ---- 2 ----
@pytest.mark.parametrize("ne", [2, 3])
def test_pointwise_bound(ne):
    """|device - longdouble chain| <= bound(19, A) (order 1), bound(42, A) (order 2) at every point.  Measured on the MI355X, worst
    error / bound: order 1 0.142 (random) and 0.015 (smooth), order 2 0.028 and 0.003; the oracle's own fp64 composition reaches 0.128
    (order 1) and 0.030 (order 2) in test_biharmonic_view_cpu.py."""
    import elem_ops_ld as ld
    assert ld.has_extended_precision(), np.finfo(np.longdouble)
    h, o = _hip(ne), _oracle(ne)
    nf, nk = 1, 3
    for kind, f in (("random", bm.random_field(o.nelem, nf, nk, seed=3)), ("smooth", bm.smooth_field(o, nf, nk))):
        for order in bm.ORDERS:
            ref, A = bm.longdouble(o, f, order)
            for name in ("dense", "ij"):
                got = _run(h, f, name, order)
                worst = float(bm.ratio(got, ref, A, order).max())
                print("biharmonic_view ne%d order %d %s %s: worst error / bound = %.3f" % (ne, order, kind, name, worst))
                assert worst < 1.0, (ne, order, kind, name, worst)


# ---- 3 ----
@pytest.mark.parametrize("order", bm.ORDERS)
def test_linearity_in_powers_of_two(order):
    """values of order 300 times 2^+-200: the second Laplacian's results are of order 1e-20 times that, far from both ends of the range"""
    ne, nf, nk = 2, 2, 5
    h = _hip(ne)
    f = bm.random_field(h.nelemd, nf, nk, seed=5)
    for name, out_name in (("dense", None), ("lev_even", "ij")):
        base = _run(h, f, name, order, out_name)
        assert np.isfinite(base).all() and (np.abs(base) > 1e-200).all()
        for p in (200, -200):
            got = _run(h, np.ldexp(f, p), name, order, out_name)
            assert dm.same(got, np.ldexp(base, p)), (order, name, p)
            assert np.isfinite(got).all() and (np.abs(got) > 2.0 ** -900).all()


# ---- 4 ----
@pytest.mark.parametrize("order", bm.ORDERS)
def test_layers_are_independent(order):
    ne, nlev = 3, 72
    h = _hip(ne)
    nf, nk = 2, nlev
    f = np.array(_case(ne, nf, nk, order)[0])
    n = f.shape[0]
    perm = np.random.default_rng(11).permutation(nf * nk)
    assert (perm != np.arange(nf * nk)).any()
    fp = np.ascontiguousarray(f.reshape(n, nf * nk, 4, 4)[:, perm]).reshape(f.shape)
    for name, out_name in (("dense", None), ("lev0", None), ("ij", "dense")):
        base = _run(h, f, name, order, out_name)
        got = _run(h, fp, name, order, out_name)
        assert dm.same(got.reshape(n, nf * nk, 4, 4), base.reshape(n, nf * nk, 4, 4)[:, perm]), (order, name)
        for q, k in ((0, 0), (1, 37), (1, nlev - 1)):                          # a layer alone: nf = nk = 1
            one = _run(h, np.ascontiguousarray(f[:, q:q + 1, k:k + 1]), name, order, out_name)
            assert dm.same(one[:, 0, 0], base[:, q, k]), (order, name, q, k)


# ---- 5 ----
@pytest.mark.parametrize("nlev", [64, 80])
def test_other_level_counts(nlev):
    from transport_se_amd.hip_mod import biharmonic_view_plan
    ne, nf = 2, 2
    h = _hip(ne, nlev)
    for order in bm.ORDERS:
        f, want = _case(ne, nf, nlev, order, nlev)
        for name, out_name in (("lev0", None), ("lev_odd", None), ("lev_odd8", "dense"), ("epad", "lev_even")):
            plan = biharmonic_view_plan(h.nelemd, nf, nlev, dm.layout(name, h.nelemd, nf, nlev)[0],
                                        None if out_name is None else dm.layout(out_name, h.nelemd, nf, nlev)[0], nlev=nlev)
            assert 1 in [p["path"] for p in plan], plan
            assert dm.same(_run(h, f, name, order, out_name), want), (nlev, order, name, out_name)


# ---- 6 ----
LIB_FIELDS = ("qdp1", "qdp2", "dp", "q", "divdp", "divdp_proj", "dp3d", "ps_v", "qmin", "qmax")
GROUPS = ("dss", "lap", "view", "level", "fielddss", "fieldremap", "remap", "advance", "minmax", "forcing", "stateq")


def test_the_library_is_untouched():
    import torch
    ne, nlev, dt = 2, 72, 1800.0
    o = _oracle(ne)
    h, twin = _make(ne), _make(ne)
    try:
        for x in (h, twin):
            x.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm)
            x.dcmip_set_initial()
            x.dcmip_step_inputs(0, dt); x.advec_tracers_remap_rk2(dt, 1, 2)      # leaves the element bounds of Qdp(2) cached
            x.state_q(2)                                                          # "q" and "lnps" exist and are fresh
        before = {k: _raw(h, k) for k in LIB_FIELDS}
        assert h.device_ptr("view_stage") == (None, 0)
        h.timing(True)
        assert h.kernel_time("fieldlap") == (0.0, 0)
        calls, stage = 0, []
        # layers per call: 144, 144, 73 (smaller: reused), 144, then 365 (grows once), 365, 144
        for nf, nk, name, out_name, order in ((2, nlev, "lev0", None, 2), (2, nlev, "dense", "ij", 1), (1, nlev + 1, "ij", None, 2), (2, nlev, "epad", "lev_even", 2),
                                              (5, nlev + 1, "dense", None, 2), (5, nlev + 1, "lev_even", "dense", 1), (2, nlev, "lev0", None, 1)):
            f, want = _case(ne, nf, nk, order)
            assert dm.same(_run(h, f, name, order, out_name), want), (nf, nk, name, out_name, order)
            calls += 1
            assert h.kernel_time("fieldlap")[1] == LAUNCHES * calls
            stage.append(h.device_ptr("view_stage"))
        assert h.kernel_time("fieldlap")[0] > 0.0
        assert stage[0] == stage[1] == stage[2] == stage[3] and stage[0][1] == h.nelemd * 144 * 128
        assert stage[4] == stage[5] == stage[6] and stage[4][1] == h.nelemd * 365 * 128
        for g in GROUPS:
            assert h.kernel_time(g)[1] == 0, g
        # an interleaved dss_view of another layer count still gives its own bits, and the next biharmonic its own
        w = dm.field(h.nelemd, 3, 7)
        t = torch.from_numpy(w.copy()).cuda()
        h.dss_view(t, "eqkji", mode="average")
        assert dm.same(t.cpu().numpy(), dm.model(o, w, "average"))
        f, want = _case(ne, 1, nlev + 1, 2)
        assert dm.same(_run(h, f, "dense", 2), want)
        assert h.device_ptr("view_stage") == stage[4] and h.kernel_time("fielddss")[1] == 2
        h.timing(False)
        for k in LIB_FIELDS:
            assert dm.same(_raw(h, k), before[k]), k
        for x in (h, twin):                                                      # the cached bounds survive: the next step is the twin's
            x.dcmip_step_inputs(1, dt); x.advec_tracers_remap_rk2(dt, 2, 1)
        shape = (h.nelemd, QSIZE, nlev, 4, 4)
        assert dm.same(h.fetch("qdp1", shape), twin.fetch("qdp1", shape))
        assert all(dm.same(a, b) for a, b in zip(h.get_qminmax(), twin.get_qminmax()))
    finally:
        h.close(); twin.close()


# ---- 7 ----
def test_stream_order_and_capture():
    import torch
    from transport_se_amd.hip_mod import TseError
    ne, nlev, nf = 3, 72, 2
    h = _hip(ne)
    f, _ = _case(ne, nf, nlev, 2)
    lf = np.ascontiguousarray(np.moveaxis(f.reshape(f.shape[:3] + (16,)), 2, -1)).reshape(f.shape[0], nf, 4, 4, nlev)   # [e][q][j][i][k]
    x = (lf - 1.0) / 2.0
    made = x * 2.0 + 1.0                                                       # what the device will hold: the host knows its bits
    ref = torch.from_numpy(made.copy()).cuda()
    h.biharmonic_view(ref, "eqjik")                                            # stream=None: complete on return
    want = ref.cpu().numpy()
    assert not dm.same(want, made)
    s = torch.cuda.Stream()
    pinned = torch.from_numpy(x).pin_memory()
    for separate in (False, True):
        field = torch.zeros(pinned.shape, dtype=torch.float64, device="cuda")
        res = torch.zeros(pinned.shape, dtype=torch.float64, device="cuda") if separate else field
        out = torch.zeros(pinned.shape, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            field.copy_(pinned, non_blocking=True)
            field.mul_(2.0); field.add_(1.0)                                   # the producer
            h.biharmonic_view(field, "eqjik", out=res if separate else None, stream=s)
            out.copy_(res, non_blocking=True)                                  # the consumer
            field.zero_(); res.zero_()                                         # the caller reuses its arrays at once
        torch.cuda.synchronize()
        assert dm.same(out.cpu().numpy(), want) and not res.any().item(), separate
    # a stream that is being captured
    h.timing(True)
    keep = ref.clone()
    torch.cuda.synchronize()
    with vc.capturing(s):
        with pytest.raises(TseError, match="captured"):
            h.biharmonic_view(ref, "eqjik", stream=s)
    assert h.kernel_time("fieldlap")[1] == 0
    h.timing(False)
    assert torch.equal(ref.view(torch.int64), keep.view(torch.int64))


# ---- 8 ----
RANK_CASES = ((2, 72, "dense"), (1, 73, "lev_odd"), (3, 1, "dense"))


def _rank_body(ne):
    nelem = 6 * ne * ne

    def body(rank, h, mine, geo, hv):
        out = {}
        h.comm_timing(True)
        for order in bm.ORDERS:
            for nf, nk, name in RANK_CASES:
                f = bm.random_field(nelem, nf, nk, seed=7)[mine]
                out[(nf, nk, name, order)] = _run(h, f, name, order)
            out[("comm", order)] = sum(v[1] for v in h.comm_times().values())
        h.comm_timing(False)
        return out
    return body


@pytest.mark.parametrize("ne", [3, 4])
def test_ranks_give_the_bits_of_one_context(ne):
    from test_gpu_multirank_emulated import _run_ne
    nelem = 6 * ne * ne
    (mine1, one), = _run_ne(1, ne=ne, body=_rank_body(ne))
    assert np.array_equal(np.sort(mine1), np.arange(nelem))
    assert one.pop(("comm", 1)) == 0 and one.pop(("comm", 2)) == 0
    for key, val in one.items():
        full = np.empty_like(val); full[mine1] = val
        one[key] = full
    for world in (2, 3):
        res = _run_ne(world, ne=ne, body=_rank_body(ne))
        assert all(r is not None for r in res), world
        for mine, r in res:
            assert r[("comm", 1)] == 0, (world, r[("comm", 1)])               # order 1 exchanges nothing
            assert r[("comm", 2)] > 0, world                                  # order 2 packs, exchanges and waits
        for key, want in one.items():
            got = np.empty_like(want)
            for mine, r in res:
                got[mine] = r[key]
            assert dm.same(got, want), (ne, world, key, int((dm.bits(got) != dm.bits(want)).sum()))


# ---- 9 ----
def test_refusals_launch_nothing():
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    ne, nlev, nf = 2, 72, 2
    h = _hip(ne)
    f, want = _case(ne, nf, nlev, 2)
    E, plane = h.nelemd, nlev * 16
    dense = [nf * plane, plane, 16, 4, 1]
    big = torch.full((2 * f.size + 64,), SENTINEL, dtype=torch.float64, device="cuda")   # room for in, and for an out that overlaps or touches it
    big[:f.size] = torch.from_numpy(np.array(f)).reshape(-1).cuda()
    buf = big[:f.size].view(f.shape)
    other = torch.full(f.shape, SENTINEL, dtype=torch.float64, device="cuda")
    keep, keep_other = big.clone(), other.clone()
    host = np.array(f)
    h.timing(True)

    def view(strides, ptr):
        return _lib.View(ptr, (C.c_longlong * 5)(*strides))
    p0 = buf.data_ptr()
    vin = view(dense, p0)
    q1, nbytes = h.device_ptr("qdp1")
    assert nbytes == E * QSIZE * plane * 8
    libview = _Fake((E, QSIZE, nlev, 4, 4), [QSIZE * plane, plane, 16, 4, 1], q1)
    h.biharmonic_view(other, "eqkji")                                         # (the staging field exists from here on)
    other.copy_(keep_other)
    h.timing(True)
    st, stbytes = h.device_ptr("view_stage")
    assert st and stbytes >= f.size * 8
    # an allocation of the field's size made with the runtime itself, and the range the runtime reports for it (it may round the size
    # up): an out view of the field's shape that ends one double beyond that range is refused
    raw = vc.RawAllocation(f.size * 8, fill=host)
    beyond, raw_now = raw.beyond, lambda: raw.read(f.shape)
    cases = [
        ("device", lambda: h.biharmonic_view(_Fake(f.shape, dense, host.ctypes.data), "eqkji")),
        ("device", lambda: h.biharmonic_view(buf, "eqkji", out=_Fake(f.shape, dense, host.ctypes.data))),
        ("outside its allocation", lambda: h.biharmonic_view(buf, "eqkji", out=_Fake(f.shape, dense, beyond))),                 # one double beyond
        ("in: .* allocation of the library", lambda: h.biharmonic_view(libview, "eqkji", out=other)),
        ("out: .* allocation of the library", lambda: h.biharmonic_view(_Fake((E, QSIZE, nlev, 4, 4), dense, p0), "eqkji", out=libview)),
        ("out: .* allocation of the library", lambda: h.biharmonic_view(buf, "eqkji", out=_Fake(f.shape, dense, st))),   # the staging field itself
        ("order=3", lambda: h.biharmonic_view(buf, "eqkji", order=3)),
        ("order=0", lambda: h.biharmonic_view(buf, "eqkji", order=0)),
        ("unknown order", lambda: h.biharmonic_view(buf, "eqkji", order="cubic")),
        ("nf = 0", lambda: h.biharmonic_view(vin, None, nf=0, nk=nlev)),
        ("nk = %d" % (nlev + 2), lambda: h.biharmonic_view(vin, None, nf=1, nk=nlev + 2)),
        (r"stride 0 on the j axis.*\(in\)", lambda: h.biharmonic_view(view([nf * plane, plane, 16, 0, 1], p0), None, out=view(dense, other.data_ptr()), nf=nf, nk=nlev)),
        (r"stride 0 on the q axis.*\(out\)", lambda: h.biharmonic_view(vin, None, out=view([nf * plane, 0, 16, 4, 1], other.data_ptr()), nf=nf, nk=nlev)),
        (r"overlap itself.*\(out\)", lambda: h.biharmonic_view(vin, None, out=view([nf * plane, plane // 2, 16, 4, 1], other.data_ptr()), nf=nf, nk=nlev)),
        ("overlaps in", lambda: h.biharmonic_view(vin, None, out=view(dense, p0 + 8 * 16), nf=nf, nk=nlev)),             # shifted by one slab
        ("overlaps in", lambda: h.biharmonic_view(vin, None, out=view(dense, p0 + 8 * (f.size - 1)), nf=nf, nk=nlev)),   # one double shared
        ("overlaps in", lambda: h.biharmonic_view(vin, None, out=view([nf * 16 * nlev, 16 * nlev, 1, 4 * nlev, nlev], p0), nf=nf, nk=nlev)),
        ("fields of", lambda: h.biharmonic_view(buf, "eqkji", out=other[:, :1])),
        ("null view pointer", lambda: h.biharmonic_view(view(dense, None), None, nf=nf, nk=nlev)),
        ("null view pointer", lambda: h.biharmonic_view(vin, None, out=view(dense, None), nf=nf, nk=nlev)),
        ("not 8-byte aligned", lambda: h.biharmonic_view(vin, None, out=view(dense, other.data_ptr() + 4), nf=nf, nk=nlev)),
    ]
    for text, call in cases:
        print("biharmonic_view refusal:", text)
        with pytest.raises(TseError, match=text):
            call()
        assert h.kernel_time("fieldlap")[1] == 0, text
        assert torch.equal(big.view(torch.int64), keep.view(torch.int64)), text
        assert torch.equal(other.view(torch.int64), keep_other.view(torch.int64)), text
    L = h.L
    assert L.tse_biharmonic_view(h.h, nf, nlev, 2, None, None, None) != 0 and b"null" in L.tse_last_error()
    assert L.tse_biharmonic_view(h.h, nf, nlev, 2, C.byref(vin), None, None) != 0 and b"null" in L.tse_last_error()
    assert h.kernel_time("fieldlap")[1] == 0
    # good calls afterwards: an out that touches in's end, then in place
    h.biharmonic_view(vin, None, out=view(dense, p0 + 8 * f.size), nf=nf, nk=nlev)
    assert h.kernel_time("fieldlap")[1] == LAUNCHES
    assert dm.same(big[f.size:2 * f.size].view(f.shape).cpu().numpy(), want) and dm.same(buf.cpu().numpy(), f)
    assert torch.equal(big[2 * f.size:], keep[2 * f.size:])
    h.biharmonic_view(buf, "eqkji")
    assert h.kernel_time("fieldlap")[1] == 2 * LAUNCHES and dm.same(buf.cpu().numpy(), want)
    assert dm.same(raw_now(), f)
    src = torch.from_numpy(np.array(f)).cuda()
    h.biharmonic_view(src, "eqkji", out=_Fake(f.shape, dense, raw.ptr))        # the out view that fits exactly is served
    assert dm.same(raw_now(), want) and dm.same(src.cpu().numpy(), f)
    h.timing(False)
    raw.free()
