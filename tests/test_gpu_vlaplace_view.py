"""-m gpu: tse_vlaplace_view -- the weak vector Laplacian (order 1) and the weak vector biharmonic (order 2) of a host's own wind on the
device through strided views, in place or into a second view.

The reference of every bit comparison is the entry itself on the dense layout, composed with the entry the library had before: order 1 in
place on [e][c][k][j][i]; for order 2 then HipMod.dss_view(mode="weak") with nf = 2 and order 1 again -- computed once per (mesh, nk,
order, nu_ratio) and shared.  What the numbers are is held by the bound against vlaplace_model's longdouble chain.
 1 bits          both orders, ne2 / ne3, nk in nlev, nlev + 1, 1, 2: `in` in every layout, `out` in place and a separate array in a layout
                 of each other path; NaN-filled gaps keep every bit, a separate `in` keeps every bit
 2 bound         under bound(28, A) / bound(60, A) against the longdouble chain, smooth and random fields, nu_ratio 1.0 and 2.5
 3 linearity     the input times 2^+-200 gives the output times the same power, bit for bit
 4 independence  a permutation of the levels permutes the output; a level alone has the bits it has among nlev
 5 swap          the components swapped: another result, under the bound of the swapped input
 6 levels        the 64- and 80-level libraries on the level-fastest path
 7 untouched     the library's fields and timer groups, the launch count, the shared staging buffer, interleaved dss_view / biharmonic_view
 8 stream        producer -> vlaplace_view -> consumer on one side stream; a stream under capture is refused
 9 ranks         2 and 3 contexts on one GPU through the callback exchange == one context, bit for bit; order 1 exchanges nothing
10 refusals      nothing launched, the arrays unchanged"""
import ctypes as C
import functools

import numpy as np
import pytest

import dss_view_model as dm
import view_common as vc
import vlaplace_model as vm
from view_common import FakeArray as _Fake, raw_field as _raw

pytestmark = pytest.mark.gpu
QSIZE = 2
LAUNCHES = 2   # per call, either order: k_vlap_view_stage and k_vlap_view_out
SENTINEL = -7.25


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
    """a context of qsize 2 on the oracle's mesh with the vector tables set up (kept for the session: contexts are small)"""
    return _make(ne, nlev)


def compose(h, f, order, nu=1.0):
    """order 1 on the dense layout; order 2: order 1, dss_view(weak), order 1 -- f[n][2][nk][4][4] -> the same shape"""
    import torch
    t = torch.from_numpy(np.array(f)).cuda()
    h.vlaplace_view(t, "eqkji", order=1, nu_ratio=nu)
    if order == 2:
        h.dss_view(t, "eqkji", mode="weak")
        h.vlaplace_view(t, "eqkji", order=1, nu_ratio=nu)
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(ne, nk, order, nlev=72, seed=0, nu=1.0):
    """(field, the composition's result), shared and read-only"""
    h = _hip(ne, nlev)
    f = vm.random_field(h.nelemd, nk, seed)
    want = compose(h, f, order, nu)
    f.setflags(write=False); want.setflags(write=False)
    return f, want


def _run(h, f, name, order, out_name=None, stream=None, nu=1.0):
    """vlaplace_view of a host array through a layout, in place (out_name None) or into a second array -> the result; every gap keeps
    its bits, and with a separate out the whole of `in` does"""
    import torch
    S = dm.Strided(f, name)
    buf = torch.from_numpy(S.host.copy()).cuda()
    vin = _Fake(S.shape, S.s, buf.data_ptr() + 8 * S.base)
    if out_name is None:
        h.vlaplace_view(vin, "eqkji", order=order, nu_ratio=nu, stream=stream)
        T, res = S, buf
    else:
        T = dm.Strided(np.full(f.shape, SENTINEL), out_name)
        res = torch.from_numpy(T.host.copy()).cuda()
        h.vlaplace_view(vin, "eqkji", out=_Fake(T.shape, T.s, res.data_ptr() + 8 * T.base), order=order, nu_ratio=nu, stream=stream)
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


@pytest.mark.parametrize("order", vm.ORDERS)
@pytest.mark.parametrize("ne", [2, 3])
def test_bits_of_the_composition(ne, order):
    from transport_se_amd.hip_mod import vlaplace_view_plan
    h, nlev = _hip(ne), 72
    pairs = set()
    for nk in (nlev, nlev + 1, 1, 2):
        nu = 2.5 if nk == 2 else 1.0
        f, want = _case(ne, nk, order, nu=nu)
        assert not dm.same(f, want) and np.isfinite(want).all()
        for i, name in enumerate(dm.LAYOUTS):
            pin = dm.expected_path(name, nk, nlev)
            outs = [None] + [r for r in OUT_REPS if dm.expected_path(r, nk, nlev) != pin] + [OUT_ODD[i % 2]]
            for out_name in outs:
                pout = pin if out_name is None else dm.expected_path(out_name, nk, nlev)
                plan = vlaplace_view_plan(h.nelemd, nk, dm.layout(name, h.nelemd, 2, nk)[0],
                                          None if out_name is None else dm.layout(out_name, h.nelemd, 2, nk)[0])
                assert [p["path"] for p in plan] == [pin, pout], (name, out_name, plan)
                pairs.add((pin, pout))
                got = _run(h, f, name, order, out_name, nu=nu)
                assert dm.same(got, want), (ne, order, nk, name, out_name, int((dm.bits(got) != dm.bits(want)).sum()))
    assert pairs == {(a, b) for a in range(3) for b in range(3)}, pairs
    if order == 2:
        assert not dm.same(_case(ne, nlev, 1)[1], _case(ne, nlev, 2)[1])


def test_a_wind_without_its_level_axis_and_in_other_axes():
    """a missing k letter: extent 1 and stride 0; E3SM's state%v order [e][k][c][j][i]; out in other axes than in"""
    import torch
    ne, nlev = 2, 72
    h = _hip(ne)
    f, want = _case(ne, 1, 2)
    sfc = torch.from_numpy(np.array(f[:, :, 0])).cuda()                       # [e][c][j][i]
    h.vlaplace_view(sfc, "eqji")
    assert dm.same(sfc.cpu().numpy(), want[:, :, 0])
    f, want = _case(ne, nlev, 2)
    v = torch.from_numpy(np.ascontiguousarray(np.swapaxes(f, 1, 2))).cuda()   # [e][k][c][j][i]: component stride 16, level stride 32
    out = torch.full((h.nelemd, 2, 4, 4, nlev), SENTINEL, dtype=torch.float64, device="cuda")   # [e][c][j][i][k]
    h.vlaplace_view(v, "ekqji", out=out, out_axes="eqjik", order="vbiharmonic")
    assert dm.same(np.ascontiguousarray(np.moveaxis(out.cpu().numpy(), -1, 2)), want)
    h.vlaplace_view(v, "ekqji", order="vlaplace")
    assert dm.same(np.ascontiguousarray(np.swapaxes(v.cpu().numpy(), 1, 2)), _case(ne, nlev, 1)[1])


# ---- 2 ----
@pytest.mark.parametrize("ne", [2, 3])
def test_pointwise_bound(ne):
    """|device - longdouble chain| <= bound(28, A) (order 1), bound(60, A) (order 2) at every point.  Measured on the MI355X, worst
    error / bound over both meshes and both ratios: order 1 0.089 (random) and 0.028 (smooth), order 2 0.012 and 0.003; the fp64
    restatement of the reference reaches 0.067 (order 1) and 0.010 (order 2) in test_vlaplace_cpu.py."""
    import elem_ops_ld as ld
    assert ld.has_extended_precision(), np.finfo(np.longdouble)
    h, o = _hip(ne), _oracle(ne)
    D, mi, mp = _host(ne)
    nk = 3
    for kind, f in (("random", vm.random_field(o.nelem, nk, seed=3)), ("smooth", vm.smooth_field(o, nk))):
        for nu in (1.0, 2.5):
            for order in vm.ORDERS:
                ref, A = vm.longdouble(o, D, mi, mp, f, order, nu)
                for name in ("dense", "ij"):
                    got = _run(h, f, name, order, nu=nu)
                    worst = float(vm.ratio(got, ref, A, order).max())
                    print("vlaplace_view ne%d order %d nu_ratio %.1f %s %s: worst error / bound = %.3f" % (ne, order, nu, kind, name, worst))
                    assert worst < 1.0, (ne, order, nu, kind, name, worst)


# ---- 3 ----
@pytest.mark.parametrize("order", vm.ORDERS)
def test_linearity_in_powers_of_two(order):
    """values of order 30 times 2^+-200: the second Laplacian's results are of order 1e-22 times that, far from both ends of the range"""
    ne, nk = 2, 5
    h = _hip(ne)
    f = vm.random_field(h.nelemd, nk, seed=5)
    for name, out_name in (("dense", None), ("lev_even", "ij")):
        base = _run(h, f, name, order, out_name, nu=2.5)
        assert np.isfinite(base).all() and (np.abs(base) > 1e-200).all()
        for p in (200, -200):
            got = _run(h, np.ldexp(f, p), name, order, out_name, nu=2.5)
            assert dm.same(got, np.ldexp(base, p)), (order, name, p)
            assert np.isfinite(got).all() and (np.abs(got) > 2.0 ** -900).all()


# ---- 4 ----
@pytest.mark.parametrize("order", vm.ORDERS)
def test_levels_are_independent(order):
    ne, nlev = 3, 72
    h = _hip(ne)
    nk = nlev
    f = np.array(_case(ne, nk, order)[0])
    perm = np.random.default_rng(11).permutation(nk)
    assert (perm != np.arange(nk)).any()
    fp = np.ascontiguousarray(f[:, :, perm])
    for name, out_name in (("dense", None), ("lev0", None), ("ij", "dense")):
        base = _run(h, f, name, order, out_name)
        assert dm.same(base, _case(ne, nk, order)[1])
        got = _run(h, fp, name, order, out_name)
        assert dm.same(got, base[:, :, perm]), (order, name)
        for k in (0, 37, nlev - 1):                                            # a level alone: nk = 1
            one = _run(h, np.ascontiguousarray(f[:, :, k:k + 1]), name, order, out_name)
            assert dm.same(one[:, :, 0], base[:, :, k]), (order, name, k)


# ---- 5 ----
@pytest.mark.parametrize("order", vm.ORDERS)
def test_swapped_components_give_another_bounded_result(order):
    """a kernel that read one component twice, or wrote them crossed, would pass every comparison of the entry with itself"""
    ne, nk = 2, 3
    h, o = _hip(ne), _oracle(ne)
    D, mi, mp = _host(ne)
    f = vm.random_field(o.nelem, nk, seed=9)
    sw = np.ascontiguousarray(f[:, ::-1])
    a, b = _run(h, f, "dense", order), _run(h, sw, "dense", order)
    assert not dm.same(a, b) and not dm.same(a, np.ascontiguousarray(b[:, ::-1]))
    for x, got in ((f, a), (sw, b)):
        ref, A = vm.longdouble(o, D, mi, mp, x, order)
        assert float(vm.ratio(got, ref, A, order).max()) < 1.0
    one = f.copy(); one[:, 1] = 0.0                                            # each component alone reaches both outputs
    r = _run(h, one, "dense", 1)
    assert (np.abs(r[:, 0]) > 0).any() and (np.abs(r[:, 1]) > 0).any()


# ---- 6 ----
@pytest.mark.parametrize("nlev", [64, 80])
def test_other_level_counts(nlev):
    from transport_se_amd.hip_mod import vlaplace_view_plan
    ne = 2
    h = _hip(ne, nlev)
    for order in vm.ORDERS:
        f, want = _case(ne, nlev, order, nlev)
        for name, out_name in (("lev0", None), ("lev_odd", None), ("lev_odd8", "dense"), ("epad", "lev_even")):
            plan = vlaplace_view_plan(h.nelemd, nlev, dm.layout(name, h.nelemd, 2, nlev)[0],
                                      None if out_name is None else dm.layout(out_name, h.nelemd, 2, nlev)[0], nlev=nlev)
            assert 1 in [p["path"] for p in plan], plan
            assert dm.same(_run(h, f, name, order, out_name), want), (nlev, order, name, out_name)
    # the numbers, not only their agreement: the bound on the level-fastest path of this library
    o = _oracle(ne)
    D, mi, mp = _host(ne)
    f, _ = _case(ne, nlev, 2, nlev)
    ref, A = vm.longdouble(o, D, mi, mp, f[:, :, :2], 2)
    assert float(vm.ratio(_run(h, f, "lev0", 2)[:, :, :2], ref, A, 2).max()) < 1.0


# ---- 7 ----
LIB_FIELDS = ("qdp1", "qdp2", "dp", "q", "divdp", "divdp_proj", "dp3d", "ps_v", "qmin", "qmax")
GROUPS = ("dss", "lap", "view", "level", "fielddss", "fieldlap", "fieldremap", "remap", "advance", "minmax", "forcing", "stateq")


def test_the_library_is_untouched():
    import torch
    import biharmonic_model as bm
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
        assert h.kernel_time("fieldvlap") == (0.0, 0)
        calls, stage = 0, []
        # layers per call: 144, 144, 4 (smaller: reused), 144, then 146 (grows once), 146, 144
        for nk, name, out_name, order in ((nlev, "lev0", None, 2), (nlev, "dense", "ij", 1), (2, "ij", None, 2), (nlev, "epad", "lev_even", 2),
                                          (nlev + 1, "dense", None, 2), (nlev + 1, "lev_even", "dense", 1), (nlev, "lev0", None, 1)):
            nu = 2.5 if nk == 2 else 1.0
            f, want = _case(ne, nk, order, nu=nu)
            assert dm.same(_run(h, f, name, order, out_name, nu=nu), want), (nk, name, out_name, order)
            calls += 1
            assert h.kernel_time("fieldvlap")[1] == LAUNCHES * calls
            stage.append(h.device_ptr("view_stage"))
        assert h.kernel_time("fieldvlap")[0] > 0.0
        assert stage[0] == stage[1] == stage[2] == stage[3] and stage[0][1] == h.nelemd * 144 * 128
        assert stage[4] == stage[5] == stage[6] and stage[4][1] == h.nelemd * 146 * 128
        for g in GROUPS:
            assert h.kernel_time(g)[1] == 0, g
        # an interleaved dss_view and biharmonic_view of other layer counts still give their own bits, and the next vlaplace its own
        w = dm.field(h.nelemd, 3, 7)
        t = torch.from_numpy(w.copy()).cuda()
        h.dss_view(t, "eqkji", mode="average")
        assert dm.same(t.cpu().numpy(), dm.model(o, w, "average"))
        s = bm.random_field(h.nelemd, 1, 5)
        ts = torch.from_numpy(s.copy()).cuda()
        h.biharmonic_view(ts, "eqkji", order=1)
        lap = np.stack([h.laplace_sphere_wk(np.ascontiguousarray(s[:, 0, l])) for l in range(5)], axis=1)
        assert dm.same(ts.cpu().numpy()[:, 0], lap)
        f, want = _case(ne, nlev + 1, 2)
        assert dm.same(_run(h, f, "dense", 2), want)
        assert h.device_ptr("view_stage") == stage[4] and h.kernel_time("fielddss")[1] == 2 and h.kernel_time("fieldlap")[1] == 2
        assert h.kernel_time("fieldvlap")[1] == LAUNCHES * (calls + 1)
        h.timing(False)
        for k in LIB_FIELDS:
            assert dm.same(_raw(h, k), before[k]), k
        # a second vector_setup with the same fields leaves the same bits
        h.vector_setup(*_host(ne))
        assert dm.same(_run(h, f, "dense", 2), want)
        for x in (h, twin):                                                      # the cached bounds survive: the next step is the twin's
            x.dcmip_step_inputs(1, dt); x.advec_tracers_remap_rk2(dt, 2, 1)
        shape = (h.nelemd, QSIZE, nlev, 4, 4)
        assert dm.same(h.fetch("qdp1", shape), twin.fetch("qdp1", shape))
        assert all(dm.same(a, b) for a, b in zip(h.get_qminmax(), twin.get_qminmax()))
    finally:
        h.close(); twin.close()


# ---- 8 ----
def test_stream_order_and_capture():
    import torch
    from transport_se_amd.hip_mod import TseError
    ne, nlev = 3, 72
    h = _hip(ne)
    f, _ = _case(ne, nlev, 2)
    lf = np.ascontiguousarray(np.moveaxis(f.reshape(f.shape[:3] + (16,)), 2, -1)).reshape(f.shape[0], 2, 4, 4, nlev)   # [e][c][j][i][k]
    x = (lf - 1.0) / 2.0
    made = x * 2.0 + 1.0                                                       # what the device will hold: the host knows its bits
    ref = torch.from_numpy(made.copy()).cuda()
    h.vlaplace_view(ref, "eqjik")                                              # stream=None: complete on return
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
            h.vlaplace_view(field, "eqjik", out=res if separate else None, stream=s)
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
            h.vlaplace_view(ref, "eqjik", stream=s)
    assert h.kernel_time("fieldvlap")[1] == 0
    h.timing(False)
    assert torch.equal(ref.view(torch.int64), keep.view(torch.int64))


# ---- 9 ----
RANK_CASES = ((72, "dense"), (73, "lev_odd"), (72, "lev0"), (1, "dense"))


def _rank_body(ne):
    from transport_se_amd import cube_mesh as cm
    nelem = 6 * ne * ne

    def body(rank, h, mine, geo, hv):
        out = {}
        h.vector_setup(geo["D"][mine], cm.metinv(geo["D"])[mine], geo["mp"][mine])
        h.comm_timing(True)
        for order in vm.ORDERS:
            for nk, name in RANK_CASES:
                f = vm.random_field(nelem, nk, seed=7)[mine]
                out[(nk, name, order)] = _run(h, f, name, order, nu=2.5)
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


# ---- 10 ----
def test_refusals_launch_nothing():
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    ne, nlev = 2, 72
    h = _hip(ne)
    f, want = _case(ne, nlev, 2)
    E, plane = h.nelemd, nlev * 16
    dense = [2 * plane, plane, 16, 4, 1]
    big = torch.full((2 * f.size + 64,), SENTINEL, dtype=torch.float64, device="cuda")   # room for in, and for an out that overlaps or touches it
    big[:f.size] = torch.from_numpy(np.array(f)).reshape(-1).cuda()
    buf = big[:f.size].view(f.shape)
    other = torch.full(f.shape, SENTINEL, dtype=torch.float64, device="cuda")
    keep, keep_other = big.clone(), other.clone()
    host = np.array(f)

    def view(strides, ptr):
        return _lib.View(ptr, (C.c_longlong * 5)(*strides))
    p0 = buf.data_ptr()
    vin = view(dense, p0)
    # before vector_setup: a context of its own
    bare = _make(ne, setup=False)
    try:
        bare.timing(True)
        with pytest.raises(TseError, match="tse_vector_setup first"):
            bare.vlaplace_view(buf, "eqkji")
        with pytest.raises(TseError, match="vector_setup: D"):
            bare.vector_setup(_host(ne)[0][:1], _host(ne)[1], _host(ne)[2])
        assert bare.kernel_time("fieldvlap")[1] == 0 and bare.device_ptr("view_stage") == (None, 0)
        assert torch.equal(big.view(torch.int64), keep.view(torch.int64))
        bare.vector_setup(*_host(ne))                                          # ... and after it the call is served
        bare.vlaplace_view(buf, "eqkji", out=other)
        assert dm.same(other.cpu().numpy(), want) and bare.kernel_time("fieldvlap")[1] == LAUNCHES
        other.copy_(keep_other)
    finally:
        bare.close()
    q1, nbytes = h.device_ptr("qdp1")
    assert nbytes == E * QSIZE * plane * 8
    libview = _Fake((E, QSIZE, nlev, 4, 4), [QSIZE * plane, plane, 16, 4, 1], q1)
    h.vlaplace_view(other, "eqkji")                                            # (the staging field exists from here on)
    other.copy_(keep_other)
    h.timing(True)
    st, stbytes = h.device_ptr("view_stage")
    assert st and stbytes >= f.size * 8
    cases = [
        ("device", lambda: h.vlaplace_view(_Fake(f.shape, dense, host.ctypes.data), "eqkji")),
        ("device", lambda: h.vlaplace_view(buf, "eqkji", out=_Fake(f.shape, dense, host.ctypes.data))),
        ("in: .* allocation of the library", lambda: h.vlaplace_view(libview, "eqkji", out=other)),
        ("out: .* allocation of the library", lambda: h.vlaplace_view(_Fake((E, QSIZE, nlev, 4, 4), dense, p0), "eqkji", out=libview)),
        ("out: .* allocation of the library", lambda: h.vlaplace_view(buf, "eqkji", out=_Fake(f.shape, dense, st))),   # the staging field itself
        ("order=3", lambda: h.vlaplace_view(buf, "eqkji", order=3)),
        ("order=0", lambda: h.vlaplace_view(buf, "eqkji", order=0)),
        ("unknown order", lambda: h.vlaplace_view(buf, "eqkji", order="biharmonic")),
        ("nu_ratio = nan", lambda: h.vlaplace_view(buf, "eqkji", nu_ratio=float("nan"))),
        ("nu_ratio = inf", lambda: h.vlaplace_view(buf, "eqkji", nu_ratio=float("inf"))),
        ("nu_ratio = -inf", lambda: h.vlaplace_view(buf, "eqkji", order=1, nu_ratio=float("-inf"))),
        ("nk = 0", lambda: h.vlaplace_view(vin, None, nk=0)),
        ("nk = %d" % (nlev + 2), lambda: h.vlaplace_view(vin, None, nk=nlev + 2)),
        ("extent 3, not 2", lambda: h.vlaplace_view(torch.zeros((E, 3, 2, 4, 4), dtype=torch.float64, device="cuda"), "eqkji")),
        ("extent 1, not 2", lambda: h.vlaplace_view(buf[:, 0], "ekji")),
        ("components of", lambda: h.vlaplace_view(buf, "eqkji", out=other[:, :1])),
        ("components of", lambda: h.vlaplace_view(buf, "eqkji", out=other[:, :, :5])),
        (r"stride 0 on the j axis.*\(in\)", lambda: h.vlaplace_view(view([2 * plane, plane, 16, 0, 1], p0), None, out=view(dense, other.data_ptr()), nk=nlev)),
        (r"stride 0 on the q axis.*\(out\)", lambda: h.vlaplace_view(vin, None, out=view([2 * plane, 0, 16, 4, 1], other.data_ptr()), nk=nlev)),
        (r"overlap itself.*\(out\)", lambda: h.vlaplace_view(vin, None, out=view([2 * plane, plane // 2, 16, 4, 1], other.data_ptr()), nk=nlev)),
        ("overlaps in", lambda: h.vlaplace_view(vin, None, out=view(dense, p0 + 8 * 16), nk=nlev)),             # shifted by one slab
        ("overlaps in", lambda: h.vlaplace_view(vin, None, out=view(dense, p0 + 8 * (f.size - 1)), nk=nlev)),   # one double shared
        ("overlaps in", lambda: h.vlaplace_view(vin, None, out=view([2 * 16 * nlev, 16 * nlev, 1, 4 * nlev, nlev], p0), nk=nlev)),
        ("null view pointer", lambda: h.vlaplace_view(view(dense, None), None, nk=nlev)),
        ("null view pointer", lambda: h.vlaplace_view(vin, None, out=view(dense, None), nk=nlev)),
        ("not 8-byte aligned", lambda: h.vlaplace_view(vin, None, out=view(dense, other.data_ptr() + 4), nk=nlev)),
    ]
    for text, call in cases:
        print("vlaplace_view refusal:", text)
        with pytest.raises(TseError, match=text):
            call()
        assert h.kernel_time("fieldvlap")[1] == 0, text
        assert torch.equal(big.view(torch.int64), keep.view(torch.int64)), text
        assert torch.equal(other.view(torch.int64), keep_other.view(torch.int64)), text
    L = h.L
    assert L.tse_vlaplace_view(h.h, nlev, 2, 1.0, None, None, None) != 0 and b"null" in L.tse_last_error()
    assert L.tse_vlaplace_view(h.h, nlev, 2, 1.0, C.byref(vin), None, None) != 0 and b"null" in L.tse_last_error()
    assert L.tse_vector_setup(h.h, None, 0, None, 0, None, 0) != 0 and b"null argument" in L.tse_last_error()
    assert h.kernel_time("fieldvlap")[1] == 0
    # good calls afterwards: an out that touches in's end, then in place
    h.vlaplace_view(vin, None, out=view(dense, p0 + 8 * f.size), nk=nlev)
    assert h.kernel_time("fieldvlap")[1] == LAUNCHES
    assert dm.same(big[f.size:2 * f.size].view(f.shape).cpu().numpy(), want) and dm.same(buf.cpu().numpy(), f)
    assert torch.equal(big[2 * f.size:], keep[2 * f.size:])
    h.vlaplace_view(buf, "eqkji")
    assert h.kernel_time("fieldvlap")[1] == 2 * LAUNCHES and dm.same(buf.cpu().numpy(), want)
    h.timing(False)
