"""-m gpu: tse_sphere_op_view -- gradient_sphere, divergence_sphere and vorticity_sphere of a host's own fields on the device through
strided views, element-local or C0 (rspheremp * DSS(spheremp * op)), `in` and `out` each in a layout of its own.

The reference of every bit comparison is the entry itself on the dense layout, LOCAL, composed for C0 with the entry the library had
before: HipMod.dss_view(mode="average") on the output array -- computed once per (nlev, nk, op, c0) and shared.  What the numbers are is
held by the bound against sphere_ops_model's longdouble chain, and for the divergence by tse_divergence_sphere.
 1 bits          the three ops, both modes, nk in 1, 3, nlev, nlev + 1: all nine path pairs, wide and narrow accesses on either side, an
                 odd row pitch, j and i swapped, the state%v order; NaN-filled gaps of `out` and the whole of `in` keep every bit
 2 levels        a level alone has the bits it has among nlev
 3 divergence    LOCAL divergence is tse_divergence_sphere slab for slab, bit for bit
 4 bound         under bound(N, A), N = 7 / 13 / 12 (+ 5 for C0), against the longdouble chain, random and smooth fields
 5 level counts  the 64- and 80-level libraries on every path
 6 untouched     the library's fields and timer groups, the launch count, the shared staging buffer and its growth
 7 stream        producer -> sphere_op_view -> consumer on one side stream; a stream under capture is refused
 8 ranks         2 and 3 contexts on one GPU through the callback exchange == one context, bit for bit; LOCAL exchanges nothing
 9 refusals      nothing launched, the arrays unchanged
The Fortran routine sphere_op_view_hip is called by tests/fortran_resident/views_harness.F90 (test_gpu_fortran_views.py); what the
numbers are against the reference's own Fortran is held by test_gpu_reference_fieldops.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import dss_view_model as dm
import sphere_ops_model as sm
import view_common as vc
from view_common import FakeArray as _Fake, raw_field as _raw

pytestmark = pytest.mark.gpu
QSIZE = 2
NE = 2
LAUNCHES = 2   # per call, either mode: k_sphere_op_stage, then k_dss_view_sum (C0) or k_lap_view_out<., ., 1> (LOCAL)
SENTINEL = -7.25
MODES = (False, True)


def layout(name, E, nf, nk):
    """dss_view_model's layouts and three more: rows of levels at the odd pitch nk + 3 (nk even), j and i swapped, and E3SM's
    state%v(np,np,2,nlev,tl) order (one time level of three; a scalar has no such order and is dense)"""
    if name == "lev_p3":
        S = nk + 3
        return [nf * 16 * S, 16 * S, 1, 4 * S, S], 0, E * nf * 16 * S
    if name == "ji":
        return [nf * nk * 16, nk * 16, 16, 1, 4], 0, E * nf * nk * 16
    if name == "statev" and nf == 2:
        return [96 * nk, 16, 32, 4, 1], 0, E * 96 * nk
    return dm.layout("dense" if name == "statev" else name, E, nf, nk)


def expected_path(name, nk, nlev):
    if name == "lev_p3":
        return 1 if nk == nlev else 2
    if name == "ji":
        return 2
    return dm.expected_path("dense" if name == "statev" else name, nk, nlev)


class Strided(dm.Strided):
    def __init__(self, data, name):
        data = np.asarray(data, dtype=np.float64)
        E, nf, nk = data.shape[:3]
        self.s, self.base, size = layout(name, E, nf, nk)
        self.ix = dm.index(self.s, self.base, data.shape)
        assert np.unique(self.ix).size == self.ix.size and self.ix.min() >= 0 and self.ix.max() < size, name
        self.host = (np.uint64(dm.PAYLOAD) + np.arange(size, dtype=np.uint64)).view(np.float64)
        self.host[self.ix] = data
        self.shape, self.name = data.shape, name
        self.gap = np.ones(size, dtype=bool); self.gap[self.ix.ravel()] = False


@functools.lru_cache(maxsize=None)
def _oracle(ne=NE):
    return vc.oracle(ne, QSIZE)


@functools.lru_cache(maxsize=None)
def _host(ne=NE):
    import vlaplace_model as vm
    return vm.host_fields(_oracle(ne))


def _make(nlev=72, setup=True, ne=NE):
    return vc.make_hip(_oracle(ne), QSIZE, nlev, setup=_host(ne) if setup else None)


@functools.lru_cache(maxsize=None)
def _hip(nlev=72):
    """a context on the ne2 mesh with the vector tables set up (kept for the session: contexts are small)"""
    return _make(nlev)


def _out_shape(f, op):
    return (f.shape[0], sm.NF[op][1]) + f.shape[2:]


def compose(h, f, op, c0):
    """LOCAL on the dense layout; C0: then dss_view(average) on the output array"""
    import torch
    t = torch.from_numpy(np.array(f)).cuda()
    out = torch.full(_out_shape(f, op), SENTINEL, dtype=torch.float64, device="cuda")
    h.sphere_op_view(t, "eqkji", out, op=op, c0=False)
    if c0:
        h.dss_view(out, "eqkji", mode="average")
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(nk, op, c0, nlev=72, seed=0):
    """(field, the composition's result), shared and read-only"""
    h = _hip(nlev)
    f = sm.random_field(h.nelemd, sm.NF[op][0], nk, seed)
    want = compose(h, f, op, c0)
    assert np.isfinite(want).all() and not (want == SENTINEL).any()
    f.setflags(write=False); want.setflags(write=False)
    return f, want


def _run(h, f, op, c0, name, out_name, stream=None):
    """sphere_op_view of a host array through a layout into a second array in another -> the result; every gap of out and the whole of
    `in` keep their bits"""
    import torch
    S = Strided(f, name)
    buf = torch.from_numpy(S.host.copy()).cuda()
    T = Strided(np.full(_out_shape(f, op), SENTINEL), out_name)
    res = torch.from_numpy(T.host.copy()).cuda()
    h.sphere_op_view(_Fake(S.shape, S.s, buf.data_ptr() + 8 * S.base), "eqkji", _Fake(T.shape, T.s, res.data_ptr() + 8 * T.base), op=op, c0=c0, stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    got, gaps = T.read(res.cpu().numpy())
    assert gaps, "bytes outside the out view changed (%s -> %s)" % (name, out_name)
    assert np.array_equal(dm.bits(buf.cpu().numpy()), dm.bits(S.host)), "in changed (%s -> %s)" % (name, out_name)
    return got


# ---- 1 ----
REPS = ("dense", "lev_even", "ij")                                     # a wide layout of paths 0 and 1, and the generic path
EXTRA = (("dense_odd8", "lev_odd8"), ("lev_odd8", "dense_odd8"), ("lev_p3", "epad"), ("epad", "lev_p3"), ("ji", "statev"), ("statev", "ji"),
         ("lev0", "lev_odd"), ("lev_odd", "lev0"))                     # narrow accesses, odd pitches, j/i swapped, the state%v order


@pytest.mark.parametrize("op", sm.OPS)
def test_bits_on_every_pair_of_paths(op):
    from transport_se_amd.hip_mod import sphere_op_view_plan
    h, nlev = _hip(), 72
    nfi, nfo = sm.NF[op]
    for nk in (nlev, nlev + 1, 1, 3):
        pairs = set()
        both = [(a, b) for a in REPS for b in REPS] + list(EXTRA)
        for c0 in MODES:
            f, want = _case(nk, op, c0)
            for name, out_name in (both if nk == nlev else both[::3]):
                plan = sphere_op_view_plan(h.nelemd, nk, op, layout(name, h.nelemd, nfi, nk)[0], layout(out_name, h.nelemd, nfo, nk)[0])
                assert [p["path"] for p in plan] == [expected_path(name, nk, nlev), expected_path(out_name, nk, nlev)], (name, out_name, plan)
                pairs.add((plan[0]["path"], plan[1]["path"]))
                got = _run(h, f, op, c0, name, out_name)
                assert dm.same(got, want), (op, c0, nk, name, out_name, int((dm.bits(got) != dm.bits(want)).sum()))
        if nk == nlev:
            assert pairs == {(a, b) for a in range(3) for b in range(3)}, pairs
    assert not dm.same(_case(nlev, op, False)[1], _case(nlev, op, True)[1])


def test_fields_without_a_level_or_component_axis_and_in_the_state_order():
    """grad(ps): a surface scalar [e][j][i] with neither q nor k; zeta = C0 vorticity of state%v [e][k][c][j][i] into [e][j][i][k]"""
    import torch
    h, nlev = _hip(), 72
    f, want = _case(1, "gradient", True)
    ps = torch.from_numpy(np.array(f[:, 0, 0])).cuda()                                  # [e][j][i]
    grad = torch.full((h.nelemd, 2, 4, 4), SENTINEL, dtype=torch.float64, device="cuda")
    h.sphere_op_view(ps, "eji", grad, "eqji", op="gradient", c0=True)
    assert dm.same(grad.cpu().numpy(), want[:, :, 0])
    for op in ("vorticity", "divergence"):
        f, want = _case(nlev, op, True)
        v = torch.from_numpy(np.ascontiguousarray(np.swapaxes(f, 1, 2))).cuda()         # [e][k][c][j][i]: component stride 16, level stride 32
        out = torch.full((h.nelemd, 4, 4, nlev), SENTINEL, dtype=torch.float64, device="cuda")
        h.sphere_op_view(v, "ekqji", out, "ejik", op=op, c0=True)
        assert dm.same(np.ascontiguousarray(np.moveaxis(out.cpu().numpy(), -1, 1)), want[:, 0])


# ---- 2 ----
@pytest.mark.parametrize("op", sm.OPS)
def test_a_level_alone_has_the_bits_it_has_among_others(op):
    h, nlev = _hip(), 72
    for c0 in MODES:
        f, want = _case(nlev, op, c0)
        for name, out_name in (("dense", "dense"), ("ij", "lev0"), ("lev_even", "ij")):
            for k in (0, 37, nlev - 1):
                one = _run(h, np.ascontiguousarray(f[:, :, k:k + 1]), op, c0, name, out_name)
                assert dm.same(one[:, :, 0], want[:, :, k]), (op, c0, name, k)
            few = _run(h, np.ascontiguousarray(f[:, :, 5:8]), op, c0, name, out_name)
            assert dm.same(few, want[:, :, 5:8]), (op, c0, name)


# ---- 3 ----
@pytest.mark.parametrize("nlev", [72, 64, 80])
def test_local_divergence_is_tse_divergence_sphere(nlev):
    h = _hip(nlev)
    f, want = _case(nlev, "divergence", False, nlev)
    for k in (0, 1, nlev // 2, nlev - 1):
        slab = h.divergence_sphere(np.ascontiguousarray(f[:, :, k]))
        assert dm.same(np.asarray(slab).reshape(h.nelemd, 4, 4), want[:, 0, k]), (nlev, k)
    f3, want3 = _case(3, "divergence", False, nlev)
    for k in range(3):
        assert dm.same(np.asarray(h.divergence_sphere(np.ascontiguousarray(f3[:, :, k]))).reshape(h.nelemd, 4, 4), want3[:, 0, k]), (nlev, k)


# ---- 4 ----
@pytest.mark.parametrize("op", sm.OPS)
def test_pointwise_bound(op):
    """|device - longdouble chain| <= bound(N, A) at every point, N = 7 (gradient), 13 (divergence), 12 (vorticity), + 5 for C0.
    Measured on the MI355X, worst error / bound over the random, the smooth and the nodal field (LOCAL, C0): gradient 0.439, 0.235;
    divergence 0.193, 0.120; vorticity 0.162, 0.112.  Nothing tighter than the derived bound is asserted."""
    import elem_ops_ld as ld
    assert ld.has_extended_precision(), np.finfo(np.longdouble)
    h, o = _hip(), _oracle()
    D = _host()[0]
    nk, nfi = 3, sm.NF[op][0]
    for kind, f in (("random", sm.random_field(o.nelem, nfi, nk, seed=3)), ("smooth", sm.smooth_field(o, nfi, nk)), ("nodal", sm.node_field(o, nfi, nk))):
        for c0 in MODES:
            ref, A = sm.longdouble(o, D, op, f, c0)
            for name, out_name in (("dense", "ij"), ("ij", "dense")):
                got = _run(h, f, op, c0, name, out_name)
                worst = float(sm.ratio(got, ref, A, op, c0).max())
                print("sphere_op_view %s c0=%d %s %s->%s: worst error / bound = %.3f" % (op, c0, kind, name, out_name, worst))
                assert worst < 1.0, (op, c0, kind, name, worst)


def test_swapped_components_give_another_bounded_result():
    """a kernel that read one component twice, or wrote the gradient's crossed, would pass every comparison of the entry with itself"""
    h, o = _hip(), _oracle()
    D = _host()[0]
    f = sm.random_field(o.nelem, 2, 3, seed=9)
    sw = np.ascontiguousarray(f[:, ::-1])
    for op in ("divergence", "vorticity"):
        a, b = _run(h, f, op, False, "dense", "dense"), _run(h, sw, op, False, "dense", "dense")
        assert not dm.same(a, b)
        ref, A = sm.longdouble(o, D, op, sw)
        assert float(sm.ratio(b, ref, A, op).max()) < 1.0


# ---- 5 ----
@pytest.mark.parametrize("nlev", [64, 80])
def test_other_level_counts(nlev):
    from transport_se_amd.hip_mod import sphere_op_view_plan
    h, o = _hip(nlev), _oracle()
    D = _host()[0]
    for op in sm.OPS:
        nfi, nfo = sm.NF[op]
        for c0 in MODES:
            for nk in (nlev, nlev + 1, 1, 3):
                f, want = _case(nk, op, c0, nlev)
                for name, out_name in ((("lev0", "lev_p3"), ("lev_odd8", "dense"), ("epad", "lev_even"), ("ij", "lev0")) if nk == nlev else (("lev_even", "dense"), ("dense", "ij"))):
                    plan = sphere_op_view_plan(h.nelemd, nk, op, layout(name, h.nelemd, nfi, nk)[0], layout(out_name, h.nelemd, nfo, nk)[0], nlev=nlev)
                    assert [p["path"] for p in plan] == [expected_path(name, nk, nlev), expected_path(out_name, nk, nlev)], plan
                    assert dm.same(_run(h, f, op, c0, name, out_name), want), (nlev, op, c0, nk, name, out_name)
        # the numbers, not only their agreement: the bound on the level-fastest path of this library
        f, _ = _case(nlev, op, True, nlev)
        ref, A = sm.longdouble(o, D, op, f[:, :, :2], True)
        assert float(sm.ratio(_run(h, f, op, True, "lev0", "lev0")[:, :, :2], ref, A, op, True).max()) < 1.0


# ---- 6 ----
GROUPS = ("dss", "lap", "view", "level", "fielddss", "fieldlap", "fieldvlap", "fieldremap", "remap", "advance", "minmax", "forcing", "stateq")


def test_the_library_is_untouched():
    import call_sequences as cs
    nlev, dt = 72, 1800.0
    o = _oracle()
    h, twin = _make(), _make()
    try:
        for x in (h, twin):
            x.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm)
            x.dcmip_set_initial()
            x.dcmip_step_inputs(0, dt); x.advec_tracers_remap_rk2(dt, 1, 2)      # leaves the element bounds of Qdp(2) cached
            x.state_q(2)                                                          # "q" and "lnps" exist and are fresh
        names = [k for k in cs.FIELDS + ("q", "lnps") if h.device_ptr(k)[0]]
        assert set(cs.FIELDS) <= set(names)
        before = {k: _raw(h, k) for k in names}
        assert h.device_ptr("view_stage") == (None, 0)
        h.timing(True)
        assert h.kernel_time("fieldop") == (0.0, 0)
        calls, stage = 0, []
        # layers per call (nf_out * nk): 72, 72, 144 (grows), 3 (smaller: reused), 144, 146 (grows), 73, 146
        for nk, op, c0, name, out_name in ((nlev, "vorticity", True, "lev0", "dense"), (nlev, "divergence", False, "dense", "ij"),
                                           (nlev, "gradient", True, "epad", "lev_even"), (3, "vorticity", True, "ij", "dense"),
                                           (nlev, "gradient", False, "lev_even", "dense"), (nlev + 1, "gradient", True, "dense", "dense"),
                                           (nlev + 1, "divergence", True, "lev_even", "dense"), (nlev + 1, "gradient", False, "ij", "epad")):
            f, want = _case(nk, op, c0)
            assert dm.same(_run(h, f, op, c0, name, out_name), want), (nk, op, c0, name, out_name)
            calls += 1
            assert h.kernel_time("fieldop")[1] == LAUNCHES * calls
            stage.append(h.device_ptr("view_stage"))
        assert h.kernel_time("fieldop")[0] > 0.0
        assert stage[0] == stage[1] and stage[0][1] == h.nelemd * 72 * 128
        assert stage[2] == stage[3] == stage[4] and stage[2][1] == h.nelemd * 144 * 128          # grown by the call with more layers
        assert stage[5] == stage[6] == stage[7] and stage[5][1] == h.nelemd * 146 * 128          # steady state: nothing is allocated
        for g in GROUPS:
            assert h.kernel_time(g)[1] == 0, g
        h.timing(False)
        for k in names:
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
    h, nlev = _hip(), 72
    f, _ = _case(nlev, "vorticity", True)
    lf = np.ascontiguousarray(np.moveaxis(f.reshape(f.shape[:3] + (16,)), 2, -1)).reshape(f.shape[0], 2, 4, 4, nlev)   # [e][c][j][i][k]
    x = (lf - 1.0) / 2.0
    made = x * 2.0 + 1.0                                                       # what the device will hold: the host knows its bits
    src = torch.from_numpy(made.copy()).cuda()
    ref = torch.zeros((f.shape[0], 4, 4, nlev), dtype=torch.float64, device="cuda")
    h.sphere_op_view(src, "eqjik", ref, "ejik", op="vorticity", c0=True)       # stream=None: complete on return
    want = ref.cpu().numpy()
    assert np.abs(want).max() > 0
    s = torch.cuda.Stream()
    pinned = torch.from_numpy(x).pin_memory()
    field = torch.zeros(pinned.shape, dtype=torch.float64, device="cuda")
    res = torch.zeros(ref.shape, dtype=torch.float64, device="cuda")
    out = torch.zeros(ref.shape, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        field.copy_(pinned, non_blocking=True)
        field.mul_(2.0); field.add_(1.0)                                       # the producer
        h.sphere_op_view(field, "eqjik", res, "ejik", op="vorticity", c0=True, stream=s)
        out.copy_(res, non_blocking=True)                                      # the consumer
        field.zero_(); res.zero_()                                             # the caller reuses its arrays at once
    torch.cuda.synchronize()
    assert dm.same(out.cpu().numpy(), want) and not res.any().item()
    # a stream that is being captured
    h.timing(True)
    keep = ref.clone()
    torch.cuda.synchronize()
    with vc.capturing(s):
        with pytest.raises(TseError, match="captured"):
            h.sphere_op_view(src, "eqjik", ref, "ejik", op="vorticity", c0=True, stream=s)
    assert h.kernel_time("fieldop")[1] == 0
    h.timing(False)
    assert torch.equal(ref.view(torch.int64), keep.view(torch.int64))


# ---- 8 ----
RANK_CASES = ((72, "dense", "lev0"), (73, "lev_odd", "dense"), (72, "lev0", "ij"), (1, "dense", "dense"), (3, "ij", "epad"))


def _rank_body(ne):
    from transport_se_amd import cube_mesh as cm
    nelem = 6 * ne * ne

    def body(rank, h, mine, geo, hv):
        import torch
        out = {}
        h.vector_setup(geo["D"][mine], cm.metinv(geo["D"])[mine], geo["mp"][mine])
        h.comm_timing(True)
        for c0 in MODES:
            for op in sm.OPS:
                for nk, name, out_name in RANK_CASES:
                    f = sm.random_field(nelem, sm.NF[op][0], nk, seed=7)[mine]
                    out[(nk, name, op, c0)] = _run(h, f, op, c0, name, out_name)
                    if c0:                                                    # claim 3 on this cut of the mesh: LOCAL, then dss_view(average)
                        t = torch.from_numpy(_run(h, f, op, False, name, "dense")).cuda()
                        h.dss_view(t, "eqkji", mode="average")
                        out[(nk, name, op, "composed")] = t.cpu().numpy()
            if not c0:
                out["comm local"] = sum(v[1] for v in h.comm_times().values())
        out["comm"] = sum(v[1] for v in h.comm_times().values())
        h.comm_timing(False)
        return out
    return body


def test_ranks_give_the_bits_of_one_context():
    from test_gpu_multirank_emulated import _run_ne
    ne = NE
    nelem = 6 * ne * ne
    (mine1, one), = _run_ne(1, ne=ne, body=_rank_body(ne))
    assert np.array_equal(np.sort(mine1), np.arange(nelem))
    assert one.pop("comm local") == 0 and one.pop("comm") == 0
    for key, val in one.items():
        full = np.empty_like(val); full[mine1] = val
        one[key] = full
    for (nk, name, op, c0), val in one.items():
        if c0 == "composed":
            assert dm.same(val, one[(nk, name, op, True)]), (nk, name, op)
    for world in (2, 3):
        res = _run_ne(world, ne=ne, body=_rank_body(ne))
        assert all(r is not None for r in res), world
        for mine, r in res:
            assert r["comm local"] == 0, (world, r["comm local"])               # LOCAL exchanges nothing
            assert r["comm"] > 0, world                                         # C0 packs, exchanges and waits
        for key, want in one.items():
            got = np.empty_like(want)
            for mine, r in res:
                got[mine] = r[key]
            assert dm.same(got, want), (world, key, int((dm.bits(got) != dm.bits(want)).sum()))


# ---- 9 ----
def test_refusals_launch_nothing():
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    nlev = 72
    h = _hip()
    f, want = _case(nlev, "vorticity", True)
    E, plane = h.nelemd, nlev * 16
    dense2, dense1 = [2 * plane, plane, 16, 4, 1], [plane, 0, 16, 4, 1]
    big = torch.full((2 * f.size + 64,), SENTINEL, dtype=torch.float64, device="cuda")   # room for in, and for an out that overlaps or touches it
    big[:f.size] = torch.from_numpy(np.array(f)).reshape(-1).cuda()
    buf = big[:f.size].view(f.shape)
    other = torch.full((E, nlev, 4, 4), SENTINEL, dtype=torch.float64, device="cuda")
    wind = torch.full(f.shape, SENTINEL, dtype=torch.float64, device="cuda")
    keep, keep_other, keep_wind = big.clone(), other.clone(), wind.clone()
    host = np.array(f)
    hout = np.zeros((E, nlev, 4, 4))

    def view(strides, ptr):
        return _lib.View(ptr, (C.c_longlong * 5)(*strides))
    p0 = buf.data_ptr()
    vin = view(dense2, p0)
    vout = view(dense1, other.data_ptr())
    # vorticity before vector_setup: a context of its own; gradient and divergence need no set-up
    bare = _make(setup=False)
    try:
        bare.timing(True)
        with pytest.raises(TseError, match="TSE_OP_VORTICITY: call tse_vector_setup first"):
            bare.sphere_op_view(buf, "eqkji", other, "ekji", op="vorticity")
        assert bare.kernel_time("fieldop")[1] == 0 and bare.device_ptr("view_stage") == (None, 0)
        assert torch.equal(other.view(torch.int64), keep_other.view(torch.int64))
        bare.sphere_op_view(buf, "eqkji", other, "ekji", op="divergence", c0=True)
        assert dm.same(other.cpu().numpy(), _run(h, np.array(f), "divergence", True, "dense", "dense")[:, 0])
        bare.sphere_op_view(other, "ekji", wind, "eqkji", op="gradient")
        assert bare.kernel_time("fieldop")[1] == 2 * LAUNCHES and not (wind == SENTINEL).any().item()
        bare.vector_setup(*_host())                                            # ... and after it the call is served
        bare.sphere_op_view(buf, "eqkji", other, "ekji", op="vorticity", c0=True)
        assert dm.same(other.cpu().numpy(), want[:, 0]) and bare.kernel_time("fieldop")[1] == 3 * LAUNCHES
        other.copy_(keep_other); wind.copy_(keep_wind)
    finally:
        bare.close()
    q1, nbytes = h.device_ptr("qdp1")
    assert nbytes == E * QSIZE * plane * 8
    libview = _Fake((E, QSIZE, nlev, 4, 4), [QSIZE * plane, plane, 16, 4, 1], q1)
    libscalar = _Fake((E, nlev, 4, 4), [QSIZE * plane, 16, 4, 1], q1)
    st, stbytes = h.device_ptr("view_stage")
    assert st and stbytes >= other.numel() * 8
    h.timing(True)
    V = lambda **kw: h.sphere_op_view(buf, "eqkji", other, "ekji", **kw)
    cases = [
        ("device", lambda: h.sphere_op_view(_Fake(f.shape, dense2, host.ctypes.data), "eqkji", other, "ekji")),
        ("device", lambda: h.sphere_op_view(buf, "eqkji", _Fake(hout.shape, [plane, 16, 4, 1], hout.ctypes.data), "ekji")),
        ("in: .* allocation of the library", lambda: h.sphere_op_view(libview, "eqkji", other, "ekji")),
        ("out: .* allocation of the library", lambda: h.sphere_op_view(buf, "eqkji", libscalar, "ekji")),
        ("out: .* allocation of the library", lambda: h.sphere_op_view(buf, "eqkji", _Fake(hout.shape, [plane, 16, 4, 1], st), "ekji")),   # the staging field itself
        ("op=3", lambda: V(op=3)),
        ("op=-1", lambda: V(op=-1)),
        ("unknown op", lambda: V(op="curl")),
        ("c0=2", lambda: V(op="vorticity", c0=2)),
        ("c0=-1", lambda: V(op="divergence", c0=-1)),
        ("nk = 0", lambda: h.sphere_op_view(vin, None, vout, nk=0)),
        ("nk = %d" % (nlev + 2), lambda: h.sphere_op_view(vin, None, vout, nk=nlev + 2)),
        ("field: .*extent 1, not 2", lambda: h.sphere_op_view(other, "ekji", wind, "eqkji", op="vorticity")),
        ("out: a scalar field has a q axis of extent 2", lambda: h.sphere_op_view(buf, "eqkji", wind, "eqkji", op="divergence")),
        ("field: a scalar field has a q axis of extent 2", lambda: h.sphere_op_view(buf, "eqkji", wind, "eqkji", op="gradient")),
        ("out: .*extent 1, not 2", lambda: h.sphere_op_view(other, "ekji", other, "ekji", op="gradient")),
        ("levels, field has", lambda: h.sphere_op_view(buf, "eqkji", other[:, :5], "ekji")),
        (r"stride 0 on the q axis.*\(in\)", lambda: h.sphere_op_view(view([2 * plane, 0, 16, 4, 1], p0), None, vout, nk=nlev)),
        (r"stride 0 on the j axis.*\(out\)", lambda: h.sphere_op_view(vin, None, view([plane, 0, 16, 0, 1], other.data_ptr()), nk=nlev)),
        (r"stride 0 on the q axis.*\(out\)", lambda: h.sphere_op_view(view(dense1, other.data_ptr()), None, view([2 * plane, 0, 16, 4, 1], wind.data_ptr()), op="gradient", nk=nlev)),
        ("overlaps in", lambda: h.sphere_op_view(vin, None, view(dense1, p0), nk=nlev)),                          # the same pointer: no in-place form
        ("overlaps in", lambda: h.sphere_op_view(vin, None, view(dense1, p0 + 8 * (f.size - 1)), nk=nlev)),       # one double shared
        ("overlaps in", lambda: h.sphere_op_view(vin, None, view([16 * nlev, 0, 1, 4 * nlev, nlev], p0 + 8 * 16), nk=nlev)),
        ("null view pointer", lambda: h.sphere_op_view(view(dense2, None), None, vout, nk=nlev)),
        ("null view pointer", lambda: h.sphere_op_view(vin, None, view(dense1, None), nk=nlev)),
        ("not 8-byte aligned", lambda: h.sphere_op_view(vin, None, view(dense1, other.data_ptr() + 4), nk=nlev)),
    ]
    for text, call in cases:
        print("sphere_op_view refusal:", text)
        with pytest.raises(TseError, match=text):
            call()
        assert h.kernel_time("fieldop")[1] == 0, text
        assert torch.equal(big.view(torch.int64), keep.view(torch.int64)), text
        assert torch.equal(other.view(torch.int64), keep_other.view(torch.int64)), text
        assert torch.equal(wind.view(torch.int64), keep_wind.view(torch.int64)), text
    L = h.L
    assert L.tse_sphere_op_view(h.h, nlev, 2, 1, None, None, None) != 0 and b"null" in L.tse_last_error()
    assert L.tse_sphere_op_view(h.h, nlev, 2, 1, C.byref(vin), None, None) != 0 and b"null" in L.tse_last_error()
    assert h.kernel_time("fieldop")[1] == 0
    # a good call afterwards: an out that touches in's end
    h.sphere_op_view(vin, None, view(dense1, p0 + 8 * f.size), op="vorticity", c0=True, nk=nlev)
    assert h.kernel_time("fieldop")[1] == LAUNCHES
    assert dm.same(big[f.size:f.size + other.numel()].view(other.shape).cpu().numpy(), want[:, 0]) and dm.same(buf.cpu().numpy(), f)
    assert torch.equal(big[f.size + other.numel():], keep[f.size + other.numel():])
    h.timing(False)
