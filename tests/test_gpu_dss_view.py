"""-m gpu: tse_dss_view -- direct stiffness summation of a host's own device arrays through strided views, in place.

The reference of every bit comparison is dss_view_model.model = rspheremp * Oracle.dss(w) (tests/test_dss_view_cpu.py holds it to the
longdouble DSS and shows that it sees a dropped corner, a swapped order, a missing rspheremp and a fused product), computed once per
(mesh, nf, nk, mode) on dss_view_model.field.
 1 bits        ne2 / ne3, both modes: every layout at nk = nlev with nf = 2; nf in {1, 2, 5} x nk in {1, nlev, nlev + 1} on the dense and on a
               level-fastest layout; one case each on the 64- and 80-level libraries; NaN-filled gaps keep every bit; the plan's path
 2 continuity  on the device result all copies of a shared node hold equal bits: at every node on inputs whose sums do not depend on the
               order of addition (every element its own integer, a mass matrix that is one per node), across edges on every field
 3 untouched   checksums of the library's fields, the next tracer step against a twin's, the timer groups
 4 growth      a call with more layers than the one before, then a smaller one
 5 stream      fill -> dss_view -> consumer on one side stream; a stream under capture is refused
 6 ranks       2 and 3 contexts on one GPU through the callback exchange == one context, bit for bit (the in-library RCCL exchange is
               not exercised here: test_gpu_rccl_exchange's loopback set-up runs its own fixed sequence of calls)
 7 refusals    nothing launched, the field unchanged"""
import ctypes as C
import functools

import numpy as np
import pytest

import dss_view_model as dm
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


@functools.lru_cache(maxsize=None)
def _case(ne, nf, nk, mode):
    """(field, the model's result), shared and read-only"""
    o = _oracle(ne)
    f = dm.field(o.nelem, nf, nk)
    want = dm.model(o, f, mode)
    f.setflags(write=False); want.setflags(write=False)
    return f, want


def _run(h, f, name, mode, stream=None):
    """dss_view of a host array through a layout -> the field afterwards; every gap must keep its bits"""
    import torch
    S = dm.Strided(f, name)
    buf = torch.from_numpy(S.host.copy()).cuda()
    h.dss_view(_Fake(S.shape, S.s, buf.data_ptr() + 8 * S.base), "eqkji", mode=mode, stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    got, gaps = S.read(buf.cpu().numpy())
    assert gaps, "bytes outside the view changed (%s)" % name
    return got


# ---- 1 / 2 ----
@pytest.mark.parametrize("mode", dm.MODES)
@pytest.mark.parametrize("ne", [2, 3])
def test_bits_of_the_model_on_every_layout(ne, mode):
    from transport_se_amd.hip_mod import dss_view_plan
    h, o, nlev = _hip(ne), _oracle(ne), 72
    paths = set()
    f, want = _case(ne, 2, nlev, mode)
    for name in dm.LAYOUTS:
        plan = dss_view_plan(h.nelemd, 2, nlev, dm.layout(name, h.nelemd, 2, nlev)[0])
        assert plan["path"] == dm.expected_path(name, nlev, nlev), (name, plan)
        paths.add(plan["path"])
        got = _run(h, f, name, mode)
        assert dm.same(got, want), (ne, mode, name, int((dm.bits(got) != dm.bits(want)).sum()))
        assert dm.continuous(o, got, copies=(2,))[0], (ne, mode, name)          # across an edge: a + b = b + a
    assert paths == {0, 1, 2}
    for nf in (1, 2, 5):
        for nk in (1, nlev, nlev + 1):
            f, want = _case(ne, nf, nk, mode)
            for name in ("dense", "lev_even"):
                got = _run(h, f, name, mode)
                assert dm.same(got, want), (ne, mode, name, nf, nk, int((dm.bits(got) != dm.bits(want)).sum()))
    assert not dm.same(_case(ne, 2, nlev, "average")[1], _case(ne, 2, nlev, "weak")[1])


@pytest.mark.parametrize("ne", [2, 3])
def test_device_result_is_continuous(ne):
    """On the device result all copies of a shared node hold equal bits, at every node of two, three and four elements: every element has
    its own value beforehand (dss_view_model.own_values: small integers, no sum depends on the order in which an element adds its
    neighbours) and the context's mass matrix is one per node (node_weights), the node identity comes from the mesh's coordinates.  The
    values are checked too: rspheremp times the exact total of the node, which is also the model's result.  (With the mesh's own
    rspheremp and fields of full mantissa width the copies of a node of three or four elements differ in the last bits, as in the
    reference: dss_view_model says why; test_bits_of_the_model_on_every_layout holds those to the model and, across edges, to equal bits.)"""
    o, nlev = _oracle(ne), 72
    w = dm.node_weights(o)
    h = _make(ne, weights=w)
    try:
        for nf, nk in ((2, nlev), (1, 1), (1, nlev + 1)):
            f = dm.own_values(o.nelem, nf, nk)
            assert not dm.continuous(o, f)[0]
            want = w[1][:, None, None] * dm.node_sums(o, f)
            for mode in dm.MODES:
                assert dm.same(dm.model(o, f, mode, weights=w), want)
                for name in ("dense", "lev0", "ij"):
                    got = _run(h, f, name, mode)
                    ok, nbad, n = dm.continuous(o, got)
                    assert ok and n > 0, (ne, nf, nk, mode, name, nbad, n)
                    assert dm.same(got, want), (ne, nf, nk, mode, name)
    finally:
        h.close()


def test_a_surface_field_and_a_layer_field_without_their_unit_axes():
    """a missing q or k letter: extent 1 and stride 0"""
    import torch
    ne, nlev = 2, 72
    h = _hip(ne)
    f, want = _case(ne, 1, 1, "average")
    ps = torch.from_numpy(np.array(f[:, 0, 0])).cuda()                        # [e][j][i]
    h.dss_view(ps, "eji")
    assert dm.same(ps.cpu().numpy(), want[:, 0, 0])
    f, want = _case(ne, 1, nlev, "weak")
    T = torch.from_numpy(np.ascontiguousarray(np.moveaxis(f[:, 0], 1, -1))).cuda()   # [e][j][i][k]
    h.dss_view(T, "ejik", mode="weak")
    assert dm.same(np.ascontiguousarray(np.moveaxis(T.cpu().numpy(), -1, 1)), want[:, 0])


@pytest.mark.parametrize("nlev", [64, 80])
def test_other_level_counts(nlev):
    ne = 2
    h = _hip(ne, nlev)
    for nf, nk, name, mode in ((2, nlev, "lev0", "average"), (2, nlev, "lev_odd", "weak"), (2, nlev, "dense", "average"), (1, nlev + 1, "lev_odd", "average"),
                               (1, nlev + 1, "epad", "weak")):
        f, want = _case(ne, nf, nk, mode)
        got = _run(h, f, name, mode)
        assert dm.same(got, want), (nlev, nf, nk, name, mode)


# ---- 3 ----
LIB_FIELDS = ("qdp1", "qdp2", "dp", "divdp", "divdp_proj", "dp3d", "ps_v", "qmin", "qmax")
GROUPS = ("dss", "view", "level", "fieldremap", "remap", "advance", "minmax")


def test_the_library_is_untouched():
    ne, nlev, dt = 2, 72, 1800.0
    o = _oracle(ne)
    h, twin = _make(ne), _make(ne)
    try:
        for x in (h, twin):
            x.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm)
            x.dcmip_set_initial()
            x.dcmip_step_inputs(0, dt); x.advec_tracers_remap_rk2(dt, 1, 2)      # leaves the element bounds of Qdp(2) cached
        before = {k: _raw(h, k) for k in LIB_FIELDS}
        h.timing(True)
        assert h.kernel_time("fielddss") == (0.0, 0)
        for i, (name, mode) in enumerate((("lev0", "average"), ("dense", "weak"), ("ij", "average"))):
            f, want = _case(ne, 2, nlev, mode)
            assert dm.same(_run(h, f, name, mode), want)
            assert h.kernel_time("fielddss")[1] == 2 * (i + 1)                   # the stage and the sum launch of every call
        assert h.kernel_time("fielddss")[0] > 0.0
        for g in GROUPS:
            assert h.kernel_time(g)[1] == 0, g
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


# ---- 4 ----
def test_buffers_grow_and_are_reused():
    ne, nlev = 3, 72
    h = _make(ne)
    try:
        for nf, nk, name in ((1, 1, "dense"), (5, nlev + 1, "lev_even"), (2, nlev, "lev0"), (5, nlev + 1, "dense"), (1, nlev, "lev_odd")):
            for mode in dm.MODES:
                f, want = _case(ne, nf, nk, mode)
                assert dm.same(_run(h, f, name, mode), want), (nf, nk, name, mode)
    finally:
        h.close()


# ---- 5 ----
def test_stream_order_and_capture():
    import torch
    from transport_se_amd.hip_mod import TseError
    ne, nlev, nf = 3, 72, 2
    h = _hip(ne)
    f, _ = _case(ne, nf, nlev, "average")
    lf = np.ascontiguousarray(np.moveaxis(f.reshape(f.shape[:3] + (16,)), 2, -1)).reshape(f.shape[0], nf, 4, 4, nlev)   # [e][q][j][i][k]
    x = (lf - 1.0) / 2.0
    made = x * 2.0 + 1.0                                                       # what the device will hold: the host knows its bits
    ref = torch.from_numpy(made.copy()).cuda()
    h.dss_view(ref, "eqjik")                                                   # stream=None: complete on return
    want = ref.cpu().numpy()
    assert not dm.same(want, made)
    s = torch.cuda.Stream()
    pinned = torch.from_numpy(x).pin_memory()
    field = torch.zeros(pinned.shape, dtype=torch.float64, device="cuda")
    out = torch.zeros(pinned.shape, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        field.copy_(pinned, non_blocking=True)
        field.mul_(2.0); field.add_(1.0)
        h.dss_view(field, "eqjik", stream=s)
        out.copy_(field, non_blocking=True)
        field.zero_()                                                          # the caller reuses its array at once
    torch.cuda.synchronize()
    assert dm.same(out.cpu().numpy(), want) and not field.any().item()
    # a stream that is being captured
    h.timing(True)
    keep = ref.clone()
    torch.cuda.synchronize()
    with vc.capturing(s):
        with pytest.raises(TseError, match="captured"):
            h.dss_view(ref, "eqjik", stream=s)
    assert h.kernel_time("fielddss")[1] == 0
    h.timing(False)
    assert torch.equal(ref.view(torch.int64), keep.view(torch.int64))


# ---- 6 ----
RANK_CASES = ((2, 72, "dense"), (2, 72, "lev0"), (1, 73, "lev_odd"), (3, 1, "dense"))   # none has the tracer exchange's qsize * nlev = 216 layers


def _rank_body(ne):
    nelem = 6 * ne * ne

    def body(rank, h, mine, geo, hv):
        out = {}
        for nf, nk, name in RANK_CASES:
            f = dm.field(nelem, nf, nk, seed=7)[mine]
            for mode in dm.MODES:
                out[(nf, nk, name, mode)] = _run(h, f, name, mode)
        return out
    return body


@pytest.mark.parametrize("ne", [3, 4])
def test_ranks_give_the_bits_of_one_context(ne):
    from test_gpu_multirank_emulated import _run_ne
    nelem = 6 * ne * ne
    (mine1, one), = _run_ne(1, ne=ne, body=_rank_body(ne))
    assert np.array_equal(np.sort(mine1), np.arange(nelem))
    for key, val in one.items():
        full = np.empty_like(val); full[mine1] = val
        one[key] = full
        f = dm.field(nelem, key[0], key[1], seed=7)
        assert not dm.same(full, f)
    for world in (2, 3):
        res = _run_ne(world, ne=ne, body=_rank_body(ne))
        assert all(r is not None for r in res), world
        for key, want in one.items():
            got = np.empty_like(want)
            for mine, r in res:
                got[mine] = r[key]
            assert dm.same(got, want), (ne, world, key, int((dm.bits(got) != dm.bits(want)).sum()))


# ---- 7 ----
def test_refusals_launch_nothing():
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    ne, nlev, nf = 2, 72, 2
    h = _hip(ne)
    f, want = _case(ne, nf, nlev, "average")
    E, plane = h.nelemd, nlev * 16
    dense = [nf * plane, plane, 16, 4, 1]
    buf = torch.from_numpy(np.array(f)).cuda()
    keep = buf.clone()
    host = np.array(f)
    h.timing(True)

    def view(strides, ptr):
        return _lib.View(ptr, (C.c_longlong * 5)(*strides))
    q1, nbytes = h.device_ptr("qdp1")
    assert nbytes == E * QSIZE * plane * 8
    # an allocation of the field's size made with the runtime itself, and the range the runtime reports for it (it may round the size
    # up): a view of the field's shape that ends one double beyond that range is refused, the one at the allocation's start is served
    raw = vc.RawAllocation(f.size * 8, fill=host)
    beyond, raw_now = raw.beyond, lambda: raw.read(f.shape)
    cases = [
        ("device", lambda: h.dss_view(_Fake(f.shape, dense, host.ctypes.data), "eqkji")),
        ("outside its allocation", lambda: h.dss_view(_Fake(f.shape, dense, beyond), "eqkji")),                        # one double beyond
        ("allocation of the library", lambda: h.dss_view(_Fake((E, QSIZE, nlev, 4, 4), [QSIZE * plane, plane, 16, 4, 1], q1), "eqkji")),
        ("mode=2", lambda: h.dss_view(buf, "eqkji", mode=2)),
        ("unknown mode", lambda: h.dss_view(buf, "eqkji", mode="strong")),
        ("nf = 0", lambda: h.dss_view(view(dense, buf.data_ptr()), None, nf=0, nk=nlev)),
        ("nk = %d" % (nlev + 2), lambda: h.dss_view(view(dense, buf.data_ptr()), None, nf=1, nk=nlev + 2)),
        ("stride 0 on the j axis", lambda: h.dss_view(view([nf * plane, plane, 16, 0, 1], buf.data_ptr()), None, nf=nf, nk=nlev)),
        ("overlap itself", lambda: h.dss_view(view([nf * plane, plane // 2, 16, 4, 1], buf.data_ptr()), None, nf=nf, nk=nlev)),
        ("null view pointer", lambda: h.dss_view(view(dense, None), None, nf=nf, nk=nlev)),
        ("not 8-byte aligned", lambda: h.dss_view(view(dense, buf.data_ptr() + 4), None, nf=nf, nk=nlev)),
    ]
    for text, call in cases:
        print("dss_view refusal:", text)
        with pytest.raises(TseError, match=text):
            call()
        assert h.kernel_time("fielddss")[1] == 0, text
        assert torch.equal(buf.view(torch.int64), keep.view(torch.int64)), text
    assert dm.same(raw_now(), f)
    L = h.L
    assert L.tse_dss_view(h.h, nf, nlev, 0, None, None) != 0 and b"null" in L.tse_last_error()
    h.dss_view(buf, "eqkji")
    assert h.kernel_time("fielddss")[1] == 2 and dm.same(buf.cpu().numpy(), want)
    h.dss_view(_Fake(f.shape, dense, raw.ptr), "eqkji")                        # the view that fits exactly is served
    assert dm.same(raw_now(), want)
    h.timing(False)
    raw.free()
