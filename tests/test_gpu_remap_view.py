"""-m gpu: tse_remap_view -- remap_Q_ppm of a host's own device arrays through strided views, in place, on the host's own grids.

Inputs: remap_ld.inputs / grids (24 elements, five grid families that reach one-layer and many-layer displacements; the 80-level ones
as tests/nlev80_common.py makes them).  The reference of every bit comparison is HipMod.remap_q_ppm of a context with qsize = nf
(k_remap through the host-array entry), computed once per (nlev, alg, nf).
 1 bits            dense point-fastest field == remap_q_ppm, nlev 72 / 64 / 80, alg 0 / 2, nf in remap_ld.QSIZES
 2 paths           level-fastest (unpadded, padded by 2 and by 3), element and q swapped, negative level stride, odd base, i/j swapped;
                   the three views on different paths; everything outside the footprints (a NaN payload pattern) keeps every bit
 3 nf / qsize      on a context with qsize = 4: nf = 1, 2, 19; slot f == the same columns remapped alone
 4 pointwise       remap_ld's longdouble bound as test_gpu_remap_pointwise._check holds it (nlev 72, alg 0 / 2, nf = 19)
 5 mean            a' == ((a * dp_src) remapped as mass) / dp_tgt, the products and quotients in numpy fp64; a zero target layer
 6 untouched       checksums of the library's fields, the next tracer step against a twin's, the timer groups
 7 own Qdp         the library's qdp2 as the field: bits, the cache dropped, Q stale; dp3d refused
 8 refusals        nothing launched
 9 bad grids       decided on the device per element: codes 1-4, the refused elements keep every bit, the others are remapped
10 stream order    fill -> remap_view -> consumer on one side stream, no host synchronisation"""
import ctypes as C
import functools

import numpy as np
import pytest

import view_common as vc
from view_common import FakeArray as _Fake, raw_field as _raw

pytestmark = pytest.mark.gpu
NLEVS = (72, 64, 80)
PAYLOAD = 0x7FF8DEAD00000000   # quiet NaNs that carry their own index


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rl(nlev):
    import remap_ld as rl
    if nlev == 80:
        import nlev80_common  # noqa: F401  (teaches remap_ld the 80-level grid)
    return rl


@functools.lru_cache(maxsize=None)
def _inputs(nlev, nf):
    return _rl(nlev).inputs(nlev, nf)


@functools.lru_cache(maxsize=None)
def _hip(nlev, qsize, alg=0):
    """a context on the ne2 mesh (kept for the session: contexts are small)"""
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.driver import partition
    from transport_se_amd.hip_mod import HipMod
    rl = _rl(nlev)
    hv = rl.hvcoord(nlev)
    topo = cm.topology(2); geo = cm.geometry(2, topo)
    d = cm.edge_descriptors(topo, partition(2, 1), 0)
    mine = d["elems"]
    elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, 1e19, device=0, vert_remap_q_alg=alg)
    assert h.nlev == nlev and h.nelemd == rl.NELEM
    h.mine, h.hv = mine, hv
    return h


@functools.lru_cache(maxsize=None)
def _ref(nlev, alg, nf):
    """the bits every test compares with: tse_remap_q_ppm of a context with qsize = nf"""
    Q, dp1, dp2 = _inputs(nlev, nf)
    h = _hip(nlev, nf, alg)
    out = h.remap_q_ppm(Q, dp1, dp2)
    out.setflags(write=False)
    return out


# ---- layouts: (strides of e, q, k, j, i; base; size) in doubles for a field of nf slots; nf = 0: a grid (no q axis) ----
def _layout(name, E, nf, K):
    q = max(nf, 1)
    if name == "dense":
        s, base, size = [q * K * 16, K * 16, 16, 4, 1], 0, E * q * K * 16
    elif name in ("lev0", "lev2", "lev3"):       # [e][q][j][i][k + pad]
        S = K + int(name[3])
        s, base, size = [q * 16 * S, 16 * S, 1, 4 * S, S], 0, E * q * 16 * S
    elif name == "oddbase":                     # level-fastest rows one double off a 16-byte boundary
        s, base, size = [q * 16 * K, 16 * K, 1, 4 * K, K], 1, E * q * 16 * K + 1
    elif name == "swap":                        # [q][e][k][j][i]
        s, base, size = [K * 16, E * K * 16, 16, 4, 1], 0, E * q * K * 16
    elif name == "negk":                        # levels stored bottom-up
        s, base, size = [q * K * 16, K * 16, -16, 4, 1], (K - 1) * 16, E * q * K * 16
    elif name == "ij":                          # [e][q][k][i][j]: any strides
        s, base, size = [q * K * 16 + 5, K * 16, 16, 1, 4], 3, E * (q * K * 16 + 5) + 3
    else:
        raise ValueError(name)
    if nf == 0:
        s[1] = 0
    return s, base, size


PATH = dict(dense=0, lev0=1, lev2=1, lev3=1, oddbase=1, swap=0, negk=0, ij=2)


def _index(s, base, shape):
    ix = np.full(shape, base, dtype=np.int64)
    for ax, n in enumerate(shape):
        sh = [1] * len(shape); sh[ax] = n
        ix = ix + s[ax] * np.arange(n, dtype=np.int64).reshape(sh)
    return ix


class _Dev:
    """host data laid into a payload-filled device buffer as a layout names it"""
    def __init__(self, data, name):
        import torch
        data = np.asarray(data, dtype=np.float64)
        grid = data.ndim == 4
        d5 = data[:, None] if grid else data
        E, q, K = d5.shape[:3]
        self.s, self.base, size = _layout(name, E, 0 if grid else q, K)
        self.ix = _index(self.s, self.base, d5.shape)
        assert np.unique(self.ix).size == self.ix.size and self.ix.min() >= 0 and self.ix.max() < size
        host = (np.uint64(PAYLOAD) + np.arange(size, dtype=np.uint64)).view(np.float64)
        host[self.ix] = d5
        self.host, self.grid, self.shape = host, grid, d5.shape
        self.buf = torch.from_numpy(host.copy()).cuda()
        self.view = _Fake(d5.shape, self.s, self.buf.data_ptr() + 8 * self.base)
        self.axes = "eqkji"

    def args(self):
        """(array, axes) as HipMod.remap_view takes them"""
        if self.grid:
            return _Fake((self.shape[0],) + self.shape[2:], [self.s[0]] + self.s[2:], self.buf.data_ptr() + 8 * self.base), "ekji"
        return self.view, "eqkji"

    def result(self):
        out = self.buf.cpu().numpy()
        got = out[self.ix]
        mask = np.ones(out.size, dtype=bool); mask[self.ix.ravel()] = False
        assert np.array_equal(_bits(out[mask]), _bits(self.host[mask])), "bytes outside the view changed"
        return got[:, 0] if self.grid else got


def _run(h, field, src, tgt, lf="dense", ls="dense", lt="dense", **kw):
    """remap_view of host arrays through the named layouts -> (return code, the field afterwards); the grids and all padding must keep their bits"""
    F, S, T = _Dev(field, lf), _Dev(src, ls), _Dev(tgt, lt)
    rc = h.remap_view(*F.args(), *S.args(), *T.args(), **kw)
    if kw.get("stream") is not None:
        import torch
        torch.cuda.synchronize()
    assert _same(S.result(), np.asarray(src)) and _same(T.result(), np.asarray(tgt))
    return rc, F.result()


# ---- 1 ----
@pytest.mark.parametrize("alg", [0, 2])
@pytest.mark.parametrize("nlev", NLEVS)
def test_bits_of_remap_q_ppm(nlev, alg):
    rl = _rl(nlev)
    h = _hip(nlev, 4)
    for nf in rl.QSIZES:
        Q, dp1, dp2 = _inputs(nlev, nf)
        rc, got = _run(h, Q, dp1, dp2, alg=alg)
        assert rc == 0 and _same(got, _ref(nlev, alg, nf)), (nlev, alg, nf)
    assert not _same(_ref(nlev, 0, 3), _ref(nlev, 2, 3))


# ---- 2 ----
COMBOS = [("lev0", "dense", "dense"), ("lev2", "lev3", "ij"), ("lev3", "dense", "lev0"), ("swap", "negk", "lev2"), ("negk", "ij", "oddbase"),
          ("oddbase", "lev0", "negk"), ("ij", "oddbase", "lev3"), ("dense", "lev2", "swap")]


@pytest.mark.parametrize("nlev", NLEVS)
def test_paths_give_the_same_bits_and_keep_the_padding(nlev):
    from transport_se_amd.hip_mod import remap_view_plan
    h = _hip(nlev, 4)
    for nf, alg in ((3, 0), (19, 2)):
        Q, dp1, dp2 = _inputs(nlev, nf)
        for lf, ls, lt in COMBOS:
            plan = remap_view_plan(h.nelemd, nf, _layout(lf, h.nelemd, nf, nlev)[0], _layout(ls, h.nelemd, 0, nlev)[0], _layout(lt, h.nelemd, 0, nlev)[0], nlev=nlev)
            assert [p["path"] for p in plan] == [PATH[lf], PATH[ls], PATH[lt]], (lf, ls, lt, plan)
            rc, got = _run(h, Q, dp1, dp2, lf, ls, lt, alg=alg)
            assert rc == 0 and _same(got, _ref(nlev, alg, nf)), (nlev, nf, alg, lf, ls, lt)


# ---- 3 ----
def test_nf_is_independent_of_qsize_and_a_column_of_its_companions():
    nlev = 72
    h = _hip(nlev, 4)
    Q, dp1, dp2 = _inputs(nlev, 19)
    alone = [_run(h, Q[:, f:f + 1], dp1, dp2)[1] for f in range(19)]
    for f in range(19):
        assert _same(alone[f], _ref(nlev, 0, 19)[:, f:f + 1]), f
    for nf in (1, 2, 19):
        for layout in ("dense", "lev0"):
            rc, got = _run(h, Q[:, :nf], dp1, dp2, layout)
            assert rc == 0
            for f in range(nf):
                assert _same(got[:, f:f + 1], alone[f]), (nf, layout, f)


# ---- 4 ----
@pytest.mark.parametrize("alg", [0, 2])
def test_pointwise_bound(alg):
    from step_ld import has_extended_precision
    from test_gpu_remap_pointwise import _check
    assert has_extended_precision(), np.finfo(np.longdouble)
    rl, nlev, nf = _rl(72), 72, 19
    Q, dp1, dp2 = _inputs(nlev, nf)
    t, safe, kid = rl.remap_q_ppm(Q, dp1, dp2, alg)
    for layout in ("dense", "lev0"):
        rc, got = _run(_hip(nlev, 4), Q, dp1, dp2, layout, alg=alg)
        assert rc == 0 and np.isfinite(got).all()
        worst = {}
        _check("remap_view L%d alg%d %s" % (nlev, alg, layout), nf, got, Q, t, safe, kid, worst)   # the bound at safe outputs, UNSAFE_TOL elsewhere, every column's mass
        for key, val in sorted(worst.items(), key=str):
            print("remap_view pointwise alg%d %s %s: %.4g" % (alg, layout, key, val[0]))


# ---- 5 ----
@pytest.mark.parametrize("nlev", NLEVS)
def test_mean_mode(nlev):
    h = _hip(nlev, 4)
    nf = 3
    Q, dp1, dp2 = _inputs(nlev, nf)
    a = Q / dp1[:, None]
    for alg in (0, 2):
        m = a * dp1[:, None]                                   # one fp64 product
        rc, m2 = _run(h, m, dp1, dp2, alg=alg)
        want = m2 / dp2[:, None]                               # a true division
        assert rc == 0
        for lf, ls, lt in (("dense", "dense", "dense"), ("lev0", "lev2", "lev0"), ("lev3", "dense", "lev3"), ("ij", "ij", "ij"), ("oddbase", "negk", "swap")):
            rc, got = _run(h, a, dp1, dp2, lf, ls, lt, mode="mean", alg=alg)
            assert rc == 0 and _same(got, want), (nlev, alg, lf, ls, lt)
    # a target grid with an empty layer: a mean cannot be divided by it, a mass does not care
    z = dp2.copy(); z[2, 6, 1, 3] += z[2, 5, 1, 3]; z[2, 5, 1, 3] = 0.0
    rc, got = _run(h, a, dp1, z, mode="mean", alg=2)
    assert rc == 2 and "dp2 is zero" in h.last_error() and "element 2, column 7, level 5" in h.last_error(), h.last_error()
    assert _same(got[2], a[2])
    keep = [e for e in range(h.nelemd) if e != 2]
    assert _same(got[keep], want[keep])                         # (alg 2, the last of the loop above)
    rc, got = _run(h, Q, dp1, z, alg=2)
    assert rc == 0 and np.isfinite(got).all() and _same(got[keep], _ref(nlev, 2, nf)[keep])


# ---- 6 / 7: the library's own state ----
LIB_FIELDS = ("qdp1", "qdp2", "dp", "divdp", "divdp_proj", "dp3d", "ps_v", "qmin", "qmax")


def _state_after_one_step(h, dt=1800.0):
    from transport_se_amd import cube_mesh as cm
    geo = cm.geometry(2, cm.topology(2))
    h.dcmip_init(1, geo["lat"][h.mine], geo["lon"][h.mine], h.hv.hyam, h.hv.hybm)
    h.dcmip_set_initial()
    h.dcmip_step_inputs(0, dt); h.advec_tracers_remap_rk2(dt, 1, 2)       # leaves the element bounds of Qdp(2) cached


def _twin(nlev, qsize):
    """a second context of the same shape (never the cached one)"""
    return _hip.__wrapped__(nlev, qsize)


def test_the_library_is_untouched():
    nlev, dt = 72, 1800.0
    h, twin = _hip(nlev, 4), _twin(nlev, 4)
    try:
        for x in (h, twin):
            _state_after_one_step(x)
        before = {k: _raw(h, k) for k in LIB_FIELDS}
        h.timing(True)
        Q, dp1, dp2 = _inputs(nlev, 19)
        rc, got = _run(h, Q, dp1, dp2, "lev0")
        assert rc == 0 and _same(got, _ref(nlev, 0, 19))
        assert h.kernel_time("fieldremap")[1] == 1 and h.kernel_time("remap")[1] == 0
        h.timing(False)
        for k in LIB_FIELDS:
            assert _same(_raw(h, k), before[k]), k
        for x in (h, twin):                                                  # the cached bounds survive: the next step is the twin's
            x.dcmip_step_inputs(1, dt); x.advec_tracers_remap_rk2(dt, 2, 1)
        shape = (h.nelemd, 4, nlev, 4, 4)
        assert _same(h.fetch("qdp1", shape), twin.fetch("qdp1", shape))
        assert all(_same(a, b) for a, b in zip(h.get_qminmax(), twin.get_qminmax()))
    finally:
        twin.close()


def test_the_librarys_own_qdp_as_the_field():
    from transport_se_amd.hip_mod import TseError
    nlev, dt, nf = 72, 1800.0, 3
    h, twin = _hip(nlev, nf), _twin(nlev, nf)
    try:
        Q, dp1, dp2 = _inputs(nlev, nf)
        shape = Q.shape
        elem = dict(Qdp=np.ascontiguousarray(np.stack([Q, Q], axis=1)))
        for x in (h, twin):
            _state_after_one_step(x)
            x.copy_qdp_h2d(elem, 2)
        out = dict(Q=np.zeros(shape))
        h.state_q(2); h.copy_q_d2h(out)
        S, T = _Dev(dp1, "dense"), _Dev(dp2, "lev0")
        plane = nlev * 16
        dense = [nf * plane, plane, 16, 4, 1]
        q2, _ = h.device_ptr("qdp2")
        assert h.remap_view(_Fake(shape, dense, q2), "eqkji", *S.args(), *T.args()) == 0
        got = h.fetch("qdp2", shape)
        assert _same(got, _ref(nlev, 0, nf))
        with pytest.raises(TseError, match="stale"):                        # Q / lnps went stale with the field
            h.copy_q_d2h(out)
        twin.copy_qdp_h2d(dict(Qdp=np.ascontiguousarray(np.stack([got, got], axis=1))), 2)
        for x in (h, twin):                                                  # the cache is dropped: both form their bounds afresh
            x.dcmip_step_inputs(1, dt); x.advec_tracers_remap_rk2(dt, 2, 1)
        assert _same(h.fetch("qdp1", shape), twin.fetch("qdp1", shape))
        # every other allocation of the library is out of reach, as the field or as a grid
        d3, _ = h.device_ptr("dp3d")
        F = _Dev(Q[:, :1], "dense")
        with pytest.raises(TseError, match="allocation of the library"):
            h.remap_view(_Fake((h.nelemd, 1, nlev, 4, 4), [plane, plane, 16, 4, 1], d3), "eqkji", *S.args(), *T.args())
        with pytest.raises(TseError, match="allocation of the library"):
            h.remap_view(*F.args(), _Fake((h.nelemd, nlev, 4, 4), [plane, 16, 4, 1], d3), "ekji", *T.args())
        with pytest.raises(TseError, match="allocation of the library"):
            h.remap_view(*F.args(), *S.args(), _Fake((h.nelemd, nlev, 4, 4), [nf * plane, 16, 4, 1], q2), "ekji")
        assert _same(F.result(), Q[:, :1])
    finally:
        twin.close()


# ---- 8 ----
def test_refusals_launch_nothing():
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    nlev, nf = 72, 3
    h = _hip(nlev, 4)
    Q, dp1, dp2 = _inputs(nlev, nf)
    F, S, T = _Dev(Q, "dense"), _Dev(dp1, "dense"), _Dev(dp2, "dense")
    E, plane = h.nelemd, nlev * 16
    dense, gdense = [nf * plane, plane, 16, 4, 1], [plane, 16, 4, 1]
    h.timing(True)
    assert h.remap_view(*F.args(), *S.args(), *T.args()) == 0
    n0 = h.kernel_time("fieldremap")[1]
    assert n0 == 1
    after = F.buf.clone()
    host = np.zeros(Q.shape)
    fp, sp = F.buf.data_ptr(), S.buf.data_ptr()

    def view(strides, ptr):
        return _lib.View(ptr, (C.c_longlong * 5)(*strides))
    g5 = [plane, 0, 16, 4, 1]
    cases = [
        ("device", lambda: h.remap_view(_Fake(Q.shape, dense, host.ctypes.data), "eqkji", *S.args(), *T.args())),
        ("device", lambda: h.remap_view(*F.args(), _Fake(dp1.shape, gdense, dp1.ctypes.data), "ekji", *T.args())),
        ("outside its allocation", lambda: h.remap_view(_Fake(Q.shape, [1 << 40] + dense[1:], fp), "eqkji", *S.args(), *T.args())),
        ("outside its allocation", lambda: h.remap_view(*F.args(), *S.args(), _Fake(dp1.shape, [1 << 40] + gdense[1:], T.buf.data_ptr()), "ekji")),
        ("overlaps dp_src", lambda: h.remap_view(*F.args(), _Fake(dp1.shape, gdense, fp + 8 * plane), "ekji", *T.args())),
        ("overlaps dp_tgt", lambda: h.remap_view(_Fake((E, 1, nlev, 4, 4), [plane, plane, 16, 4, 1], sp), "eqkji", *T.args(), *S.args())),
        ("overlap itself", lambda: h.remap_view(view([nf * plane, plane // 2, 16, 4, 1], fp), None, *S.args(), *T.args(), nf=nf)),
        ("stride 0", lambda: h.remap_view(view([nf * plane, plane, 16, 0, 1], fp), None, *S.args(), *T.args(), nf=nf)),
        ("nf = 0", lambda: h.remap_view(view(dense, fp), None, *S.args(), *T.args(), nf=0)),
        ("mode=2", lambda: h.remap_view(*F.args(), *S.args(), *T.args(), mode=2)),
        ("unknown mode", lambda: h.remap_view(*F.args(), *S.args(), *T.args(), mode="layer")),
        ("alg=3", lambda: h.remap_view(*F.args(), *S.args(), *T.args(), alg=3)),
        ("alg=-1", lambda: h.remap_view(*F.args(), *S.args(), *T.args(), alg=-1)),
        ("null view pointer", lambda: h.remap_view(*F.args(), view(g5, None), None, *T.args())),
        ("not 8-byte aligned", lambda: h.remap_view(*F.args(), view(g5, sp + 4), None, *T.args())),
    ]
    for text, call in cases:
        with pytest.raises(TseError, match=text):
            call()
    L = h.L
    assert L.tse_remap_view(h.h, nf, 0, 0, None, None, None, None) != 0 and b"null" in L.tse_last_error()
    assert L.tse_remap_view(None, nf, 0, 0, None, None, None, None) != 0 and b"null" in L.tse_last_error()
    # a stream that is being captured
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with vc.capturing(s):
        with pytest.raises(TseError, match="captured"):
            h.remap_view(*F.args(), *S.args(), *T.args(), stream=s)
    assert h.kernel_time("fieldremap")[1] == n0 and h.kernel_time("remap")[1] == 0
    h.timing(False)
    assert torch.equal(F.buf.view(torch.int64), after.view(torch.int64)) and _same(F.result(), _ref(nlev, 0, nf))
    assert h.remap_view_status() == (0, None)


# ---- 9 ----
def _plant(dp1, dp2, nlev):
    """one offence of each code in four of the 24 elements -> (dp1, dp2, {element: (code, column, level)})"""
    a, b = dp1.copy(), dp2.copy()
    a[4, 10, 1, 2] = -1.0                                                      # 1: dp_src not positive
    a[9, :, 0, 1] = 1.0; a[9, 0, 0, 1] = 2.0 ** 53 - (nlev - 1)                # 2: sum(dp_src) = 2^53
    b[15, 20, 3, 3] = -1e-3                                                    # 3: dp_tgt negative
    b[22, :, 2, 1] *= 3.0                                                      # 4: the target column leaves the source column
    return a, b


@pytest.mark.parametrize("nlev", NLEVS)
def test_bad_grids_are_decided_on_the_device(nlev):
    import torch
    from host_tables import check_remap_grids
    h = _hip(nlev, 4)
    nf = 3
    Q, dp1, dp2 = _inputs(nlev, nf)
    a, b = _plant(dp1, dp2, nlev)
    bad = (4, 9, 15, 22)
    # what the shared column check says of every element alone, on the host
    want = {}
    for e in range(h.nelemd):
        r = check_remap_grids(a[e:e + 1], b[e:e + 1])
        assert (r is not None) == (e in bad), (e, r)
        if r:
            want[e] = r
    codes = {4: 1, 9: 2, 15: 3, 22: 4}
    good = [e for e in range(h.nelemd) if e not in bad]
    for lf, ls, lt in (("dense", "dense", "dense"), ("lev0", "lev3", "ij")):
        rc, got = _run(h, Q, a, b, lf, ls, lt)
        assert rc == 2
        msg = h.last_error()
        assert "4 of %d elements" % h.nelemd in msg and want[4][1].replace("element 0", "element 4") in msg, msg
        assert _same(got[list(bad)], Q[list(bad)])                              # refused: every bit kept
        assert _same(got[good], _ref(nlev, 0, nf)[good])                        # the others: the clean run's bits
        p, nbytes = h.device_ptr("remap_status")
        st = np.empty((h.nelemd, 4), dtype=np.int32)
        assert nbytes == st.nbytes and C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(st.ctypes.data), C.c_void_p(p), C.c_size_t(nbytes), C.c_int(2)) == 0
        for e in range(h.nelemd):
            if e in bad:
                (_, col, lev), _msg = want[e]
                assert tuple(st[e, :3]) == (codes[e], col, lev), (e, st[e], want[e])
            else:
                assert tuple(st[e, :3]) == (0, 0, 0), (e, st[e])
    # with a stream: 0 now, the verdict later, accumulated over calls until it is read
    s = torch.cuda.Stream()
    rc, got = _run(h, Q, a, b, "lev0", "dense", "lev2", stream=s)
    assert rc == 0 and _same(got[list(bad)], Q[list(bad)]) and _same(got[good], _ref(nlev, 0, nf)[good])
    first = (4,) + want[4][0][1:] + (1,)
    assert h.remap_view_status() == (4, first)
    assert h.remap_view_status() == (0, None)
    c, d = dp1.copy(), dp2.copy(); d[2, 3, 0, 0] = np.nan
    assert _run(h, Q, c, d, stream=s)[0] == 0 and _run(h, Q, a, b, stream=s)[0] == 0
    assert h.remap_view_status() == (5, (2, 0, 3, 3))                          # the lowest element of the EARLIEST call
    assert h.remap_view_status() == (0, None)


# ---- 10 ----
def test_stream_order():
    import torch
    nlev, nf = 72, 3
    h = _hip(nlev, 4)
    Q, dp1, dp2 = _inputs(nlev, nf)
    S, T = _Dev(dp1, "dense"), _Dev(dp2, "dense")
    lf = np.ascontiguousarray(np.moveaxis(Q.reshape(Q.shape[:3] + (16,)), 2, -1)).reshape(Q.shape[0], nf, 4, 4, nlev)   # [e][q][j][i][k]
    x = (lf - 1.0) / 2.0
    made = x * 2.0 + 1.0                                                       # what the device will hold: the host knows its bits
    Qm = np.ascontiguousarray(np.moveaxis(made.reshape(Q.shape[0], nf, 16, nlev), -1, 2)).reshape(Q.shape)
    want = _hip(nlev, nf).remap_q_ppm(Qm, dp1, dp2)
    s = torch.cuda.Stream()
    pinned = torch.from_numpy(x).pin_memory()
    field = torch.zeros(pinned.shape, dtype=torch.float64, device="cuda")
    out = torch.zeros(pinned.shape, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        field.copy_(pinned, non_blocking=True)
        field.mul_(2.0); field.add_(1.0)
        assert h.remap_view(field, "eqjik", *S.args(), *T.args(), stream=s) == 0
        out.copy_(field, non_blocking=True)
        field.zero_()                                                          # the caller reuses its array at once
    torch.cuda.synchronize()
    got = np.ascontiguousarray(np.moveaxis(out.cpu().numpy().reshape(Q.shape[0], nf, 16, nlev), -1, 2)).reshape(Q.shape)
    assert _same(got, want) and not field.any().item()
    assert h.remap_view_status() == (0, None)
