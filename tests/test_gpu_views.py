"""-m gpu: state exchange with a GPU-resident host through strided device views (tse_view_put / tse_view_get; HipMod.put / get).

The views only move data, so every comparison is bit for bit against the host route -- tse_copy_qdp_h2d/_d2h, tse_set_derived,
tse_set_divdp, tse_get_derived, tse_copy_q_d2h, tse_copy_lnps_d2h -- on every conversion path (0 point-fastest, 1 level-fastest through
LDS in its 16-byte and 8-byte forms, 2 generic), with padding that must keep its bytes, on a non-default stream without host
synchronisation, and at 72, 64 and 80 levels.  Device arrays are torch tensors; their memory belongs to torch.  No view here leaves
its tensor: the refusal tests pass only views the library's checks turn down before anything is launched."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import view_common
import view_model as vm
from view_common import FakeArray as _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VC = os.path.join(ROOT, "tests", "golden", "vcoord")
pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FF4DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
SBITS = np.uint64(0x7FF4DEADBEEF0001)
# the library's own array of every put field, for HipMod.fetch
LIB_NAME = {"qdp": "qdp%d", "vn0": "vn0", "dp": "dp", "eta_dot_dpdn": "eta_dot_dpdn", "omega_p": "omega_p", "divdp": "divdp",
            "divdp_proj": "divdp_proj"}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# layouts: (label, strides in doubles, doubles the buffer needs, offset of the view's first entry, expected path)
def layouts(ext, has):
    e, q, k, j, i = range(5)
    pr = lambda order: [a for a in order if has[a]]   # noqa: E731
    K, lev = ext[k], has[k]
    out = []
    s, n = vm.nested_strides(ext, pr((i, j, k, q, e)))
    out.append(("p0 dense", s, n, 0, 0))
    last = q if has[q] else (k if has[k] else j)   # the axis below the element axis: qsize_d = 5 tracers per element and a gap of 48 doubles
    s, n = vm.nested_strides(ext, pr((i, j, k, q, e)), pads={last: ((5 - ext[q]) * K * 16 if has[q] else 0) + 48})
    out.append(("p0 qsize_d=5 and an element gap", s, n, 0, 0))
    s, n = vm.nested_strides(ext, pr((k, i, j, q, e)))
    out.append(("p1 dense", s, n, 0, 1 if lev else 0))
    s, n = vm.nested_strides(ext, pr((k, i, j, q, e)), pads={k: 3} if lev else {j: 3})
    out.append(("p1 rows padded by 3", s, n, 0, 1 if lev else 0))
    s, n = vm.nested_strides(ext, pr((k, i, j, q, e)))
    out.append(("p1 base shifted by one double", s, n + 1, 1, 1 if lev else 0))
    s, n = vm.nested_strides(ext, pr((e, i, j, k, q)))
    out.append(("p2 element index fastest", s, n, 0, 2 if ext[e] > 1 else 0))
    return [(lab, s, n + 5, base, path) for lab, s, n, base, path in out]   # (five spare doubles behind every view)


def _tensor(torch, buf, ext, has, strides, base):
    """the strided torch view of the flat device buffer, its dimensions in the order e q k j i (the axes the field has)"""
    size = [n for n, h in zip(ext, has) if h]
    st = [s for s, h in zip(strides, has) if h]
    axes = "".join(a for a, h in zip(vm.AXES, has) if h)
    return torch.as_strided(buf, size, st, base), axes


def _logical(rng, ext, has):
    return rng.standard_normal([n for n, h in zip(ext, has) if h])


def _host_put(hip, field, x, nt):
    """the host entry that writes `field` (x: the field's own array, axes e q k j i)"""
    n, K = hip.nelemd, hip.nlev
    if field == "qdp":
        qd = np.zeros((n, 2, hip.qsize, K, 4, 4)); qd[:, nt - 1] = x
        hip.copy_qdp_h2d(dict(Qdp=qd), nt)
    elif field == "vn0":
        hip.set_derived(dict(vn0=np.ascontiguousarray(x.transpose(0, 2, 1, 3, 4))))   # elem%derived%vn0 is [e][k][c][j][i]
    elif field in ("dp", "eta_dot_dpdn", "omega_p"):
        hip.set_derived({field: np.ascontiguousarray(x)})
    else:
        hip.set_divdp({field: np.ascontiguousarray(x)})


def _fetch(hip, field, nt):
    n, K = hip.nelemd, hip.nlev
    shape = {"qdp": (n, hip.qsize, K, 4, 4), "vn0": (n, K, 2, 4, 4), "eta_dot_dpdn": (n, K + 1, 4, 4)}.get(field, (n, K, 4, 4))
    return hip.fetch(LIB_NAME[field] % nt if field == "qdp" else LIB_NAME[field], shape)


def check_put(hip, fields, seed=1, stream=None):
    """test 1: for every field and layout, put + fetch == what the host entry leaves.  Returns the number of put calls."""
    import torch
    rng = np.random.default_rng(seed)
    calls = 0
    for field in fields:
        ext, has = vm.extents(field, hip.nelemd, hip.qsize, hip.nlev), vm.has_axes(field)
        for t, (label, strides, size, base, path) in enumerate(layouts(ext, has)):
            nt = 1 + t % 2
            x = _logical(rng, ext, has)
            _host_put(hip, field, x, nt)
            ref = _fetch(hip, field, nt)
            _host_put(hip, field, _logical(rng, ext, has), nt)          # other data, so that the put has something to do
            assert not _same(_fetch(hip, field, nt), ref)
            host = vm.scatter(field, x, hip.nelemd, hip.qsize, hip.nlev, strides, np.full(size, SENTINEL), base)
            buf = torch.from_numpy(host).cuda()
            arr, axes = _tensor(torch, buf, ext, has, strides, base)
            assert hip.view_plan(field, arr, axes)["path"] == path, (field, label)
            torch.cuda.synchronize()
            hip.put(field, arr, axes, nt=nt, stream=stream)
            calls += 1
            assert _same(_fetch(hip, field, nt), ref), (field, label)
            assert _same(buf.cpu().numpy(), host), (field, label, "a put wrote into its source")
    return calls


def host_get_refs(hip, fields, nt):
    """test 2's references: what the host entries download"""
    n, K, qs = hip.nelemd, hip.nlev, hip.qsize
    der = dict(divdp_proj=np.zeros((n, K, 4, 4)), eta_dot_dpdn=np.zeros((n, K, 4, 4)), omega_p=np.zeros((n, K, 4, 4)), divdp=np.zeros((n, K, 4, 4)),
               dp3d=np.zeros((n, K, 4, 4)), ps_v=np.zeros((n, 4, 4)))
    hip.get_derived(der)
    refs = {f: der[f] for f in fields if f in der}
    if "qdp" in fields:
        qd = np.zeros((n, 2, qs, K, 4, 4)); hip.copy_qdp_d2h(dict(Qdp=qd), nt); refs["qdp"] = qd[:, nt - 1].copy()
    if "q" in fields:
        out = dict(Q=np.zeros((n, qs, K, 4, 4)), lnps=np.zeros((n, 4, 4)))
        hip.copy_q_d2h(out); hip.copy_lnps_d2h(out)
        refs["q"], refs["lnps"] = out["Q"], out["lnps"]
    return refs


def check_get(hip, refs, nt, stream=None):
    """test 2: for every field and layout, get == the host entry's download; every other double of the destination keeps its sentinel.
    Returns the number of get calls."""
    import torch
    calls = 0
    for field, ref in refs.items():
        ext, has = vm.extents(field, hip.nelemd, hip.qsize, hip.nlev, True), vm.has_axes(field, True)
        extra = []
        if field == "eta_dot_dpdn":   # a destination with nlev + 1 levels per element: the last one is not the library's to write
            s, n = vm.nested_strides((ext[0], 1, ext[2] + 1, 4, 4), [4, 3, 2, 0])
            extra = [("p0 rows of nlev + 1 levels", s, n, 0, 0)]
        for label, strides, size, base, path in layouts(ext, has) + extra:
            buf = torch.full((size,), float("nan"), dtype=torch.float64, device="cuda")
            buf.view(torch.int64).fill_(int(SBITS))
            arr, axes = _tensor(torch, buf, ext, has, strides, base)
            assert hip.view_plan(field, arr, axes, for_get=True)["path"] == path, (field, label)
            torch.cuda.synchronize()
            hip.get(field, arr, axes, nt=nt, stream=stream)
            calls += 1
            if stream is not None:
                torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert _same(vm.gather(field, hip.nelemd, hip.qsize, hip.nlev, strides, host, base, True), ref), (field, label)
            untouched = np.ones(size, dtype=bool)
            untouched[(vm.offsets(field, hip.nelemd, hip.qsize, hip.nlev, strides, True) + base).reshape(-1)] = False
            assert (_bits(host)[untouched] == SBITS).all(), (field, label, "a get wrote outside its view")
            if label.startswith("p0 rows of nlev + 1"):
                assert (_bits(host[:ext[0] * (ext[2] + 1) * 16].reshape(ext[0], ext[2] + 1, 16)[:, ext[2]]) == SBITS).all()
    return calls


# ---------------------------------------------------------------------------------------------------------------------------
# contexts
def _mesh_hip(nlev, qsize, one_element=False, limiter=8):
    """a context on the ne2 mesh from cube_mesh (no oracle: any level count); one_element: the single element of rank 0 of 24"""
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.driver import partition
    from transport_se_amd.hip_mod import HipMod
    from transport_se_amd.hybvcoord import HvCoord
    if nlev == 72:
        hv = HvCoord()
    elif nlev == 64:
        hv = HvCoord(os.path.join(VC, "12k_top-64m.ascii"), os.path.join(VC, "12k_top-64i.ascii"))
    else:
        from nlev80_common import hv80
        hv = hv80()
    topo = cm.topology(2); geo = cm.geometry(2, topo)
    d = cm.edge_descriptors(topo, partition(2, 24 if one_element else 1), 0)
    mine = d["elems"]
    elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    hip = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, 1e19, device=0, limiter_option=limiter,
                 schedule=dict(send=d["send"], recv=d["recv"]))
    assert hip.nlev == nlev and hip.nelemd == (1 if one_element else 24)
    return hip


def _oracle_hip(qsize=3, limiter=8, dcmip=True):
    import pyoracle as po
    from gpu_common import elem_from_oracle, make_hip
    o = po.Oracle(2, qsize, nu_q=1e19)
    elem = elem_from_oracle(o)
    hip = make_hip(o, elem, limiter_option=limiter)
    if dcmip:
        hip.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm)
        hip.dcmip_set_initial()
    return o, elem, hip


def _filled(hip, seed):
    """random contents for everything a host entry can write (the get tests of the contexts without a prescribed case)"""
    rng = np.random.default_rng(seed)
    for nt in (1, 2):
        _host_put(hip, "qdp", _logical(rng, vm.extents("qdp", hip.nelemd, hip.qsize, hip.nlev), [True] * 5), nt)
    for field in ("eta_dot_dpdn", "omega_p", "divdp", "divdp_proj"):
        _host_put(hip, field, _logical(rng, vm.extents(field, hip.nelemd, hip.qsize, hip.nlev), vm.has_axes(field)), 1)


@pytest.fixture(scope="module")
def ctx():
    o, elem, hip = _oracle_hip()
    yield o, hip
    hip.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------------------
def test_put_equals_the_host_route(ctx):
    """1: every put field, every layout, ne2 x 3 tracers; and a context of one element and one tracer"""
    o, hip = ctx
    assert check_put(hip, vm.PUT_FIELDS) == 6 * len(vm.PUT_FIELDS)
    one = _mesh_hip(72, 1, one_element=True)
    check_put(one, ("qdp", "vn0", "eta_dot_dpdn"), seed=2)
    one.close()


def test_get_equals_the_host_route(ctx):
    """2: every get field after a remap cycle of the prescribed case (dp3d, ps_v, Q and lnps hold real data); q / lnps are refused as
    stale until tse_state_q and again after a put("qdp")"""
    import torch
    from transport_se_amd.hip_mod import TseError
    o, hip = ctx
    hip.dcmip_set_initial()
    assert hip.prim_run_subcycle(1800.0, 1, 0) == 3
    n, qs = hip.nelemd, hip.qsize
    qt = torch.zeros((n, qs, 72, 4, 4), dtype=torch.float64, device="cuda"); lt = torch.zeros((n, 4, 4), dtype=torch.float64, device="cuda")
    for field, arr, axes in (("q", qt, "eqkji"), ("lnps", lt, "eji")):
        with pytest.raises(TseError, match="stale"):
            hip.get(field, arr, axes)
    hip.state_q(2)
    refs = host_get_refs(hip, vm.GET_FIELDS, 2)
    assert sorted(refs) == sorted(vm.GET_FIELDS) and all(np.abs(refs[f]).max() > 0 for f in ("qdp", "q", "lnps", "dp3d", "ps_v", "eta_dot_dpdn"))
    check_get(hip, refs, 2)
    hip.put("qdp", qt, "eqkji", nt=1)
    for field, arr, axes in (("q", qt, "eqkji"), ("lnps", lt, "eji")):
        with pytest.raises(TseError, match="stale"):
            hip.get(field, arr, axes)
    one = _mesh_hip(72, 1, one_element=True)
    _filled(one, 3)
    check_get(one, host_get_refs(one, ("qdp", "eta_dot_dpdn", "omega_p"), 1), 1)
    one.close()


def _inputs(o, nstep, dt):
    o.dcmip_step_inputs(1, nstep, dt)
    return dict(vn0=o.vn0.transpose(0, 2, 1, 3, 4).copy(), dp=o.dp.copy(), eta_dot_dpdn=o.eta_dot_dpdn.copy(), omega_p=o.omega_p.copy())


def _level_fastest(torch, x):
    """[e](q)[k][j][i] on the host -> a device tensor with the level index fastest, and its axes"""
    t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, -3, -1))).cuda()   # [e](q)[j][i][k]
    return t, ("eqjik" if x.ndim == 5 else "ejik")


@pytest.mark.parametrize("limiter", [8, 9, 0])
def test_put_has_the_side_effects_of_the_host_entries(limiter):
    """3: a step caches the element bounds of Qdp(np1); a put of another Qdp must drop them, as tse_copy_qdp_h2d does: the next step equals
    the same step of a fresh context fed through the host entries"""
    import torch
    dt = 1800.0
    o, elem, a = _oracle_hip(limiter=limiter, dcmip=False)
    o.dcmip_init(1)
    s0 = np.moveaxis(o.qdp, 0, 1).copy()                     # [e][tl][q][k][j][i]
    k = np.arange(72)[None, None, :, None, None]
    s1 = s0[:, 0] * (1.25 + 0.2 * np.sin(0.3 * k + np.arange(3)[None, :, None, None, None]))
    in0, in1 = _inputs(o, 0, dt), _inputs(o, 1, dt)
    elem["Qdp"][...] = s0
    a.copy_qdp_h2d(elem, 1); a.copy_qdp_h2d(elem, 2)
    a.set_derived(dict(vn0=in0["vn0"].transpose(0, 2, 1, 3, 4).copy(), dp=in0["dp"], eta_dot_dpdn=in0["eta_dot_dpdn"], omega_p=in0["omega_p"]))
    a.advec_tracers_remap_rk2(dt, 1, 2)                      # leaves the bounds of Qdp(2) cached
    t1, ax = _level_fastest(torch, s1)
    a.put("qdp", t1, ax, nt=1); a.put("qdp", t1, ax, nt=2)
    for name, x in in1.items():
        t, ax1 = _level_fastest(torch, x)
        a.put(name, t, ax1)
    a.advec_tracers_remap_rk2(dt, 2, 1)
    got = dict(qdp=a.fetch("qdp1", s1.shape), eta=a.fetch("eta_dot_dpdn", (24, 73, 4, 4)), omega_p=a.fetch("omega_p", (24, 72, 4, 4)),
               divdp_proj=a.fetch("divdp_proj", (24, 72, 4, 4)))
    a.close()
    from gpu_common import make_hip
    b = make_hip(o, elem, limiter_option=limiter)
    elem["Qdp"][:, 0] = s1; elem["Qdp"][:, 1] = s1
    b.copy_qdp_h2d(elem, 1); b.copy_qdp_h2d(elem, 2)
    b.set_derived(dict(vn0=in1["vn0"].transpose(0, 2, 1, 3, 4).copy(), dp=in1["dp"], eta_dot_dpdn=in1["eta_dot_dpdn"], omega_p=in1["omega_p"]))
    b.advec_tracers_remap_rk2(dt, 2, 1)
    ref = dict(qdp=b.fetch("qdp1", s1.shape), eta=b.fetch("eta_dot_dpdn", (24, 73, 4, 4)), omega_p=b.fetch("omega_p", (24, 72, 4, 4)),
               divdp_proj=b.fetch("divdp_proj", (24, 72, 4, 4)))
    b.close(); o.close()
    assert np.isfinite(ref["qdp"]).all() and not _same(ref["qdp"], s1)
    for key in ref:
        assert _same(got[key], ref[key]), (limiter, key)


def test_put_dp_clears_the_static_inputs_flag(ctx):
    """3: after put("dp") the next tse_dcmip_step_inputs writes the prescribed dp again (tse_set_derived's rule)"""
    import torch
    o, hip = ctx
    hip.dcmip_set_initial()
    hip.dcmip_step_inputs(0, 1800.0)
    ref = hip.fetch("dp", (24, 72, 4, 4))
    junk = torch.full((24, 72, 4, 4), 12345.0, dtype=torch.float64, device="cuda")
    hip.put("dp", junk, "ekji")
    assert (hip.fetch("dp", (24, 72, 4, 4)) == 12345.0).all()
    hip.dcmip_step_inputs(1, 1800.0)
    assert _same(hip.fetch("dp", (24, 72, 4, 4)), ref)


def test_a_gpu_resident_remap_cycle():
    """4: rsplit = 3 steps and the remap with every input through put and every output through get, level-fastest tensors, a non-default
    stream, no host synchronisation between the calls: equal to the host-route run"""
    import torch
    dt = 1800.0
    o, elem, b = _oracle_hip(dcmip=False)
    o.dcmip_init(1)
    s0 = np.moveaxis(o.qdp, 0, 1).copy()
    steps = [_inputs(o, nstep, dt) for nstep in range(3)]
    # the host route
    elem["Qdp"][...] = s0
    b.copy_qdp_h2d(elem, 1); b.copy_qdp_h2d(elem, 2)
    for nstep, inp in enumerate(steps):
        b.set_derived(dict(vn0=inp["vn0"].transpose(0, 2, 1, 3, 4).copy(), dp=inp["dp"], eta_dot_dpdn=inp["eta_dot_dpdn"], omega_p=inp["omega_p"]))
        n0 = 1 if nstep % 2 == 0 else 2
        b.advec_tracers_remap_rk2(dt, n0, 3 - n0)
    b.vertical_remap(3 * dt, 2)
    ref = host_get_refs(b, ("qdp", "dp3d", "ps_v", "divdp_proj", "eta_dot_dpdn", "omega_p"), 2)
    b.close()
    # the same cycle of a GPU-resident host
    from gpu_common import make_hip
    a = make_hip(o, elem)
    q1, qax = _level_fastest(torch, s0[:, 0]); q2, _ = _level_fastest(torch, s0[:, 1])
    dev = [{name: _level_fastest(torch, x) for name, x in inp.items()} for inp in steps]
    out = {f: torch.zeros(r.shape[:-3] + (4, 4, r.shape[-3]) if r.ndim > 3 else r.shape, dtype=torch.float64, device="cuda") for f, r in ref.items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a.put("qdp", q1, qax, nt=1, stream=s); a.put("qdp", q2, qax, nt=2, stream=s)
    for nstep in range(3):
        for name, (t, ax) in dev[nstep].items():
            a.put(name, t, ax, stream=s)
        n0 = 1 if nstep % 2 == 0 else 2
        a.advec_tracers_remap_rk2(dt, n0, 3 - n0)
    a.vertical_remap(3 * dt, 2)
    for f, t in out.items():
        a.get(f, t, {5: "eqjik", 4: "ejik", 3: "eji"}[t.dim()], nt=2, stream=s)
    s.synchronize()
    for f, t in out.items():
        got = t.cpu().numpy()
        got = np.moveaxis(got, -1, -3) if got.ndim > 3 else got
        assert _same(np.ascontiguousarray(got), ref[f]), f
    assert all(np.abs(ref[f]).max() > 0 for f in ("qdp", "dp3d", "ps_v"))
    a.close(); o.close()


def test_stream_contract(ctx):
    """5: the source is produced on a side stream right before the put and overwritten on it right after; a get and its consumer follow on
    the same stream; one synchronise at the end.  And a stream that is being captured is refused."""
    import torch
    from transport_se_amd.hip_mod import TseError
    o, hip = ctx
    n, qs = hip.nelemd, hip.qsize
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, qs, 4, 4, 72))
    expect = x.copy()
    for _ in range(5):
        expect = expect * 2.0; expect = expect + 1.0

    def run(stream):
        pinned = torch.from_numpy(x.copy()).pin_memory()
        src = torch.zeros((n, qs, 4, 4, 72), dtype=torch.float64, device="cuda")
        dst = torch.zeros((n, qs, 72, 4, 4), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            src.copy_(pinned, non_blocking=True)
            for _ in range(5):
                src.mul_(2.0); src.add_(1.0)
            if stream is None:
                torch.cuda.synchronize()
            hip.put("qdp", src, "eqjik", nt=1, stream=stream)
            src.zero_()                                  # the caller reuses its source at once
            hip.get("qdp", dst, "eqkji", nt=1, stream=stream)
            out = dst.clone()
        torch.cuda.synchronize()
        return out.cpu().numpy()
    side = run(torch.cuda.Stream())
    sync = run(None)
    want = np.ascontiguousarray(np.moveaxis(expect, -1, -3))
    assert _same(sync, want) and _same(side, sync)

    s = torch.cuda.Stream()
    t = torch.zeros((n, qs, 72, 4, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    before = hip.fetch("qdp1", (n, qs, 72, 4, 4))
    with view_common.capturing(s):
        for call in (hip.put, hip.get):
            with pytest.raises(TseError, match="captured"):
                call("qdp", t, "eqkji", nt=1, stream=s)
    assert _same(hip.fetch("qdp1", (n, qs, 72, 4, 4)), before) and not t.any().item()


# ---- 6: the libraries built for 64 and 80 levels, each in a child process -------------------------------------------------------
def _worker(spec):
    nlev = spec["nlev"]
    fields = ("qdp", "omega_p", "eta_dot_dpdn")
    hip = _mesh_hip(nlev, 3)
    assert hip.L.tse_nlev() == nlev
    assert check_put(hip, fields) == 18
    _filled(hip, 7)
    assert check_get(hip, host_get_refs(hip, fields, 2), 2) == 19
    hip.close()
    print("views at %d levels: ok" % nlev)


@pytest.mark.parametrize("nlev", [64, 80])
def test_views_at_other_level_counts(nlev):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(dict(nlev=nlev))], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert res.returncode == 0 and b"levels: ok" in res.stdout, res.stdout.decode()[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    """7: every refused call leaves the launch count of the "view" group and the library's fields as they were"""
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    o, hip = ctx
    n, qs = hip.nelemd, hip.qsize
    hip.timing(True)
    t = torch.zeros((n, qs, 72, 4, 4), dtype=torch.float64, device="cuda")
    lev = torch.zeros((n, 72, 4, 4), dtype=torch.float64, device="cuda")
    hip.put("qdp", t, "eqkji", nt=1); hip.get("qdp", t, "eqkji", nt=1)
    assert hip.kernel_time("view")[1] == 2
    before = [hip.fetch("qdp1", t.shape), hip.fetch("dp", lev.shape)]
    dense = [qs * 1152, 1152, 16, 4, 1]
    host = np.zeros(t.shape)
    cases = [
        ("device", lambda: hip.put("qdp", _Fake(t.shape, dense, host.ctypes.data), "eqkji", nt=1)),            # a numpy array's address
        ("device", lambda: hip.get("qdp", _Fake(t.shape, dense, host.ctypes.data), "eqkji", nt=1)),
        ("outside its allocation", lambda: hip.put("qdp", _Fake(t.shape, [1 << 40] + dense[1:], t.data_ptr()), "eqkji", nt=1)),
        ("outside its allocation", lambda: hip.get("qdp", _Fake(t.shape, [1 << 40] + dense[1:], t.data_ptr()), "eqkji", nt=1)),
        ("overlap", lambda: hip.get("qdp", _Fake(t.shape, [1152, 1152, 16, 4, 1], t.data_ptr()), "eqkji", nt=1)),   # elements on top of tracers
        ("overlap", lambda: hip.get("dp3d", _Fake(lev.shape, [1152, 16, 4, 2], lev.data_ptr()), "ekji")),
        ("cannot be written", lambda: hip.put("dp3d", lev, "ekji")),
        ("cannot be written", lambda: hip.put("q", t, "eqkji")),
        ("cannot be read", lambda: hip.get("vn0", torch.zeros((n, 2, 72, 4, 4), dtype=torch.float64, device="cuda"), "eqkji")),
        ("nt=3", lambda: hip.put("qdp", t, "eqkji", nt=3)),
        ("nt=3", lambda: hip.get("qdp", t, "eqkji", nt=3)),
        ("nt=0", lambda: hip.put("qdp", t, "eqkji")),
    ]
    for text, call in cases:
        with pytest.raises(TseError, match=text):
            call()
    # the library itself (not only the Python builder) refuses the wrong direction, a null view and a null pointer
    v = _lib.View(t.data_ptr(), (C.c_longlong * 5)(*dense))
    lv = _lib.View(lev.data_ptr(), (C.c_longlong * 5)(1152, 0, 16, 4, 1))
    L = hip.L
    assert L.tse_view_put(hip.h, b"dp3d", 1, C.byref(lv), None) != 0 and b"cannot be written" in L.tse_last_error()
    assert L.tse_view_put(hip.h, b"q", 1, C.byref(v), None) != 0 and b"cannot be written" in L.tse_last_error()
    assert L.tse_view_get(hip.h, b"vn0", 1, C.byref(v), None) != 0 and b"cannot be read" in L.tse_last_error()
    assert L.tse_view_put(hip.h, b"dp", 1, None, None) != 0 and b"null" in L.tse_last_error()
    assert L.tse_view_get(hip.h, b"dp3d", 1, None, None) != 0 and b"null" in L.tse_last_error()
    null = _lib.View(None, (C.c_longlong * 5)(1152, 0, 16, 4, 1))
    assert L.tse_view_put(hip.h, b"dp", 1, C.byref(null), None) != 0 and b"null" in L.tse_last_error()
    assert hip.kernel_time("view")[1] == 2
    assert _same(hip.fetch("qdp1", t.shape), before[0]) and _same(hip.fetch("dp", lev.shape), before[1])
    hip.timing(False)
    assert check_put(hip, vm.PUT_FIELDS, seed=11) == 6 * len(vm.PUT_FIELDS)   # the context still passes test 1


def test_view_timer_group(ctx):
    """8: the "view" group counts one launch per put / get; the existing groups read what they read without views"""
    o, hip = ctx
    hip.dcmip_set_initial()
    hip.timing(True)
    hip.dcmip_step_inputs(0, 1800.0); hip.advec_tracers_remap_rk2(1800.0, 1, 2)
    groups = ("advance", "dss", "lap", "minmax", "remap", "level", "dcmip", "avg", "stateq")
    base = {g: hip.kernel_time(g)[1] for g in groups}
    assert base["advance"] > 0 and hip.kernel_time("view") == (0.0, 0)
    hip.timing(True)
    calls = check_put(hip, vm.PUT_FIELDS, seed=8)
    hip.state_q(2)
    calls += check_get(hip, host_get_refs(hip, ("qdp", "q", "lnps", "omega_p", "eta_dot_dpdn"), 2), 2)
    ms, n = hip.kernel_time("view")
    assert n == calls and ms > 0
    assert all(hip.kernel_time(g)[1] == (1 if g == "stateq" else 0) for g in groups)
    hip.dcmip_set_initial()
    hip.timing(True)
    hip.dcmip_step_inputs(0, 1800.0); hip.advec_tracers_remap_rk2(1800.0, 1, 2)
    assert {g: hip.kernel_time(g)[1] for g in groups} == base and hip.kernel_time("view")[1] == 0
    hip.timing(False)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    _worker(json.loads(sys.argv[2]))
