"""-m gpu: tracer forcing on the device from a host's strided view (tse_apply_forcing / tse_apply_forcing_host; HipMod.apply_forcing,
PrimRun.apply_forcing).

The rule and the budget are restated operation for operation in tests/forcing_model.py, so every comparison here is bit for bit: against
that model on the fields of its generator (every branch of the clip, signed zeros, landings one ulp either side of zero), on every path and
layout of the FQ view, at 72, 64 and 80 levels; against the get / compute / put route on fields where the limiter's bounds matter; across
the copies of shared nodes, across partitions, across streams.  Device arrays are torch tensors; no view here leaves its tensor: the
refusal tests pass only views the library's checks turn down before anything is launched."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import forcing_model as fm
import view_common
import view_model as vm
from view_common import FakeArray as _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VC = os.path.join(ROOT, "tests", "golden", "vcoord")
pytestmark = pytest.mark.gpu

SBITS = np.uint64(0x7FF4DEADBEEF0001)
SENTINEL = np.array([SBITS], dtype=np.uint64).view(np.float64)[0]
MODES = {0: "tendency", 1: "adjust"}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _hv(nlev):
    from transport_se_amd.hybvcoord import HvCoord
    if nlev == 72:
        return HvCoord()
    if nlev == 64:
        return HvCoord(os.path.join(VC, "12k_top-64m.ascii"), os.path.join(VC, "12k_top-64i.ascii"))
    from nlev80_common import hv80
    return hv80()


class Ctx:
    """a context on the ne2 mesh of cube_mesh (any level count), the whole mesh or rank `rank` of `world`, with the host-side pieces the
    model needs: spheremp of its elements and the vertical coordinate"""

    def __init__(self, nlev=72, qsize=3, world=1, rank=0, limiter=8):
        from transport_se_amd import cube_mesh as cm
        from transport_se_amd.driver import partition
        from transport_se_amd.hip_mod import HipMod
        hv = _hv(nlev)
        topo = cm.topology(2); geo = cm.geometry(2, topo)
        d = cm.edge_descriptors(topo, partition(2, world), rank)
        self.mine = mine = d["elems"]
        elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                    rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
        self.hip = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, 1e19, device=0, limiter_option=limiter,
                          schedule=dict(send=d["send"], recv=d["recv"]))
        self.hv = (hv.hyai, hv.hybi, hv.ps0)
        self.spheremp = np.ascontiguousarray(geo["spheremp"][mine])
        self.n, self.qs, self.nlev = len(mine), qsize, nlev
        assert self.hip.nlev == nlev
        self._rt = C.CDLL("libamdhip64.so")

    def poke(self, name, x):
        """host array -> an internal field that no entry uploads on its own (ps_v)"""
        p, nbytes = self.hip.device_ptr(name)
        x = np.ascontiguousarray(x, np.float64)
        assert x.nbytes == nbytes, (name, x.nbytes, nbytes)
        self.hip.synchronize()
        assert self._rt.hipMemcpy(C.c_void_p(p), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), C.c_int(1)) == 0

    def load(self, lev1, lev2, ps_v=None):
        self.hip.copy_qdp_h2d(dict(Qdp=np.ascontiguousarray(np.stack([lev1, lev2], axis=1))), 1)
        self.hip.copy_qdp_h2d(dict(Qdp=np.ascontiguousarray(np.stack([lev1, lev2], axis=1))), 2)
        if ps_v is not None:
            self.poke("ps_v", ps_v)

    def qdp(self, nt):
        return self.hip.fetch("qdp%d" % nt, (self.n, self.qs, self.nlev, 4, 4))

    def close(self):
        self.hip.close()


def device_view(torch, fq, strides, size, base):
    """FQ laid into a sentinel-filled device buffer as the view names it -> (the view, the buffer, its host image)"""
    n, qs, nlev = fq.shape[:3]
    host = vm.scatter("qdp", fq, n, qs, nlev, strides, np.full(size, SENTINEL), base)
    buf = torch.from_numpy(host).cuda()
    return _Fake(fq.shape, strides, buf.data_ptr() + 8 * base), buf, host


class Case:
    """the generator's fields of one mode on one context's shape, and what the model makes of them (computed once per set of broadcast axes)"""

    def __init__(self, ctx, mode, elems=None, n_all=None):
        self.mode = mode
        qdp, fq, ps_v, self.dt = fm.forcing_fields(n_all or ctx.n, ctx.qs, ctx.nlev, mode=mode, hv=ctx.hv)
        pick = slice(None) if elems is None else elems
        self.qdp, self.fq, self.ps_v = qdp[pick], fq[pick], ps_v[pick]
        self.other = np.random.default_rng(3).standard_normal(self.qdp.shape)
        self.dp = fm.level_dp(ctx.hv[0], ctx.hv[1], ctx.hv[2], self.ps_v)
        self.w = ctx.spheremp
        self._res = {}

    def expect(self, const=()):
        if const not in self._res:
            fq = fm.broadcast_along(self.fq, const)
            res = fm.apply(self.qdp, fq, self.dt, self.mode, self.dp)
            self._res[const] = (fq, res["new"], fm.budget(self.w, res))
        return self._res[const]


def check_bits(ctx, rows=None, stream=None):
    """test 1 on one context: both modes, every layout, nt alternating; returns the number of calls"""
    import torch
    hip, calls = ctx.hip, 0
    all_rows = fm.layouts(ctx.n, ctx.qs, ctx.nlev)
    for mode in (0, 1):
        case = Case(ctx, mode)
        for t, (label, strides, size, base, path, const) in enumerate(all_rows):
            if rows is not None and t not in rows:
                continue
            nt = 1 + t % 2
            fq, new, bud = case.expect(const)
            view, buf, host = device_view(torch, fq, strides, size, base)
            assert hip.view_plan("qdp", view, "eqkji")["path"] == path, label
            for with_budget in (True, False):
                lev = [case.other, case.other]; lev[nt - 1] = case.qdp
                ctx.load(lev[0], lev[1], case.ps_v)
                torch.cuda.synchronize()
                got = hip.apply_forcing(view, "eqkji", nt, dt=case.dt, mode=MODES[mode], stream=stream, budget=with_budget)
                calls += 1
                if stream is not None:
                    torch.cuda.synchronize()
                tag = (ctx.nlev, MODES[mode], label, nt, with_budget)
                assert _same(ctx.qdp(nt), new), tag
                assert _same(ctx.qdp(3 - nt), case.other), tag + ("the other time level changed",)
                assert _same(buf.cpu().numpy(), host), tag + ("the call wrote into its view",)
                if with_budget:
                    assert _same(got, bud), tag
                else:
                    assert got is None
    return calls


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


# ---- 1: bits ---------------------------------------------------------------------------------------------------------------------
def test_bits_on_every_layout(ctx):
    assert check_bits(ctx) == 2 * 9 * 2
    case = Case(ctx, 0)
    fq, new, bud = case.expect()
    assert not _same(new, case.qdp) and (bud[:, :, 1] < 0).all() and (new[case.qdp >= 0] >= 0).all()


def _worker(spec):
    c = Ctx(nlev=spec["nlev"])
    assert c.hip.L.tse_nlev() == spec["nlev"]
    assert check_bits(c) == 36
    c.close()
    print("forcing at %d levels: ok" % spec["nlev"])


@pytest.mark.parametrize("nlev", [64, 80])
def test_bits_at_other_level_counts(nlev):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(dict(nlev=nlev))], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert res.returncode == 0 and b"levels: ok" in res.stdout, res.stdout.decode()[-4000:]


# ---- 2: other tracer counts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qsize", [1, 4])
def test_qsize_1_and_4(qsize):
    c = Ctx(qsize=qsize)
    try:
        assert check_bits(c, rows=(0, 3, 5)) == 2 * 3 * 2      # one layout per path
    finally:
        c.close()


# ---- 3: the host variant -----------------------------------------------------------------------------------------------------------
def test_host_variant_equals_the_view_variant(ctx):
    hip = ctx.hip
    for mode in (0, 1):
        case = Case(ctx, mode)
        fq, new, bud = case.expect()
        host_fq = np.full((ctx.n, 5, ctx.nlev, 4, 4), SENTINEL)      # one time level of FQ(np,np,nlev,qsize_d = 5,timelevels)
        host_fq[:, :ctx.qs] = fq
        keep = host_fq.copy()
        ctx.load(case.other, case.qdp, case.ps_v)
        got = hip.apply_forcing_host(host_fq, 2, case.dt, MODES[mode], budget=True)
        assert _same(ctx.qdp(2), new) and _same(got, bud) and _same(ctx.qdp(1), case.other) and _same(host_fq, keep), mode
        ctx.load(case.other, case.qdp, case.ps_v)
        assert hip.apply_forcing_host(host_fq, 2, case.dt, MODES[mode]) is None and _same(ctx.qdp(2), new)
        # the staging field is the Q field: a tse_state_q that follows forms Q of the new state in it
        out = dict(Q=np.zeros((ctx.n, ctx.qs, ctx.nlev, 4, 4)), lnps=np.zeros((ctx.n, 4, 4)))
        hip.state_q(2); hip.copy_q_d2h(out); hip.copy_lnps_d2h(out)
        with np.errstate(all="ignore"):
            assert _same(out["Q"], new / case.dp[:, None]), mode


# ---- 4: side effects -----------------------------------------------------------------------------------------------------------------
def _dcmip(ctx_):
    from transport_se_amd import cube_mesh as cm
    hv = _hv(ctx_.nlev)
    geo = cm.geometry(2, cm.topology(2))
    ctx_.hip.dcmip_init(1, geo["lat"][ctx_.mine], geo["lon"][ctx_.mine], hv.hyam, hv.hybm)
    ctx_.hip.dcmip_set_initial()


def test_side_effects_are_those_of_copy_qdp_h2d(ctx):
    import torch
    from transport_se_amd.hip_mod import TseError
    hip, dt = ctx.hip, 1800.0
    shape = (ctx.n, ctx.qs, ctx.nlev, 4, 4)
    qt = torch.zeros(shape, dtype=torch.float64, device="cuda")

    def route(invalidate):
        _dcmip(ctx)
        hip.dcmip_step_inputs(0, dt); hip.advec_tracers_remap_rk2(dt, 1, 2)       # leaves the element bounds of Qdp(2) cached
        hip.state_q(2); hip.get("q", qt, "eqkji")
        hip.get("qdp", qt, "eqkji", nt=2)
        fq = -qt / (4 * dt)
        hip.apply_forcing(fq, "eqkji", 2, dt=dt)
        with pytest.raises(TseError, match="stale"):
            hip.get("q", qt, "eqkji")
        if invalidate:
            hip.invalidate_cache()
        hip.dcmip_step_inputs(1, dt); hip.advec_tracers_remap_rk2(dt, 2, 1)
        return hip.get_qminmax() + (ctx.qdp(1),)
    a, b = route(False), route(True)
    assert all(_same(x, y) for x, y in zip(a, b))
    assert np.isfinite(a[2]).all() and (a[0] <= a[1]).all()


# ---- 5: route equivalence where the bounds matter ------------------------------------------------------------------------------------
@pytest.mark.parametrize("limiter", [8, 9])
def test_equals_the_get_compute_put_route_on_the_dye_fields(limiter):
    import bounds_probe as bp
    import pyoracle as po
    import torch
    from gpu_common import elem_from_oracle, make_hip
    nu, dt = bp.PARAMS[2]
    o = po.Oracle(2, 3, nu_q=nu, rsplit=bp.RSPLIT)
    o.dcmip_init(1)
    qdp0 = bp.dye(o, qsize=3)
    elem = dict(Qdp=np.ascontiguousarray(np.stack([qdp0, qdp0], axis=1)))
    hip = make_hip(o, elem_from_oracle(o), limiter_option=limiter)
    qt = torch.zeros(qdp0.shape, dtype=torch.float64, device="cuda")

    def run(forcing):
        hip.dcmip_init(1, o.lat, o.lon, o.hyam, o.hybm); hip.dcmip_set_initial()
        hip.copy_qdp_h2d(elem, 1); hip.copy_qdp_h2d(elem, 2)
        hip.dcmip_step_inputs(0, dt); hip.advec_tracers_remap_rk2(dt, 1, 2)       # nstep = 1: the bounds of Qdp(2) are cached
        forcing()
        hip.dcmip_step_inputs(1, dt); hip.advec_tracers_remap_rk2(dt, 2, 1)       # one tracer step ...
        assert hip.prim_run_subcycle(dt, 1, 2) == 2 + bp.RSPLIT                     # ... and one full cycle (n0 = 1)
        return hip.fetch("qdp2", qdp0.shape)

    def entry():
        hip.get("qdp", qt, "eqkji", nt=2)
        hip.apply_forcing(-qt / (4 * dt), "eqkji", 2, dt=dt)

    def by_hand():
        hip.get("qdp", qt, "eqkji", nt=2)
        v = dt * (-qt / (4 * dt))
        hip.put("qdp", qt + v, "eqkji", nt=2)
    try:
        a, b, plain = run(entry), run(by_hand), run(lambda: None)
    finally:
        hip.close(); o.close()
    assert np.isfinite(a).all() and _same(a, b)
    assert not _same(a, plain)


# ---- 6: shared nodes -----------------------------------------------------------------------------------------------------------------
_shared = {}


def _shared_nodes(ctx):
    """A DCMIP 1-1 cycle, then a forcing whose FQ is a smooth function of (lat, lon, level) evaluated once per unique column and handed to
    every copy of it; and the same forcing on the state made single-valued (every copy given the bits of the node's first copy).  Returns,
    per run, the [point][q, k] bit patterns before and after, and `first` / `node` (the first copy of every column, the column of every point)."""
    if _shared:
        return _shared
    import torch
    from transport_se_amd import cube_mesh as cm
    hip, dt = ctx.hip, 1800.0
    geo = cm.geometry(2, cm.topology(2))
    lat, lon = geo["lat"].reshape(-1), geo["lon"].reshape(-1)
    xyz = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1)
    _, first, node = np.unique(np.round(xyz * 1e8).astype(np.int64), axis=0, return_index=True, return_inverse=True)
    node = node.reshape(-1)
    assert first.size == 6 * 4 * 9 + 2
    k = np.arange(ctx.nlev)[None, :]
    col = 1e-4 * (np.sin(lat[first]) * np.cos(2 * lon[first]))[:, None] * (1.0 + 0.5 * np.sin(0.2 * k)) - 2e-5      # [column][k], both signs
    fq = col[node].reshape(ctx.n, 4, 4, ctx.nlev)                                                         # [e][j][i][k]
    fq = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(fq[:, None], (ctx.n, ctx.qs, 4, 4, ctx.nlev)))).cuda()
    pts = lambda x: _bits(x.transpose(0, 3, 4, 1, 2)).reshape(ctx.n * 16, ctx.qs * ctx.nlev)   # noqa: E731
    _dcmip(ctx)
    assert hip.prim_run_subcycle(dt, 1, 0) == 3
    before = ctx.qdp(2)
    bud = hip.apply_forcing(fq, "eqjik", 2, dt=3 * dt, budget=True)
    after = ctx.qdp(2)
    assert not _same(after, before) and (bud[:, :, 1] != 0).any() and (bud[:, :, 0] != 0).all()   # the clip acted: DCMIP 1-1 has empty regions
    single = pts(before).view(np.float64)[first][node].reshape(ctx.n, 4, 4, ctx.qs, ctx.nlev).transpose(0, 3, 4, 1, 2)
    ctx.load(single, single)
    hip.apply_forcing(fq, "eqjik", 2, dt=3 * dt)
    _shared.update(first=first, node=node, before=pts(before), after=pts(after), single=pts(np.ascontiguousarray(single)), single_after=pts(ctx.qdp(2)))
    return _shared


def test_copies_of_a_shared_node_stay_equal(ctx):
    """After a DCMIP 1-1 cycle plus forcing with one FQ per unique column, all copies of every shared GLL node hold equal bits.

    The forcing is pointwise, so this can hold only where it held before the call, and the state a cycle leaves is not single-valued in
    its bits: at a corner node three or four elements add the same DSS contributions, each its own first, and the copies end an ulp
    apart (the checker's own cycle on the CPU leaves 1292 of 82944 entries unequal, relative difference <= 3.9e-15; on the device at ne2,
    3 tracers, 72 levels: 1244 entries at 67 of 384 points before the forcing, 1214 at the same 67 points after it).  That is the tracer
    step's property, not the forcing's, and no forcing could repair it.  So the post-cycle state is first made single-valued through the
    host interface (every copy takes the bits of its node's first copy) and the assertion is made on ALL copies of ALL nodes of that
    state; test_forcing_adds_no_difference_between_copies holds the call on the cycle's own state to what it can answer for there."""
    s = _shared_nodes(ctx)
    first, node = s["first"], s["node"]
    for name in ("before", "after"):
        d = s[name] != s[name][first][node]
        print("shared nodes, %s the forcing on the cycle's own state: %d of %d entries differ from their node's first copy, at %d of %d points"
              % (name, int(d.sum()), d.size, int(d.any(axis=1).sum()), d.shape[0]))
    shared = np.bincount(node) > 1
    assert int(shared.sum()) == 6 * 4 * 9 + 2 - 24 * 4                 # every node but the four interior ones of each element
    assert np.array_equal(s["single"], s["single"][first][node])      # the precondition
    assert not np.array_equal(s["single"], s["single_after"])         # the forcing did something
    assert np.array_equal(s["single_after"], s["single_after"][first][node])


def test_forcing_adds_no_difference_between_copies(ctx):
    """on the state the cycle itself leaves (copies of corner nodes an ulp apart, see above): no entry whose copies held equal bits before the
    call holds unequal bits after it, and the points with any unequal entry are the same"""
    s = _shared_nodes(ctx)
    first, node = s["first"], s["node"]
    d0 = s["before"] != s["before"][first][node]
    d1 = s["after"] != s["after"][first][node]
    assert not (d1 & ~d0).any()
    assert not (d1.any(axis=1) & ~d0.any(axis=1)).any()


# ---- 7: partition ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_partition_gives_the_bits_of_one_context(ctx, world):
    import torch
    one = {}
    for mode in (0, 1):
        whole = Case(ctx, mode)
        fq, new, bud = whole.expect()
        ctx.load(whole.qdp, whole.other, whole.ps_v)
        got = ctx.hip.apply_forcing(torch.from_numpy(fq).cuda(), "eqkji", 1, dt=whole.dt, mode=MODES[mode], budget=True)
        one[mode] = (fq, ctx.qdp(1), got)
        assert _same(one[mode][1], new) and _same(got, bud)
    seen = np.zeros(ctx.n, dtype=bool)
    for rank in range(world):
        part = Ctx(world=world, rank=rank)
        try:
            mine = part.mine
            for mode in (0, 1):
                fq, one_q, one_b = one[mode]
                case = Case(part, mode, elems=mine, n_all=ctx.n)
                part.load(case.qdp, case.other, case.ps_v)
                b = part.hip.apply_forcing(torch.from_numpy(np.ascontiguousarray(fq[mine])).cuda(), "eqkji", 1, dt=case.dt, mode=MODES[mode],
                                           budget=True)
                assert _same(part.qdp(1), one_q[mine]) and _same(b, one_b[mine]), (world, rank, mode)
            seen[mine] = True
        finally:
            part.close()
    assert seen.all() and 0 < len(mine) < ctx.n


# ---- 8: stream ordering ------------------------------------------------------------------------------------------------------------------
def test_stream_contract(ctx):
    import torch
    from transport_se_amd.hip_mod import TseError
    hip = ctx.hip
    case = Case(ctx, 0)
    fq, new, _ = case.expect()
    # FQ = ((x * 2) + 1) on the device: x chosen so that the host knows the bits
    x = (fq - 1.0) / 2.0
    made = x * 2.0 + 1.0
    res = fm.apply(case.qdp, made, case.dt, 0)
    s = torch.cuda.Stream()
    pinned = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 2, -1))).pin_memory()                   # level-fastest: the LDS path
    src = torch.zeros(pinned.shape, dtype=torch.float64, device="cuda")
    ctx.load(case.qdp, case.other)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        src.copy_(pinned, non_blocking=True)
        src.mul_(2.0); src.add_(1.0)
        assert hip.apply_forcing(src, "eqjik", 1, dt=case.dt, stream=s) is None
        src.zero_()                                          # the caller reuses its source at once
    torch.cuda.synchronize()
    assert _same(ctx.qdp(1), res["new"]) and not src.any().item()

    before = ctx.qdp(1)
    torch.cuda.synchronize()
    with view_common.capturing(s):
        with pytest.raises(TseError, match="captured"):
            hip.apply_forcing(src, "eqjik", 1, dt=case.dt, stream=s)
    assert _same(ctx.qdp(1), before)


# ---- 9: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    import torch
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import TseError
    hip = ctx.hip
    shape = (ctx.n, ctx.qs, ctx.nlev, 4, 4)
    plane = ctx.nlev * 16
    dense = [ctx.qs * plane, plane, 16, 4, 1]
    case = Case(ctx, 0)
    ctx.load(case.qdp, case.qdp)
    t = torch.zeros(shape, dtype=torch.float64, device="cuda")
    hip.timing(True)
    hip.apply_forcing(t, "eqkji", 1, dt=1.0)
    assert hip.kernel_time("forcing")[1] == 1 and hip.kernel_time("view")[1] == 0
    before = [ctx.qdp(1), ctx.qdp(2)]
    host = np.zeros(shape)
    q1, _ = hip.device_ptr("qdp1")
    cases = [
        ("mode=7", lambda: hip.apply_forcing(t, "eqkji", 1, dt=1.0, mode=7)),
        ("mode=-1", lambda: hip.apply_forcing(t, "eqkji", 1, dt=1.0, mode=-1)),
        ("unknown mode", lambda: hip.apply_forcing(t, "eqkji", 1, dt=1.0, mode="relax")),
        ("nt=0", lambda: hip.apply_forcing(t, "eqkji", 0, dt=1.0)),
        ("nt=3", lambda: hip.apply_forcing(t, "eqkji", 3, dt=1.0)),
        ("not finite", lambda: hip.apply_forcing(t, "eqkji", 1, dt=float("inf"))),
        ("not finite", lambda: hip.apply_forcing(t, "eqkji", 1, dt=float("nan"), mode="adjust")),
        ("device", lambda: hip.apply_forcing(_Fake(shape, dense, host.ctypes.data), "eqkji", 1, dt=1.0)),
        ("outside its allocation", lambda: hip.apply_forcing(_Fake(shape, [1 << 40] + dense[1:], t.data_ptr()), "eqkji", 1, dt=1.0)),
        ("overlaps Qdp", lambda: hip.apply_forcing(_Fake(shape, dense, q1), "eqkji", 1, dt=1.0)),
        ("overlaps Qdp", lambda: hip.apply_forcing(_Fake(shape, [0] + dense[1:], q1 + 8 * (ctx.n - 1) * dense[0]), "eqkji", 1, dt=1.0)),
        ("nt=3", lambda: hip.apply_forcing_host(host, 3, 1.0, "tendency")),
        ("mode=2", lambda: hip.apply_forcing_host(host, 1, 1.0, 2)),
        ("not finite", lambda: hip.apply_forcing_host(host, 1, float("-inf"), "tendency")),
        ("qsize_d=2", lambda: hip.apply_forcing_host(np.zeros((ctx.n, 2, ctx.nlev, 4, 4)), 1, 1.0, "tendency")),
    ]
    for text, call in cases:
        with pytest.raises(TseError, match=text):
            call()
    # the library itself refuses a null view and a null pointer
    L = hip.L
    assert L.tse_apply_forcing(hip.h, 1, 1.0, 0, None, None, None) != 0 and b"null" in L.tse_last_error()
    null = _lib.View(None, (C.c_longlong * 5)(*dense))
    assert L.tse_apply_forcing(hip.h, 1, 1.0, 0, C.byref(null), None, None) != 0 and b"null" in L.tse_last_error()
    assert L.tse_apply_forcing_host(hip.h, 1, 1.0, 0, None, 8 * dense[0], ctx.qs, None) != 0 and b"null" in L.tse_last_error()
    assert hip.kernel_time("forcing")[1] == 1 and hip.kernel_time("view")[1] == 0
    assert _same(ctx.qdp(1), before[0]) and _same(ctx.qdp(2), before[1])
    # a view of the OTHER time level is no overlap, and the group counts every launch of both entries
    q2, _ = hip.device_ptr("qdp2")
    hip.apply_forcing(_Fake(shape, dense, q2), "eqkji", 1, dt=0.0)
    hip.apply_forcing_host(host, 1, 1.0, "tendency")
    assert hip.kernel_time("forcing")[1] == 3 and _same(ctx.qdp(1), before[0])
    hip.timing(False)


# ---- 10: the driver ------------------------------------------------------------------------------------------------------------------------
def test_primrun_apply_forcing_picks_the_level():
    import torch
    from transport_se_amd.driver import PrimRun

    def run(explicit):
        r = PrimRun(2, 3, rsplit=3)
        shape = (r.mine.size, 3, r.nlev, 4, 4)
        qt = torch.zeros(shape, dtype=torch.float64, device="cuda")
        dtp = r.rsplit * r.tstep
        out = []
        try:
            for cyc, level in ((1, 2), (2, 1)):
                np1 = r.run(3)
                assert np1 == level and r.nstep == 3 * cyc
                r.hip.get("qdp", qt, "eqkji", nt=level)
                fq = -qt / (4 * dtp)
                if explicit:
                    b = r.hip.apply_forcing(fq, "eqkji", level, dt=dtp, mode="tendency", budget=True)
                else:
                    b = r.apply_forcing(fq, budget=True)
                out += [b, r.fetch_qdp(1), r.fetch_qdp(2)]
        finally:
            r.close()
        return out
    a, b = run(False), run(True)
    assert len(a) == 6 and all(_same(x, y) for x, y in zip(a, b))
    assert (a[0][:, :, 0] <= 0).all() and (a[0][:, :, 0] < 0).any() and not _same(a[1], a[4])


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    _worker(json.loads(sys.argv[2]))
