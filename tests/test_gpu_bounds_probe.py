"""-m gpu: the limiter's neighbour bounds on every element, side and route, on the dye fields of tests/bounds_probe.py.

test_bounds_probe_cpu.py proves that on these fields (ne2, ne3, ne4, ne5; the constants of bounds_probe.py) every (element, direction)
has witness slabs -- slabs where that neighbour alone holds the bound and the limiter clips against it by >= 1e-3 of the field -- in
stage 1 and 3 of the first step, every element in stage 2, and stage 1 of a step that starts from cached bounds (after a step, after
a remap), and that a dropped neighbour then moves the result by >= 1e6 x Q_TOL.  Here the fields go through every route:

a. the bounds themselves, bit for bit: tse_euler_step(rhs_multiplier 0) with vn0 = 0 (the limiter relaxes nothing), then
   tse_get_qminmax == min / max over {e} u nbr_elem[e] of the element extremes of Qdp * (1/dp) (k_qminmax's IEEE operations), on one
   context (ne2, ne3, ne5) and per rank on ne4 / 3 ranks and ne5 / 4 ranks (k_pack_minmax, k_unpack_minmax, remote and corner-only
   remote neighbours), limiters 8 and 9;
b. the whole step against the checker (limiter 8: the C checker; limiter 9: the Python model, ne2 and ne3): one step and a second one
   that starts from cached bounds at Q_TOL; one prim_run_subcycle cycle (RSPLIT = 1 tracer step, then the remap) and a step after
   it at Q_TOL_CYCLES, fused and with TSE_REMAP_FUSED=0; also with TSE_DSS_ON_READ=0.  The winds are the device's DCMIP 1-1 fields;
c. cached against recomputed, bit for bit: step; step == step; tse_invalidate_cache; step and cycle; step == cycle;
   tse_invalidate_cache; step, on one context and on 3 emulated ranks (where the prefetched halo is dropped too), limiters 8 and 9;
d. ranks and tilings: ne4 on 2 and 3 ranks, ne5 on 4, also with TSE_BOUNDARY_STRIPS=1, give the bits of one context after every step
   and cycle of (b)'s two sequences; that context is held to the checker step by step (the step after the cycle from the device's own
   cycle state, at Q_TOL: from the checker's cycle state ne4 measures 8.6e-13, the cycle's error carried through a step that
   multiplies a perturbation of its input 12 to 20 times);
e. the 64- and 80-level libraries at ne2 (child processes: one library per process): (c) as it stands; (b) for the two steps and
   for the step after the cycle (from the device's own cycle state, as in (d)), all at Q_TOL -- the checker has 72 levels, and a
   tracer step treats every level alone, so it steps 72-level windows of the grid (80: levels 0-71 and 8-79; 64: eight made-up
   levels on top of the 64).  The remap couples the column, so the checker cannot stand in for it there: the cycle's remap is held to
   tests/remap_ld.py (longdouble, its pointwise bound on every safe output, column mass; as test_gpu_nlev80.py holds
   tse_vertical_remap) from the Qdp the tracer step left, on the layers and the surface pressure the launch stored.

Measured (MI355X): see DESIGN.md section 5; every error is recorded with conftest.record_margin."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
Q_TOL, Q_TOL_CYCLES = 1e-13, 5e-13        # the project's allowances per step and per remap cycle (test_gpu_tracer_invariance.py)
STATE = ("qdp", "vn0", "dp", "divdp", "divdp_proj", "eta_dot_dpdn", "omega_p", "dp3d", "ps_v")
PLANS = dict(steps=("step", "step"), steps_recomputed=("step", "invalidate", "step"),
             cycle=("cycle", "step"), cycle_recomputed=("cycle", "invalidate", "step"))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _fields(ne):
    """dye Qdp [e][q][k][j][i], the prescribed dp and the checker's neighbour table at ne"""
    import bounds_probe as bp
    import pyoracle as po
    o = po.Oracle(ne, bp.QSIZE)
    try:
        o.dcmip_init(1); o.dcmip_step_inputs(1, 0, bp.PARAMS[ne][1])
        return dict(qdp=bp.dye(o), dp=o.dp.copy(), nbr=np.array(o.nbr_elem))
    finally:
        o.close()


@functools.lru_cache(maxsize=None)
def _expected(ne, limiter):
    """the checker's (limiter 9: the model's) Qdp and the dp of q_err after: one step, two steps, one cycle, one cycle and a step"""
    import bounds_probe as bp
    import limiter9_model as l9
    import pyoracle as po
    import unlimited_model as um
    from tracer_fields import layer_dp
    assert bp.RSPLIT == 1
    nu, dt = bp.PARAMS[ne]
    o = po.Oracle(ne, bp.QSIZE, nu_q=nu, rsplit=bp.RSPLIT, threads=8)
    lim = l9.Limiter9(o) if limiter == 9 else None
    try:
        def step(nstep):
            o.dcmip_step_inputs(1, nstep, dt)
            if lim is None:
                o.advec_tracers_remap_rk2(dt, nstep)
            else:
                um.advec_tracers_remap_rk2(o, dt, nstep, lim)
            return o.qdp[um.qdp_levels(nstep)[1] - 1].copy(), o.dp - dt * o.divdp_proj
        o.dcmip_init(1)
        o.qdp[0] = _fields(ne)["qdp"]; o.qdp[1] = o.qdp[0]
        out = {}
        out["step1"] = step(0)
        keep = {k: getattr(o, k).copy() for k in STATE}
        out["step2"] = step(1)
        for k in STATE:
            getattr(o, k)[...] = keep[k]
        assert o.vertical_remap(dt * bp.RSPLIT, 2) == 0
        out["cycle"] = (o.qdp[1].copy(), layer_dp(o.hyai, o.hybi, o.ps_v))
        out["cycle_step"] = step(1)
        return out
    finally:
        o.close()


def _step_after(ne, qdp_cycle):
    """the checker's tracer step (limiter 8) from a given state after the cycle: a single step from the device's own inputs, so the
    per-step allowance applies.  (From the checker's own post-cycle state the comparison also carries the cycle's error through the
    step; on these fields the checker's step multiplies a 1e-13 perturbation of its input by 12 to 20 at the worst point.)"""
    import bounds_probe as bp
    import pyoracle as po
    nu, dt = bp.PARAMS[ne]
    o = po.Oracle(ne, bp.QSIZE, nu_q=nu, rsplit=bp.RSPLIT, threads=8)
    try:
        o.dcmip_init(1)
        o.qdp[0] = qdp_cycle; o.qdp[1] = qdp_cycle
        o.dcmip_step_inputs(1, bp.RSPLIT, dt); o.advec_tracers_remap_rk2(dt, bp.RSPLIT)
        return o.qdp[0].copy(), o.dp - dt * o.divdp_proj
    finally:
        o.close()


class Drive:
    """the calls of a plan on one context (a whole mesh or a rank's share): start() loads the dye state over the DCMIP 1-1 set-up"""

    def __init__(self, hip, qdp0, dt, lat, lon, hyam, hybm):
        self.hip, self.dt, self.geo = hip, dt, (lat, lon, hyam, hybm)
        self.elem = dict(Qdp=np.ascontiguousarray(np.stack([qdp0, qdp0], axis=1)))
        self.shape = (2,) + qdp0.shape

    def start(self):
        h = self.hip
        h.dcmip_init(1, *self.geo); h.dcmip_set_initial()
        h.copy_qdp_h2d(self.elem, 1); h.copy_qdp_h2d(self.elem, 2)
        self.nstep, self.last = 0, 1

    def step(self):
        n0 = 1 if self.nstep % 2 == 0 else 2
        self.hip.dcmip_step_inputs(self.nstep, self.dt)
        self.hip.advec_tracers_remap_rk2(self.dt, n0, 3 - n0)
        self.nstep += 1; self.last = 3 - n0

    def cycle(self):
        import bounds_probe as bp
        n = self.hip.prim_run_subcycle(self.dt, 1, self.nstep)
        assert n == self.nstep + bp.RSPLIT
        self.nstep = n; self.last = 2 if (n - 1) % 2 == 0 else 1

    def invalidate(self):
        self.hip.invalidate_cache()

    def qdp(self):
        return self.hip.fetch("qdp", self.shape)[self.last - 1].copy()

    def run(self, plan, snapshots=False):
        """-> Qdp after the plan (snapshots: after every step / cycle of it)"""
        self.start()
        out = []
        for op in plan:
            getattr(self, op)()
            if snapshots and op != "invalidate":
                out.append(self.qdp())
        return out if snapshots else self.qdp()


class One:
    """one context on the checker's geometry"""

    def __init__(self, ne, limiter):
        import bounds_probe as bp
        import pyoracle as po
        from gpu_common import elem_from_oracle, make_hip
        nu, dt = bp.PARAMS[ne]
        self.o = po.Oracle(ne, bp.QSIZE, nu_q=nu, rsplit=bp.RSPLIT)
        self.hip = make_hip(self.o, elem_from_oracle(self.o), limiter_option=limiter)
        self.drive = Drive(self.hip, _fields(ne)["qdp"], dt, self.o.lat, self.o.lon, self.o.hyam, self.o.hybm)

    def close(self):
        self.hip.close(); self.o.close()


def _check(name, got, ref, tol):
    from conftest import record_margin
    from tracer_fields import q_err
    err, (q, k, e) = q_err(got, ref[0], ref[1])
    for i, x in enumerate(err):
        record_margin("q_err bounds probe %s tracer %d" % (name, i), x, tol)
    print("bounds probe %s: q_err %s" % (name, ["%.2e" % x for x in err]))
    assert np.all(err <= tol), (name, err.tolist(), "worst: tracer %d level %d element %d" % (q, k, e))


def _against_checker(name, drive, exp, env=None, cycle_only=False, restart=None):
    import test_gpu_unlimited as gu
    with gu._env(**(env or {})):
        if not cycle_only:
            s1, s2 = drive.run(PLANS["steps"], snapshots=True)
            _check(name + " step", s1, exp["step1"], Q_TOL)
            _check(name + " second step (cached bounds)", s2, exp["step2"], Q_TOL)
        c1, c2 = drive.run(PLANS["cycle"], snapshots=True)
        _check(name + " cycle", c1, exp["cycle"], Q_TOL_CYCLES)
        _check(name + " step after the cycle (the remap's bounds)", c2, exp["cycle_step"], Q_TOL_CYCLES)
        if restart is not None:
            _check(name + " step after the cycle, from the device's cycle state", c2, _step_after(restart, c1), Q_TOL)


# ---- a. the bounds read back exactly ----
def _expected_bounds(ne):
    import bounds_probe as bp
    f = _fields(ne)
    Q = f["qdp"] * (1.0 / f["dp"])[:, None]
    return bp.nbr_extremes(f["nbr"], *bp.elem_extremes(Q))


def _read_bounds(hip, qdp0, dp, dt):
    n = qdp0.shape[0]
    elem = dict(Qdp=np.ascontiguousarray(np.stack([qdp0, qdp0], axis=1)), vn0=np.zeros((n, 72, 2, 4, 4)), dp=np.ascontiguousarray(dp),
                eta_dot_dpdn=np.zeros((n, 73, 4, 4)), omega_p=np.zeros((n, 72, 4, 4)))
    hip.copy_qdp_h2d(elem, 1); hip.copy_qdp_h2d(elem, 2)
    hip.set_derived(elem)
    hip.compute_divdp()
    hip.euler_step(2, 1, dt / 2, 3, 0)
    return hip.get_qminmax()


def _assert_bounds(name, got, want):
    for side, g, w in (("qmin", got[0], want[0]), ("qmax", got[1], want[1])):
        bad = np.argwhere(_bits(g) != _bits(w))
        assert bad.size == 0, "%s %s: %d of %d entries differ, first (e, q, k) = %s: %r != %r" % (
            name, side, len(bad), g.size, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("limiter", [8, 9])
@pytest.mark.parametrize("ne", [2, 3, 5])
def test_bounds_read_back_bit_for_bit(ne, limiter):
    import bounds_probe as bp
    c = One(ne, limiter)
    try:
        f = _fields(ne)
        got = _read_bounds(c.hip, f["qdp"], f["dp"], bp.PARAMS[ne][1])
    finally:
        c.close()
    _assert_bounds("ne%d limiter %d" % (ne, limiter), got, _expected_bounds(ne))


def _ranks(ne, world, limiter, body, **env):
    """body(hip, mine, geo, hv) -> dict of [local element]... arrays on every emulated rank; gathered by global element"""
    import bounds_probe as bp
    import test_gpu_multirank_emulated as me
    import test_gpu_unlimited as gu
    with gu._env(**env):
        res = me._run_ne(world, ne=ne, qsize=bp.QSIZE, nu_q=bp.PARAMS[ne][0], limiter_option=limiter, rsplit=bp.RSPLIT,
                         body=lambda r, h, mine, geo, hv: body(h, mine, geo, hv))
    out, seen = {}, np.zeros(6 * ne * ne, dtype=int)
    for mine, d in res:
        seen[mine] += 1
        for k, x in d.items():
            out.setdefault(k, np.zeros((6 * ne * ne,) + x.shape[1:]))[mine] = x
    assert (seen == 1).all()
    return out


@pytest.mark.parametrize("limiter", [8, 9])
@pytest.mark.parametrize("ne,world", [(4, 3), (5, 4)])
def test_bounds_read_back_bit_for_bit_on_ranks(ne, world, limiter):
    import bounds_probe as bp
    f = _fields(ne)

    def body(h, mine, geo, hv):
        mn, mx = _read_bounds(h, f["qdp"][mine], f["dp"][mine], bp.PARAMS[ne][1])
        return dict(mn=mn, mx=mx)
    got = _ranks(ne, world, limiter, body)
    _assert_bounds("ne%d on %d ranks, limiter %d" % (ne, world, limiter), (got["mn"], got["mx"]), _expected_bounds(ne))


# ---- b. the whole step against the checker ----
@pytest.mark.parametrize("ne,limiter", [(2, 8), (3, 8), (5, 8), (2, 9), (3, 9)])
def test_whole_step_and_cycle_against_the_checker(ne, limiter):
    exp = _expected(ne, limiter)
    c = One(ne, limiter)
    try:
        name = "ne%d limiter %d" % (ne, limiter)
        _against_checker(name, c.drive, exp, restart=ne if limiter == 8 else None)
        _against_checker(name + " TSE_REMAP_FUSED=0", c.drive, exp, dict(TSE_REMAP_FUSED="0"), cycle_only=True)
        if limiter == 8:
            _against_checker(name + " TSE_DSS_ON_READ=0", c.drive, exp, dict(TSE_DSS_ON_READ="0"))
    finally:
        c.close()


# ---- c. cached against recomputed ----
def _assert_cached_is_recomputed(name, res):
    for plan in ("steps", "cycle"):
        a, b = res[plan], res[plan + "_recomputed"]
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        bad = np.argwhere(_bits(a) != _bits(b))
        assert bad.size == 0, "%s %s: cached and recomputed bounds give %d different values, first (e, q, k, j, i) = %s" % (
            name, plan, len(bad), bad[0].tolist())


@pytest.mark.parametrize("ne,limiter", [(5, 8), (3, 9)])
def test_cached_bounds_are_the_recomputed_ones(ne, limiter):
    c = One(ne, limiter)
    try:
        res = {k: c.drive.run(p) for k, p in PLANS.items()}
    finally:
        c.close()
    _assert_cached_is_recomputed("ne%d limiter %d" % (ne, limiter), res)


def _plans_body(ne, plans, snapshots=False):
    """the plans on a rank -> {plan: Qdp after it}; snapshots: {plan_1, plan_2: Qdp after its first and its second step / cycle}"""
    import bounds_probe as bp
    f = _fields(ne)

    def body(h, mine, geo, hv):
        d = Drive(h, f["qdp"][mine], bp.PARAMS[ne][1], geo["lat"][mine], geo["lon"][mine], hv.hyam, hv.hybm)
        if not snapshots:
            return {k: d.run(PLANS[k]) for k in plans}
        return {"%s_%d" % (k, i + 1): x for k in plans for i, x in enumerate(d.run(PLANS[k], snapshots=True))}
    return body


@pytest.mark.parametrize("limiter", [8, 9])
def test_cached_bounds_are_the_recomputed_ones_on_three_ranks(limiter):
    res = _ranks(4, 3, limiter, _plans_body(4, tuple(PLANS)))
    _assert_cached_is_recomputed("ne4 on 3 ranks, limiter %d" % limiter, res)


# ---- d. ranks and tilings ----
@functools.lru_cache(maxsize=None)
def _one_rank(ne):
    """the two plans on one context of the emulated-rank harness (cube_mesh's geometry), every step of them held to the checker: the
    steps and the step after the cycle (from the device's cycle state) at Q_TOL, the cycle at Q_TOL_CYCLES"""
    res = _ranks(ne, 1, 8, _plans_body(ne, ("steps", "cycle"), snapshots=True))
    exp = _expected(ne, 8)
    _check("ne%d one rank, step" % ne, res["steps_1"], exp["step1"], Q_TOL)
    _check("ne%d one rank, second step" % ne, res["steps_2"], exp["step2"], Q_TOL)
    _check("ne%d one rank, cycle" % ne, res["cycle_1"], exp["cycle"], Q_TOL_CYCLES)
    _check("ne%d one rank, step after the cycle, from the device's cycle state" % ne, res["cycle_2"], _step_after(ne, res["cycle_1"]), Q_TOL)
    return res


@pytest.mark.parametrize("ne,world,strips", [(4, 2, 0), (4, 3, 0), (4, 3, 1), (5, 4, 0), (5, 4, 1)])
def test_ranks_and_tilings_give_the_bits_of_one_context(ne, world, strips):
    one = _one_rank(ne)
    got = _ranks(ne, world, 8, _plans_body(ne, ("steps", "cycle"), snapshots=True), **(dict(TSE_BOUNDARY_STRIPS="1") if strips else {}))
    assert sorted(got) == sorted(one) == ["cycle_1", "cycle_2", "steps_1", "steps_2"]
    for key in sorted(one):
        bad = np.argwhere(_bits(got[key]) != _bits(one[key]))
        assert bad.size == 0, "ne%d on %d ranks (strips %d) %s: %d values differ, first (e, q, k, j, i) = %s" % (
            ne, world, strips, key, len(bad), bad[0].tolist())


# ---- e. the other level counts (a child process per library) ----
def _windows(nlev):
    """72-level windows of an nlev-level grid for the 72-level checker: (first level of the grid in the window, first level of the
    window in the grid, levels of the window that are the grid's); nlev < 72: 72 - nlev made-up levels on top"""
    if nlev >= 72:
        return [(0, 0, 72), (0, nlev - 72, 72)]
    return [(72 - nlev, 0, nlev)]


def _window_vcoord(hv, pad, first):
    """the 73 interfaces and 72 mid-levels of a window: the grid's coefficients from level `first` on, behind `pad` made-up levels on
    top (interfaces halving eta towards the top, mid-levels the means)"""
    hyai, hybi = np.asarray(hv.hyai, dtype=np.float64), np.asarray(hv.hybi, dtype=np.float64)
    hyam, hybm = np.asarray(hv.hyam, dtype=np.float64), np.asarray(hv.hybm, dtype=np.float64)
    if pad:
        top = (hyai[0] + hybi[0]) * 0.5 ** np.arange(pad, 0, -1)
        hyai = np.concatenate([top, hyai]); hybi = np.concatenate([np.zeros(pad), hybi])
        hyam = np.concatenate([0.5 * (hyai[1:pad + 1] + hyai[:pad]), hyam]); hybm = np.concatenate([np.zeros(pad), hybm])
    return tuple(np.ascontiguousarray(x) for x in (hyai[first:first + 73], hybi[first:first + 73], hyam[first:first + 72], hybm[first:first + 72]))


def _target_grid(ps, hv):
    """the layers k_remap's phase 1 remaps to, from the ps_v it stored: dp2(k) = fma(hyai(k+1) - hyai(k), ps0, fl((hybi(k+1) - hybi(k)) *
    ps_v)), the FMA in exact rational arithmetic rounded once (as test_gpu_nlev80.vremap_grids) -> dp2[e][k][j][i]"""
    from fractions import Fraction
    hyai, hybi = np.asarray(hv.hyai, dtype=np.float64), np.asarray(hv.hybi, dtype=np.float64)
    dA, dB, ps0 = np.diff(hyai), np.diff(hybi), Fraction(float(hv.ps0))
    dp2 = np.empty((ps.shape[0], dA.size) + ps.shape[1:])
    for k in range(dA.size):
        t = dB[k] * ps
        dp2[:, k] = np.array([float(Fraction(float(dA[k])) * ps0 + Fraction(float(x))) for x in t.ravel()]).reshape(t.shape)
    return dp2


def _check_remap(name, got, qdp, dp3d, ps, hv):
    """the remap of a cycle at ne2 against tests/remap_ld.py: from the Qdp the tracer step left (qdp), on the layers the launch stored
    (dp3d = dp - dt*divdp_proj) and the target grid of its ps_v, every safe output under remap_ld's pointwise bound, the others and
    every column's mass as test_gpu_remap_pointwise._check holds them"""
    import remap_ld as rl
    import test_gpu_remap_pointwise as rp
    from conftest import record_margin
    from step_ld import has_extended_precision
    assert has_extended_precision(), np.finfo(np.longdouble)
    assert got.shape == qdp.shape and np.isfinite(got).all()
    dp2 = _target_grid(ps, hv)
    rl.check_inputs(dp3d, dp2)
    t, safe, kid = rl.remap_q_ppm(qdp, dp3d, dp2, 0)
    worst = {}
    rp._check(name, qdp.shape[1], got, qdp, t, safe, kid, worst)
    w = max(v[0] for k, v in worst.items() if k != "mass")
    record_margin("bounds probe %s, |got - v| / bound of remap_ld" % name, w, 1.0)
    record_margin("bounds probe %s, column mass / bound of remap_ld" % name, worst["mass"][0], 1.0)
    print("bounds probe %s: worst ratio to remap_ld's bound %.3g (m = %d), column mass %.3g, unsafe outputs %.3g %%"
          % (name, w, t.m, worst["mass"][0], 100.0 * (1.0 - safe.mean())))


def _nlev_job(nlev):
    """ne2, limiter 8, on the library built for nlev levels: the four plans; the two steps and the step after the cycle (from the device's
    own cycle state) against the checker's windows; what the remap of the cycle read and stored (for remap_ld)"""
    import bounds_probe as bp
    import pyoracle as po
    import vcoord_levels as vl
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.hip_mod import HipMod
    from transport_se_amd.hybvcoord import HvCoord
    ne = 2
    nu, dt = bp.PARAMS[ne]
    hv = HvCoord(*vl.paths(nlev))
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    d = cm.edge_descriptors(topo)
    n = 6 * ne * ne
    elem = dict(Dinv=geo["Dinv"], metdet=geo["metdet"], rmetdet=geo["rmetdet"], spheremp=geo["spheremp"], rspheremp=geo["rspheremp"],
                putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), bp.QSIZE, nu, limiter_option=8, rsplit=bp.RSPLIT, device=0,
               schedule=dict(send=d["send"], recv=d["recv"]))
    assert h.nlev == nlev and h.L.tse_nlev() == nlev
    h.dcmip_init(1, geo["lat"], geo["lon"], hv.hyam, hv.hybm); h.dcmip_set_initial(); h.dcmip_step_inputs(0, dt)
    Q = bp.dye_q(n, bp.QSIZE, bp.SEED, nlev)
    drive = Drive(h, Q * h.fetch("dp", (n, nlev, 4, 4))[:, None], dt, geo["lat"], geo["lon"], hv.hyam, hv.hybm)
    out = {k: drive.run(p) for k, p in PLANS.items()}
    s1, s2 = drive.run(PLANS["steps"], snapshots=True)
    out["step1"], out["step2"] = s1, s2
    drive.start(); drive.cycle()
    c1 = out["cycle1"] = drive.qdp()
    out["dp3d"], out["ps_v"] = h.fetch("dp3d", (n, nlev, 4, 4)), h.fetch("ps_v", (n, 4, 4))     # the remap's own layers and surface pressure
    drive.step()
    out["cycle2"] = drive.qdp()
    assert np.array_equal(_bits(out["cycle2"]), _bits(out["cycle"]))
    h.close()
    for w, (at, first, cnt) in enumerate(_windows(nlev)):
        o = po.Oracle(ne, bp.QSIZE, nu_q=nu, rsplit=bp.RSPLIT, threads=8, vcoord=_window_vcoord(hv, at, first))
        o.dcmip_init(1); o.dcmip_step_inputs(1, 0, dt)
        Qw = np.ones((n, bp.QSIZE, 72, 4, 4))
        Qw[:, :, at:at + cnt] = Q[:, :, first:first + cnt]
        o.qdp[0] = Qw * o.dp[:, None]; o.qdp[1] = o.qdp[0]
        for nstep in (0, 1):
            o.dcmip_step_inputs(1, nstep, dt); o.advec_tracers_remap_rk2(dt, nstep)
            out["ref%d_w%d" % (nstep + 1, w)] = o.qdp[1 - nstep].copy()
            out["dp%d_w%d" % (nstep + 1, w)] = o.dp - dt * o.divdp_proj
        # the step after the cycle, the one that starts from the bounds the remap emitted: the checker's step from the device's cycle
        # state (as _step_after; mixing ratio 1 on the made-up levels)
        o.dcmip_init(1); o.dcmip_step_inputs(1, bp.RSPLIT, dt)
        qw = np.repeat(o.dp[:, None], bp.QSIZE, axis=1)
        qw[:, :, at:at + cnt] = c1[:, :, first:first + cnt]
        o.qdp[0] = qw; o.qdp[1] = qw
        o.advec_tracers_remap_rk2(dt, bp.RSPLIT)
        out["ref3_w%d" % w], out["dp3_w%d" % w] = o.qdp[0].copy(), o.dp - dt * o.divdp_proj
        o.close()
    return out


def _child(spec, tmp_path, timeout=300):
    out = str(tmp_path / "r.npz")
    env = dict(os.environ)
    for k in ("TSE_REMAP_FUSED", "TSE_BOUNDARY_STRIPS", "TSE_DSS_ON_READ", "TSE_LIB", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(dict(spec, out=out))], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    return dict(np.load(out))


@pytest.mark.parametrize("nlev", [64, 80])
def test_other_level_counts(tmp_path, nlev):
    res = _child(dict(nlev=nlev), tmp_path)
    assert res["steps"].shape[2] == nlev
    _assert_cached_is_recomputed("%d levels" % nlev, res)
    import vcoord_levels as vl
    from transport_se_amd.hybvcoord import HvCoord
    steps = (("step1", 1, "step 1"), ("step2", 2, "step 2 (cached bounds)"), ("cycle2", 3, "step after the cycle (the remap's bounds)"))
    for w, (at, first, cnt) in enumerate(_windows(nlev)):
        for key, s, what in steps:
            got = res[key][:, :, first:first + cnt]
            ref = res["ref%d_w%d" % (s, w)][:, :, at:at + cnt], res["dp%d_w%d" % (s, w)][:, at:at + cnt]
            _check("%d levels, window %d, %s" % (nlev, w, what), got, ref, Q_TOL)
    _check_remap("%d levels, the cycle's remap" % nlev, res["cycle1"], res["step1"], res["dp3d"], res["ps_v"], HvCoord(*vl.paths(nlev)))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    _spec = json.loads(sys.argv[2])
    np.savez(_spec["out"], **_nlev_job(_spec["nlev"]))
