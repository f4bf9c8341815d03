"""-m gpu: the library built for 80 levels (libtransport_se_hip_L80.so) on the 80-level grid of tests/golden/vcoord (12k_top-80{m,i}).

No reference run exists at 80 levels, so the evidence is
  * level embedding, the other way round from test_gpu_nlev64.py: every horizontal operation of a tracer step is local to its level, so
    levels 0..71 of the 80-level step of a smooth 80-level state must equal the 72-level library stepping the first 72 levels (with
    hyai[:73], hybi[:73] of the 80-level grid) BIT FOR BIT, and levels 0..63 and 16..79 the 64-level library stepping those windows (a
    window starts on a multiple of 4, so that chunk boundaries coincide) -- per-stage API and whole-step call (DSS on read and
    TSE_DSS_ON_READ=0), limiter 8 and 0, nu_q > 0, one context and three emulated ranks;
  * tse_remap_q_ppm and tse_vertical_remap at 80 levels against tests/remap_ld.py's longdouble value under its pointwise bound (the
    bound, the cap on unsafe outputs, the uniform-ratio and the bad-grid guards of test_gpu_remap_pointwise.py, whose checks are
    called from here);
  * end to end on the 80-level grid through PrimRun and bin/preqx.
Each library runs in a child process of its own (this file with --worker), so that one process never holds two of them."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NLEV = 80
DT_REMAP = 512.0   # a power of two: dp - dt*divdp_proj rounds once, fused or not, so the host knows dp3d's bits


# ---------------------------------------------------------------------------------------------------------------------------
# worker side (a child process): one library, one job, results into an npz
def _state80(ne, mine, qsize, hv):
    """a smooth, deterministic 80-level tracer state and its step inputs at the elements `mine` (test_gpu_nlev64._state on 80 levels)"""
    from transport_se_amd import cube_mesh as cm
    geo = cm.geometry(ne, cm.topology(ne))
    lat, lon = geo["lat"][mine], geo["lon"][mine]                       # [e][4][4]
    ps = 1.0e5 * (1.0 + 0.01 * np.sin(2 * lon) * np.cos(lat))
    k = np.arange(NLEV)[None, :, None, None]
    dp = (np.diff(hv.hyai)[None, :, None, None] * hv.ps0 + np.diff(hv.hybi)[None, :, None, None] * ps[:, None])
    u = 20.0 * np.cos(lat)[:, None] * (1.0 + 0.3 * np.sin(0.2 * k))
    v = 5.0 * np.sin(2 * lon)[:, None] * np.cos(lat)[:, None] * np.cos(0.1 * k)
    vn0 = np.stack([u * dp, v * dp], axis=2)                               # [e][k][2][4][4]
    ki = np.arange(NLEV + 1)[None, :, None, None]
    eta = 1e-3 * np.sin(lon)[:, None] * np.cos(lat)[:, None] * np.sin(0.3 * ki) * hv.ps0
    omega = 0.1 * np.cos(lon + lat)[:, None] * np.cos(0.15 * k) * np.ones_like(dp)
    q = np.empty((mine.size, qsize, NLEV, 4, 4))
    for t in range(qsize):
        q[:, t] = (0.5 + 0.4 * np.sin(lon * (1 + t % 3) + 0.2 * t)[:, None] * np.cos(lat)[:, None] * np.cos(0.07 * (t + 1) * k)) * dp
    return dict(Qdp=q, vn0=vn0, dp=dp, eta_dot_dpdn=eta, omega_p=omega)


def _window(st, lo, n):
    return dict(Qdp=st["Qdp"][:, :, lo:lo + n], vn0=st["vn0"][:, lo:lo + n], dp=st["dp"][:, lo:lo + n],
                eta_dot_dpdn=st["eta_dot_dpdn"][:, lo:lo + n + 1], omega_p=st["omega_p"][:, lo:lo + n])


def _contexts(ne, world, nlev, lo, qsize, limiter, nu_q, body):
    """one HipMod per emulated rank (threads, exchange by device copies as tests/test_gpu_multirank_emulated.py) of the library built
    for `nlev` levels, given levels lo .. lo+nlev-1 of the 80-level grid and state; returns the results by global element"""
    import ctypes as C
    import threading
    import nlev80_common as c80
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.driver import partition
    from transport_se_amd.hip_mod import HipMod
    hv = c80.hv80()
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    owner = partition(ne, world)
    descs = [cm.edge_descriptors(topo, owner, r) for r in range(world)]
    hip = C.CDLL("libamdhip64.so")
    barrier = threading.Barrier(world)
    bufs, lens, result, errors = [None] * world, [dict() for _ in range(world)], [None] * world, []

    class Exchange:
        def __init__(self, r):
            self.r = r
            lens[r][0] = ([s[2] for s in descs[r]["send"]], [s[2] for s in descs[r]["recv"]])

        def set_minmax_layout(self, send_len, recv_len):
            lens[self.r][1] = ([int(x) for x in send_len], [int(x) for x in recv_len])

        def __call__(self, sbuf, rbuf, nlyr, kind):
            r = self.r
            bufs[r] = (sbuf, nlyr)
            barrier.wait()
            roff = np.concatenate([[0], np.cumsum(lens[r][kind][1])]).astype(int)
            for i, (peer, _, _) in enumerate(descs[r]["recv"]):
                j = [x for x, s in enumerate(descs[peer]["send"]) if s[0] == r][0]
                soff = np.concatenate([[0], np.cumsum(lens[peer][kind][0])]).astype(int)
                ln = lens[r][kind][1][i]
                assert lens[peer][kind][0][j] == ln and bufs[peer][1] == nlyr
                rc = hip.hipMemcpy(C.c_void_p(rbuf + int(roff[i]) * nlyr * 8), C.c_void_p(bufs[peer][0] + int(soff[j]) * nlyr * 8),
                                   C.c_size_t(ln * nlyr * 8), C.c_int(3))
                assert rc == 0
            assert hip.hipDeviceSynchronize() == 0
            barrier.wait()
            return 0

    def worker(r):
        try:
            d = descs[r]; mine = d["elems"]
            elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine],
                        spheremp=geo["spheremp"][mine], rspheremp=geo["rspheremp"][mine],
                        putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
            h = HipMod(elem, cm.dvv(), (hv.hyai[lo:lo + nlev + 1], hv.hybi[lo:lo + nlev + 1], hv.ps0), qsize, nu_q, device=0,
                       limiter_option=limiter, schedule=dict(send=d["send"], recv=d["recv"]), exchange=Exchange(r) if world > 1 else None)
            assert h.nlev == nlev and h.L.tse_nlev() == nlev
            result[r] = (mine, body(h, elem, _window(_state80(ne, mine, qsize, hv), lo, nlev)))
            h.close()
        except Exception as ex:  # noqa: BLE001
            errors.append(repr(ex))
            try:
                barrier.abort()
            except Exception:  # noqa: BLE001
                pass
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not errors, errors
    nelem = 6 * ne * ne
    out = {}
    for mine, res in result:
        for key, x in res.items():
            if key not in out:
                out[key] = np.zeros((nelem,) + x.shape[1:])
            out[key][mine] = x
    return out


def _embed_job(ne, world, nlev, lo, qsize, limiter, route, dt=300.0, nu_q=5e15):
    def body(h, elem, st):
        n = st["dp"].shape[0]
        elem["Qdp"] = np.ascontiguousarray(np.stack([st["Qdp"], st["Qdp"]], axis=1))
        for key in ("vn0", "dp", "eta_dot_dpdn", "omega_p"):
            elem[key] = np.ascontiguousarray(st[key])
        h.copy_qdp_h2d(elem, 1); h.copy_qdp_h2d(elem, 2)
        h.set_derived(elem)
        if route == "stages":   # Prim_Advec_Tracers_remap_rk2 through the per-stage entries (prim_advection_mod.F90:579-640)
            h.compute_divdp()
            h.euler_step(2, 1, dt / 2, 3, 0); h.euler_step(2, 2, dt / 2, 1, 1); h.euler_step(2, 2, dt / 2, 2, 2)
            h.qdp_time_avg(3, 1, 2)
        else:
            os.environ["TSE_DSS_ON_READ"] = "0" if route == "whole_dss_per_stage" else "1"
            h.advec_tracers_remap_rk2(dt, 1, 2)
        out = dict(divdp_proj=np.zeros((n, nlev, 4, 4)), eta_dot_dpdn=np.zeros((n, nlev + 1, 4, 4)), omega_p=np.zeros((n, nlev, 4, 4)),
                   divdp=np.zeros((n, nlev, 4, 4)))
        h.get_derived(out)
        h.copy_qdp_d2h(elem, 2)
        out["Qdp"] = elem["Qdp"][:, 1].copy()
        if limiter == 8:
            out["qmin"], out["qmax"] = h.get_qminmax()
        return out
    return _contexts(ne, world, nlev, lo, qsize, limiter, nu_q, body)


def _hip80(qsize, alg):
    import nlev80_common  # noqa: F401  (remap_ld.hvcoord(80))
    import test_gpu_remap_pointwise as rp
    return rp._hip(NLEV, qsize, alg)


def vremap_inputs(qsize):
    """the state of the tse_vertical_remap test from remap_ld.inputs(80, qsize): the layers the launch starts from are remap_ld's source
    grid dp1 (its target grid where the family displaces the target: `gentle`), moved by dt*divdp_proj of up to 2 %; the tracer
    families and scalings as they are.  -> Qdp, dp, divdp_proj"""
    import nlev80_common  # noqa: F401
    import remap_ld as rl
    Q, dp1, dp2 = rl.inputs(NLEV, qsize)
    src = np.stack([dp2[e] if rl.grid_family(e) == "gentle" else dp1[e] for e in range(rl.NELEM)])
    rng = np.random.default_rng(8000 + qsize)
    dv = 0.02 * src * rng.uniform(-1, 1, src.shape) / DT_REMAP
    dp = src + DT_REMAP * dv
    return Q / dp1[:, None] * (dp - DT_REMAP * dv)[:, None], dp, dv


def vremap_grids(dp, dv, hv):
    """what k_remap's phase 1 makes of (dp, divdp_proj), bit for bit: dp3d = dp - dt*divdp_proj (dt a power of two: one rounding), ps_v =
    fma(hyai(1), ps0, serial sum of dp3d), target dp2(k) = fma(hyai(k+1) - hyai(k), ps0, fl((hybi(k+1) - hybi(k)) * ps_v)) -- the FMAs in
    exact rational arithmetic, rounded once"""
    dp3d = dp - DT_REMAP * dv
    run = np.zeros_like(dp3d[:, 0])
    for k in range(dp3d.shape[1]):
        run = run + dp3d[:, k]

    def fma(a, b, c):
        return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))
    ps = np.array([fma(hv.hyai[0], hv.ps0, x) for x in run.ravel()]).reshape(run.shape)
    dA, dB = np.diff(hv.hyai), np.diff(hv.hybi)
    dp2 = np.empty_like(dp3d)
    for k in range(dp3d.shape[1]):
        t = dB[k] * ps
        dp2[:, k] = np.array([fma(dA[k], hv.ps0, x) for x in t.ravel()]).reshape(t.shape)
    return dp3d, ps, dp2


def _remap80_job(spec):
    import nlev80_common as c80
    import remap_ld as rl
    out = {}
    alg = spec["alg"]
    if spec["kind"] == "remap80":
        for qsize in c80.REMAP_QSIZES:
            Q, dp1, dp2 = rl.inputs(NLEV, qsize)          # (asserts the precondition)
            h = _hip80(qsize, alg)
            for generic in (0, 1):
                os.environ["TSE_REMAP_GENERIC"] = str(generic)
                out["%d/%d" % (qsize, generic)] = h.remap_q_ppm(Q, dp1, dp2)
            h.close()
    else:   # vremap80: TSE_REMAP_NT and TSE_REMAP_GENERIC come with the spec's env
        hv = c80.hv80()
        for qsize in c80.REMAP_QSIZES:
            Q, dp, dv = vremap_inputs(qsize)
            dp3d, ps, dp2 = vremap_grids(dp, dv, hv)
            rl.check_inputs(dp3d, dp2)                    # nothing that fails the precondition reaches the device
            h = _hip80(qsize, alg)
            n = dp.shape[0]
            elem = dict(Qdp=np.ascontiguousarray(np.stack([Q, Q], axis=1)), dp=np.ascontiguousarray(dp), divdp=np.zeros_like(dp),
                        divdp_proj=np.ascontiguousarray(dv), vn0=np.zeros((n, NLEV, 2, 4, 4)), eta_dot_dpdn=np.zeros((n, NLEV + 1, 4, 4)),
                        omega_p=np.zeros_like(dp))
            h.copy_qdp_h2d(elem, 1); h.copy_qdp_h2d(elem, 2)
            h.set_derived(elem); h.set_divdp(elem)
            h.vertical_remap(DT_REMAP, 2)
            h.copy_qdp_d2h(elem, 2)
            der = dict(dp3d=np.zeros((n, NLEV, 4, 4)), ps_v=np.zeros((n, 4, 4)))
            h.get_derived(der)
            out["%d/out" % qsize], out["%d/dp3d" % qsize], out["%d/ps_v" % qsize] = elem["Qdp"][:, 1].copy(), der["dp3d"], der["ps_v"]
            h.close()
    return out


def _prim_job(spec):
    """PrimRun on the 80-level grid: Qdp, Q, lnps, the tracer mass before / after and the state checksum"""
    import torch
    import nlev80_common as c80
    from transport_se_amd.driver import PrimRun
    run = PrimRun(spec["ne"], spec["qsize"], test_case=spec["test"], tstep=spec["tstep"], rsplit=3, hvcoord=c80.hv80(), world=1)
    assert run.nlev == NLEV and run.hip.nlev == NLEV and run.hip.L.tse_nlev() == NLEV
    m0 = run.hip.element_mass(1).sum(0)
    np1 = 2
    for n in spec["chunks"]:
        np1 = run.run(n)
    out = dict(qdp=run.fetch_qdp(np1), m0=m0, m1=run.hip.element_mass(np1).sum(0), nstep=np.array(run.nstep),
               checksum=np.array(run.state_checksum(np1, torch), dtype=np.int64))
    out["Q"], out["lnps"] = run.fetch_q(np1)
    out["ps_v"] = run.hip.fetch("ps_v", (run.mine.size, 4, 4))
    run.close()
    return out


def _primrank_job(spec):
    """one rank of a PrimRun on `world` staged ranks sharing the GPU (started by torch.distributed.run): its state checksum"""
    import torch
    import torch.distributed as dist
    import nlev80_common as c80
    from transport_se_amd.driver import PrimRun
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    run = PrimRun(spec["ne"], spec["qsize"], test_case=spec["test"], tstep=spec["tstep"], rsplit=3, hvcoord=c80.hv80(), rank=rank, world=world, device=0,
                  dist_mod=dist, torch_mod=torch, exchange="staged")
    assert run.nlev == NLEV
    np1 = 2
    for n in spec["chunks"]:
        np1 = run.run(n)
    out = dict(mine=run.mine, checksum=np.array(run.state_checksum(np1, torch), dtype=np.int64))
    run.close()
    dist.barrier()
    dist.destroy_process_group()
    return out


def _refuse_job():
    """a 72-level host (the shipped acme-72 coordinate) handed the 80-level library"""
    from transport_se_amd import _lib
    from transport_se_amd.hip_mod import HipMod
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord()
    try:
        HipMod({}, np.zeros((4, 4)), (hv.hyai, hv.hybi, hv.ps0), 1, 0.0, lib_path=_lib.so_path(NLEV))
        msg = ""
    except RuntimeError as ex:
        msg = str(ex)
    return dict(msg=np.array(msg))


def _worker(spec):
    kind = spec["kind"]
    for k, v in spec.get("env", {}).items():
        os.environ[k] = v
    out = {}
    if kind == "embed":   # every (route, qsize) of the spec, one context set after the other
        for route in spec["routes"]:
            for qsize in spec["qsizes"]:
                res = _embed_job(spec["ne"], spec["world"], spec["nlev"], spec["lo"], qsize, spec["limiter"], route)
                out.update({"%s/%d/%s" % (route, qsize, k): v for k, v in res.items()})
    elif kind in ("remap80", "vremap80"):
        out = _remap80_job(spec)
    elif kind in ("uniform", "guard"):   # test_gpu_remap_pointwise.py's own jobs at 80 levels
        import nlev80_common  # noqa: F401
        import test_gpu_remap_pointwise as rp
        rp._worker(spec)
        return
    elif kind == "prim":
        out = _prim_job(spec)
    elif kind == "primrank":
        out = _primrank_job(spec)
        spec = dict(spec, out=spec["out"] % int(os.environ["RANK"]))
    elif kind == "refuse":
        out = _refuse_job()
    np.savez(spec["out"], **out)


# ---------------------------------------------------------------------------------------------------------------------------
# test side
_results = {}   # a child's result by its spec: the 80-level runs are shared by the tests that compare against them, unchanged


def _env():
    env = dict(os.environ)
    for k in ("TSE_REMAP_GENERIC", "TSE_REMAP_NT", "TSE_REMAP_FUSED", "TSE_DSS_ON_READ", "TSE_LIB", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    return env


def _child(spec, tmp_path_factory, timeout=300):
    key = json.dumps(spec, sort_keys=True)
    if key not in _results:
        out = str(tmp_path_factory.mktemp("n80") / "r.npz")
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(dict(spec, out=out))], env=_env(), cwd=ROOT,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
        assert res.returncode == 0, res.stdout.decode()[-4000:]
        _results[key] = dict(np.load(out))
    return _results[key]


KEYS = ("Qdp", "divdp_proj", "eta_dot_dpdn", "omega_p", "qmin", "qmax")
TRACER_KEYS = ("Qdp", "qmin", "qmax")


def _assert_embedded(a80, sub, prefix, lo, n):
    """levels lo .. lo+n-1 of the 80-level result == the n-level library's result (eta_dot_dpdn: the n interfaces that are DSS'd)"""
    assert prefix + "Qdp" in sub and prefix + "Qdp" in a80, (prefix, sorted(sub)[:8])
    seen = 0
    for key in KEYS:
        if prefix + key not in sub:
            continue
        x80, xs = a80[prefix + key], sub[prefix + key]
        ax = 2 if key in TRACER_KEYS else 1
        assert x80.shape[ax] >= NLEV and xs.shape[ax] >= n
        cut = np.take(x80, range(lo, lo + n), axis=ax)
        xs = np.take(xs, range(n), axis=ax)
        assert np.isfinite(xs).all() and np.abs(xs).max() > 0, key
        if not np.array_equal(cut, xs):
            bad = np.argwhere(cut != xs)
            raise AssertionError("%s%s differs at %d entries, levels %s of the window at %d" % (prefix, key, len(bad), sorted(set(bad[:, ax].tolist()))[:20], lo))
        seen += 1
    assert seen >= 4


ROUTES = ("stages", "whole", "whole_dss_per_stage")   # per-stage API; whole step with DSS on read; whole step, TSE_DSS_ON_READ=0
QSIZES = (1, 4, 5, 7)                                  # one tracer, a whole pad of 4, one and three past it
WINDOWS = ((72, 0), (64, 0), (64, 16))                 # (library, first level): levels 72..79 are inside the last one


@pytest.mark.parametrize("nlev,lo", WINDOWS)
@pytest.mark.parametrize("limiter", [8, 0])
def test_level_embedding_is_bit_for_bit(tmp_path_factory, limiter, nlev, lo):
    """ne 4 (several patches), nu_q > 0: a window of the 80-level step == the 72- / 64-level step of that window of the state, every route"""
    assert lo % 4 == 0 and lo + nlev <= NLEV
    base = dict(kind="embed", ne=4, world=1, limiter=limiter, routes=ROUTES, qsizes=QSIZES)
    a80 = _child(dict(base, nlev=NLEV, lo=0), tmp_path_factory)
    sub = _child(dict(base, nlev=nlev, lo=lo), tmp_path_factory)
    for route in ROUTES:
        for qsize in QSIZES:
            pre = "%s/%d/" % (route, qsize)
            assert a80[pre + "Qdp"].shape[2] == NLEV and sub[pre + "Qdp"].shape[2] == nlev
            _assert_embedded(a80, sub, pre, lo, nlev)


def _three_ranks(limiter):
    return dict(kind="embed", ne=2, limiter=limiter, routes=("stages", "whole"), qsizes=(5,))


@pytest.mark.parametrize("limiter", [8, 0])
def test_three_emulated_ranks_equal_one_context_at_80_levels(tmp_path_factory, limiter):
    """ne 2 cut into 3 ranks (remote columns, packed halos): the 80-level 3-rank step equals the 80-level one-context step bit for bit"""
    a80 = _child(dict(_three_ranks(limiter), nlev=NLEV, lo=0, world=3), tmp_path_factory)
    one = _child(dict(_three_ranks(limiter), nlev=NLEV, lo=0, world=1), tmp_path_factory)
    assert sorted(a80) == sorted(one)
    for key in a80:
        assert np.array_equal(a80[key], one[key]), key


@pytest.mark.parametrize("nlev,lo", WINDOWS)
@pytest.mark.parametrize("limiter", [8, 0])
def test_level_embedding_on_three_emulated_ranks(tmp_path_factory, limiter, nlev, lo):
    """... and its windows equal the 72- and 64-level 3-rank steps"""
    a80 = _child(dict(_three_ranks(limiter), nlev=NLEV, lo=0, world=3), tmp_path_factory)
    sub = _child(dict(_three_ranks(limiter), nlev=nlev, lo=lo, world=3), tmp_path_factory)
    for route in ("stages", "whole"):
        _assert_embedded(a80, sub, "%s/5/" % route, lo, nlev)


@pytest.mark.parametrize("alg", [0, 2])
def test_remap_q_ppm_pointwise_at_80_levels(tmp_path_factory, alg):
    """tse_remap_q_ppm, lockstep and generic column loop, qsize 1, 2, 3 (segment tasks only), 7, 19: test_gpu_remap_pointwise._check
    (the bound on every safe output, at most 1 % unsafe per family pair and those within 1e-13 of the field maximum, every column's mass)"""
    import nlev80_common as c80
    import remap_ld as rl
    import test_gpu_remap_pointwise as rp
    from step_ld import has_extended_precision
    assert has_extended_precision(), np.finfo(np.longdouble)
    res = _child(dict(kind="remap80", alg=alg), tmp_path_factory)
    Q, dp1, dp2 = rl.inputs(NLEV, 1)
    assert c80.kid_offsets(dp1, dp2).max() > 15      # some column's kid(k) far outside {k, k+1}
    for qsize in c80.REMAP_QSIZES:
        Q, dp1, dp2 = rl.inputs(NLEV, qsize)
        t, safe, kid = rl.remap_q_ppm(Q, dp1, dp2, alg)
        assert t.m == 81
        for generic in (0, 1):
            got = res["%d/%d" % (qsize, generic)]
            assert got.shape == Q.shape and np.isfinite(got).all()
            worst = {}
            rp._check("L80 alg%d generic%d" % (alg, generic), qsize, got, Q, t, safe, kid, worst)
            print("pointwise remap L80 alg%d generic%d qsize %d: worst ratio %.4g, column mass %.4g"
                  % (alg, generic, qsize, max(v[0] for k, v in worst.items() if k != "mass"), worst["mass"][0]))


@pytest.mark.parametrize("alg", [0, 2])
@pytest.mark.parametrize("env", [{}, {"TSE_REMAP_NT": "2"}, {"TSE_REMAP_GENERIC": "1"}], ids=["fast", "nt2", "generic"])
def test_vertical_remap_pointwise_at_80_levels(tmp_path_factory, alg, env):
    """tse_vertical_remap (the product route: dp3d, ps_v and the target grid formed in the launch): dp3d and ps_v are the bits the host
    derives (vremap_grids), and the remapped tracers lie under the same pointwise bound on those grids; one and two tracers per thread,
    the generic loop, segment tasks (qsize 1, 2, 3, 19)"""
    import nlev80_common as c80
    import remap_ld as rl
    import test_gpu_remap_pointwise as rp
    hv = c80.hv80()
    res = _child(dict(kind="vremap80", alg=alg, env=env), tmp_path_factory)
    for qsize in c80.REMAP_QSIZES:
        Q, dp, dv = vremap_inputs(qsize)
        dp3d, ps, dp2 = vremap_grids(dp, dv, hv)
        assert np.array_equal(res["%d/dp3d" % qsize], dp3d) and np.array_equal(res["%d/ps_v" % qsize], ps)
        t, safe, kid = rl.remap_q_ppm(Q, dp3d, dp2, alg)
        got = res["%d/out" % qsize]
        assert got.shape == Q.shape and np.isfinite(got).all()
        rp._check("L80 vertical_remap alg%d %s" % (alg, env), qsize, got, Q, t, safe, kid, {})


@pytest.mark.parametrize("alg", [0, 2])
def test_uniform_mixing_ratio_and_bad_grids_at_80_levels(tmp_path_factory, alg):
    """the two guards of test_gpu_remap_pointwise.py at 80 levels: Q = c*dp1 stays c per level to Q_TOL_CYCLES; a target grid the bracket
    search cannot end on is refused before any launch"""
    import nlev80_common  # noqa: F401
    import remap_ld as rl
    import test_gpu_remap_pointwise as rp
    res = _child(dict(kind="uniform", nlev=NLEV, alg=alg), tmp_path_factory)
    Q, dp1, dp2, c = rl.uniform_inputs(NLEV)
    for generic in rp.GENERIC:
        rel = np.abs(res["%d" % generic] / dp2[:, None] / c[None, :, None, None, None] - 1.0)
        assert rel.max() <= rp.Q_TOL_CYCLES, (generic, float(rel.max()))
    if alg == 0:
        res = _child(dict(kind="guard", nlev=NLEV, alg=0), tmp_path_factory)
        msgs, (n0, n1, n2) = [str(m) for m in res["msgs"]], res["counts"]
        e, p, k = res["where"]
        assert all(m.startswith("tse_remap_q_ppm: ") for m in msgs), msgs
        assert "dp2" in msgs[0] and "element 0, column 0, level 5" in msgs[0], msgs[0]
        assert "dp1" in msgs[1] and "element 0, column 0, level 0" in msgs[1], msgs[1]
        assert "element %d, column %d, level %d" % (e, p, k) in msgs[2] and "partial sum of dp2" in msgs[2], msgs[2]
        assert n0 == 1 and n1 == n0 and n2 == n0 + 1 and bool(res["same"])


def _ranks(spec, world, tmp_path_factory, timeout=300):
    """the primrank job on `world` ranks (torch.distributed.run): the sum of the ranks' state checksums (wrap-around int64)"""
    import socket
    out = str(tmp_path_factory.mktemp("n80w") / "w_%d.npz")
    env = dict(_env(), GLOO_SOCKET_IFNAME="lo")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.abspath(__file__), "--worker", json.dumps(dict(spec, out=out))],
                         env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    parts = [np.load(out % r) for r in range(world)]
    seen = np.zeros(6 * spec["ne"] ** 2, dtype=int)
    for p in parts:
        seen[p["mine"]] += 1
    assert (seen == 1).all()
    with np.errstate(over="ignore"):
        return int(np.sum(np.array([p["checksum"] for p in parts], dtype=np.int64)))


TSTEP = {1: 900.0, 2: 300.0}   # ne 4 (test_gpu_state_q.py's DT / DT12: DCMIP 1-2's vertical motion empties layers at the 1-1 step)


@pytest.mark.parametrize("test,qsize", [(1, 4), (2, 19)])
def test_dcmip_end_to_end_on_the_80_level_grid(tmp_path_factory, test, qsize):
    """DCMIP 1-1 (4 tracers) and 1-2 (19: the fused remap with segment tasks) at ne 4 through PrimRun(hvcoord = the 80-level files), six
    steps with rsplit = 3 (two remap cycles): tracer mass kept to 1e-11 (test_gpu_nlev64.py's margin); the fused remap and
    TSE_REMAP_FUSED=0, and a run cut into chunks, leave the same bits; tse_state_q / copy_lnps give the host expression Qdp/dp bit for
    bit and lnps within 1 ulp of log(ps_v) (test_gpu_state_q.py's conditions)"""
    import math
    import nlev80_common as c80
    base = dict(kind="prim", ne=4, qsize=qsize, test=test, tstep=TSTEP[test])
    one = _child(dict(base, chunks=[6]), tmp_path_factory)
    assert int(one["nstep"]) == 6 and one["qdp"].shape[2] == NLEV and np.isfinite(one["qdp"]).all() and np.abs(one["qdp"]).max() > 0
    rel = np.abs(one["m1"] - one["m0"]) / np.abs(one["m0"])
    assert rel.max() < 1e-11, rel
    pieces = _child(dict(base, chunks=[2, 1, 3]), tmp_path_factory)
    assert np.array_equal(one["qdp"], pieces["qdp"]) and np.array_equal(one["Q"], pieces["Q"]) and np.array_equal(one["lnps"], pieces["lnps"])
    unfused = _child(dict(base, chunks=[6], env={"TSE_REMAP_FUSED": "0"}), tmp_path_factory)
    assert np.array_equal(one["qdp"], unfused["qdp"])
    hv = c80.hv80()
    assert one["Q"].shape == one["qdp"].shape and one["lnps"].shape == one["ps_v"].shape
    ref = np.vectorize(math.log)(one["ps_v"])
    assert (np.abs(one["lnps"] - ref) <= np.spacing(ref)).all()
    dp = (np.diff(hv.hyai)[None, :, None, None] * 1.0e5) + (np.diff(hv.hybi)[None, :, None, None] * one["ps_v"][:, None])
    assert np.array_equal(one["Q"], one["qdp"] / dp[:, None])


@pytest.mark.parametrize("world", [1, 2, 3])
def test_prim_run_on_staged_ranks_has_the_same_checksum_at_80_levels(tmp_path_factory, world):
    """PrimRun on the 80-level grid on 1, 2 and 3 ranks (host-staged halo, ranks sharing the GPU): the same state_checksum, which is
    the one-context run's"""
    spec = dict(ne=4, qsize=19, test=2, tstep=TSTEP[2], chunks=[6])
    one = int(_child(dict(spec, kind="prim"), tmp_path_factory)["checksum"])
    assert _ranks(dict(spec, kind="primrank"), world, tmp_path_factory) == one


NL80 = """
&ctl_nl
  test_case = "dcmip1-1"
  ne = 4
  qsize = 4
  nmax = 6
  statefreq = 3
  tstep = 900
  qsplit = 1, rsplit = 3
  nu_q = 5e17
  limiter_option = 8
  hypervis_order = 2
/
&vert_nl
  vform = "ccm"
  vfile_mid = "vcoord/12k_top-80m.ascii"
  vfile_int = "vcoord/12k_top-80i.ascii"
/
"""


def test_preqx_reads_the_80_level_namelist(tmp_path):
    """bin/preqx with a namelist whose &vert_nl names the two 80-level files (in the working directory): it runs, prints a finite norm
    line, conserved tracer mass and 80 levels' worth of work, and writes HommeTime_stats"""
    import shutil
    import vcoord_levels as vl
    os.makedirs(tmp_path / "vcoord")
    for f in vl.paths(NLEV):
        shutil.copy(f, tmp_path / "vcoord" / os.path.basename(f))
    res = subprocess.run([os.path.join(ROOT, "bin", "preqx")], input=NL80.encode(), cwd=str(tmp_path), env=_env(),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = res.stdout.decode()
    assert res.returncode == 0, out[-3000:]
    norm = [l for l in out.splitlines() if l.startswith("DCMIP 1-1:")]
    assert norm, out[-2000:]
    import re
    vals = [float(x) for x in re.findall(r"[-+]?\d+\.\d+(?:[eE][-+]?\d+)?", norm[-1].split(":", 1)[1])]
    assert vals and np.isfinite(vals).all(), norm[-1]
    changes = [l for l in out.splitlines() if "relative change" in l]
    assert changes, out[-2000:]
    for l in changes:
        assert abs(float(l.split("relative change")[1].strip(" )"))) < 1e-11, l
    assert os.path.getsize(tmp_path / "HommeTime_stats") > 0


def test_a_72_level_host_is_refused_by_the_80_level_library(tmp_path_factory):
    res = _child(dict(kind="refuse"), tmp_path_factory)
    assert "libtransport_se_hip_L80.so is built for nlev = 80, not 72" in str(res["msg"]), res["msg"]


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    _worker(json.loads(sys.argv[2]))
