"""-m gpu: the library built for 64 levels (libtransport_se_hip_L64.so; the reference's 12k_top-64 grid).

No reference run exists at 64 levels, so the evidence is
  * level embedding: every horizontal operation of a tracer step is local to its level, so the first 64 levels of a 72-level
    state (with hyai[:65], hybi[:65]) stepped by the 64-level library must equal levels 0..63 of the 72-level run BIT FOR BIT --
    per-stage API and whole-step call (DSS on read and TSE_DSS_ON_READ=0), limiter 8 and 0, nu_q > 0, one context and three
    emulated ranks;
  * the remap against tests/remap_model.py (held to the oracle at 72 levels by tests/test_nlev_cpu.py);
  * tse_vertical_remap against the same model (one and two tracers per thread, generic loop, segment tasks);
  * end to end on the 12k_top-64 grid: mass, subcycle splitting, fused and unfused remap, PrimRun on 1, 2 and 3 ranks, and bin/preqx.
Each library runs in a child process of its own (this file with --worker), so that one process never holds two of them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VC = os.path.join(ROOT, "tests", "golden", "vcoord")
pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
# worker side (a child process): one library, one job, results into an npz
def _state(ne, mine, qsize, nlev, hv):
    """a smooth, deterministic 72-level tracer state and its step inputs at the elements `mine`, cut to `nlev` levels"""
    from transport_se_amd import cube_mesh as cm
    geo = cm.geometry(ne, cm.topology(ne))
    lat, lon = geo["lat"][mine], geo["lon"][mine]                       # [e][4][4]
    ps = 1.0e5 * (1.0 + 0.01 * np.sin(2 * lon) * np.cos(lat))
    k = np.arange(72)[None, :, None, None]
    dp = (np.diff(hv.hyai)[None, :, None, None] * hv.ps0 + np.diff(hv.hybi)[None, :, None, None] * ps[:, None])
    u = 20.0 * np.cos(lat)[:, None] * (1.0 + 0.3 * np.sin(0.2 * k))
    v = 5.0 * np.sin(2 * lon)[:, None] * np.cos(lat)[:, None] * np.cos(0.1 * k)
    vn0 = np.stack([u * dp, v * dp], axis=2)                               # [e][k][2][4][4]
    ki = np.arange(73)[None, :, None, None]
    eta = 1e-3 * np.sin(lon)[:, None] * np.cos(lat)[:, None] * np.sin(0.3 * ki) * hv.ps0
    omega = 0.1 * np.cos(lon + lat)[:, None] * np.cos(0.15 * k) * np.ones_like(dp)
    q = np.empty((mine.size, qsize, 72, 4, 4))
    for t in range(qsize):
        q[:, t] = (0.5 + 0.4 * np.sin(lon * (1 + t % 3) + 0.2 * t)[:, None] * np.cos(lat)[:, None] * np.cos(0.07 * (t + 1) * k)) * dp
    return dict(Qdp=q[:, :, :nlev], vn0=vn0[:, :nlev], dp=dp[:, :nlev], eta_dot_dpdn=eta[:, :nlev + 1], omega_p=omega[:, :nlev])


def _contexts(ne, world, nlev, qsize, limiter, nu_q, body):
    """one HipMod per emulated rank (threads, exchange by device copies as tests/test_gpu_multirank_emulated.py), each running
    body(rank, hip, mine, state); returns the per-rank results"""
    import ctypes as C
    import threading
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.driver import partition
    from transport_se_amd.hip_mod import HipMod
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord()
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
            h = HipMod(elem, cm.dvv(), (hv.hyai[:nlev + 1], hv.hybi[:nlev + 1], hv.ps0), qsize, nu_q, device=0, limiter_option=limiter,
                       schedule=dict(send=d["send"], recv=d["recv"]), exchange=Exchange(r) if world > 1 else None)
            assert h.nlev == nlev and h.L.tse_nlev() == nlev
            result[r] = (mine, body(h, elem, _state(ne, mine, qsize, nlev, hv)))
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


def _embed_job(ne, world, nlev, qsize, limiter, route, dt=300.0, nu_q=5e15):
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
    return _contexts(ne, world, nlev, qsize, limiter, nu_q, body)


def _remap_job(qsize, alg, nlev=64, ne=2, seed=0):
    """tse_remap_q_ppm on a deterministic column set (the host calls remap_q_ppm of hip_mod)"""
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord(os.path.join(VC, "12k_top-64m.ascii"), os.path.join(VC, "12k_top-64i.ascii"))
    rng = np.random.default_rng(seed)

    def body(h, elem, st):
        n = st["dp"].shape[0]
        ps = 1e5 * (1 + 0.02 * rng.standard_normal((n, 1, 4, 4)))
        dp2 = np.diff(hv.hyai)[None, :, None, None] * hv.ps0 + np.diff(hv.hybi)[None, :, None, None] * ps
        dp1 = dp2 * (1 + 0.05 * rng.standard_normal(dp2.shape).clip(-2, 2))
        dp1 *= dp2.sum(1, keepdims=True) / dp1.sum(1, keepdims=True)
        q = rng.random((n, qsize, nlev, 4, 4)) * dp1[:, None] * (1 + np.arange(qsize))[None, :, None, None, None]
        return dict(q=q, dp1=dp1, dp2=dp2, out=h.remap_q_ppm(q, dp1, dp2))
    return body


def _vremap_job(qsize, alg, nlev=64, seed=1, dt=600.0):
    """tse_vertical_remap (the product route: the target grid from hyai/hybi and ps_v in phase 1) on a deterministic state: dp from
    the 12k_top-64 coefficients, layers moved by divdp_proj, Qdp at time level 2"""
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord(os.path.join(VC, "12k_top-64m.ascii"), os.path.join(VC, "12k_top-64i.ascii"))
    rng = np.random.default_rng(seed)

    def body(h, elem, st):
        n = st["dp"].shape[0]
        ps = 1e5 * (1 + 0.02 * rng.standard_normal((n, 1, 4, 4)))
        dp = np.diff(hv.hyai)[None, :, None, None] * hv.ps0 + np.diff(hv.hybi)[None, :, None, None] * ps
        divdp_proj = dp * 0.04 * rng.standard_normal(dp.shape).clip(-2, 2) / dt
        q = rng.random((n, qsize, nlev, 4, 4)) * dp[:, None] * (1 + np.arange(qsize))[None, :, None, None, None]
        elem["Qdp"] = np.ascontiguousarray(np.stack([q, q], axis=1))
        elem["dp"] = np.ascontiguousarray(dp)
        elem["divdp"] = np.zeros_like(dp); elem["divdp_proj"] = np.ascontiguousarray(divdp_proj)
        h.copy_qdp_h2d(elem, 1); h.copy_qdp_h2d(elem, 2)
        h.set_derived(elem); h.set_divdp(elem)
        h.vertical_remap(dt, 2)
        h.copy_qdp_d2h(elem, 2)
        der = dict(dp3d=np.zeros((n, nlev, 4, 4)), ps_v=np.zeros((n, 4, 4)))
        h.get_derived(der)
        return dict(q=q, dp=dp, divdp_proj=divdp_proj, dt=np.full((n,), dt), out=elem["Qdp"][:, 1].copy(), dp3d=der["dp3d"], ps_v=der["ps_v"])
    return body


def _primrank_job(spec):
    """one rank of a PrimRun on `world` ranks (started by torch.distributed.run; host-staged halo slots over gloo, the ranks
    share the GPU as bin/preqx does with TSE_EXCHANGE=staged): this rank's elements and its Qdp after the run"""
    import torch
    import torch.distributed as dist
    from transport_se_amd.driver import PrimRun
    from transport_se_amd.hybvcoord import HvCoord
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    hv = HvCoord(os.path.join(VC, "12k_top-64m.ascii"), os.path.join(VC, "12k_top-64i.ascii"))
    run = PrimRun(spec["ne"], spec["qsize"], test_case=spec["test"], rsplit=3, hvcoord=hv, rank=rank, world=world, device=0,
                  dist_mod=dist, torch_mod=torch, exchange="staged")
    assert run.nlev == 64
    np1 = 2
    for n in spec["chunks"]:
        np1 = run.run(n)
    out = dict(mine=run.mine, qdp=run.fetch_qdp(np1))
    run.close()
    dist.barrier()
    dist.destroy_process_group()
    return out


def _worker(spec):
    kind = spec["kind"]
    for k, v in spec.get("env", {}).items():
        os.environ[k] = v
    out = {}
    if kind == "embed":   # every (route, qsize) of the spec, one context set after the other
        for route in spec["routes"]:
            for qsize in spec["qsizes"]:
                res = _embed_job(spec["ne"], spec["world"], spec["nlev"], qsize, spec["limiter"], route)
                out.update({"%s/%d/%s" % (route, qsize, k): v for k, v in res.items()})
    elif kind in ("remap", "vremap"):
        job = _remap_job if kind == "remap" else _vremap_job
        for alg in (0, 2):
            for qsize in spec["qsizes"]:
                res = _contexts_remap(qsize, alg, job(qsize, alg))
                out.update({"%d/%d/%s" % (alg, qsize, k): v for k, v in res.items()})
    elif kind == "prim":
        out = _prim_job(spec)
    elif kind == "primrank":
        out = _primrank_job(spec)
        spec = dict(spec, out=spec["out"] % int(os.environ["RANK"]))
    np.savez(spec["out"], **out)


def _contexts_remap(qsize, alg, body):
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.hip_mod import HipMod
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord(os.path.join(VC, "12k_top-64m.ascii"), os.path.join(VC, "12k_top-64i.ascii"))
    ne = 2
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    from transport_se_amd.driver import partition
    d = cm.edge_descriptors(topo, partition(ne, 1), 0)
    mine = d["elems"]
    elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, 0.0, device=0, vert_remap_q_alg=alg)
    assert h.nlev == 64
    out = body(h, elem, dict(dp=np.zeros((mine.size, 64, 4, 4))))
    h.close()
    return out


def _prim_job(spec):
    """PrimRun on the 12k_top-64 grid: Qdp of both time levels and the tracer mass before / after"""
    from transport_se_amd.driver import PrimRun
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord(os.path.join(VC, "12k_top-64m.ascii"), os.path.join(VC, "12k_top-64i.ascii"))
    run = PrimRun(spec["ne"], spec["qsize"], test_case=spec["test"], rsplit=3, hvcoord=hv, world=1)
    assert run.nlev == 64 and run.hip.nlev == 64
    m0 = run.hip.element_mass(1).sum(0)
    np1 = 2
    for n in spec["chunks"]:
        np1 = run.run(n)
    out = dict(qdp=run.fetch_qdp(np1), m0=m0, m1=run.hip.element_mass(np1).sum(0), nstep=np.array(run.nstep))
    Q, lnps = run.fetch_q(np1)
    out["Q"], out["lnps"] = Q, lnps
    run.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# test side
def _child(spec, tmp_path, timeout=600):
    out = str(tmp_path / ("r%d.npz" % abs(hash(json.dumps(spec, sort_keys=True)))))
    spec = dict(spec, out=out)
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(spec)], env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    return dict(np.load(out))


KEYS = ("Qdp", "divdp_proj", "eta_dot_dpdn", "omega_p", "qmin", "qmax")


def _assert_embedded(a72, a64, prefix):
    assert prefix + "Qdp" in a64, (prefix, sorted(a64)[:8])
    for key in KEYS:
        if prefix + key not in a64:
            continue
        x72, x64 = a72[prefix + key], a64[prefix + key]
        cut = x72[:, :, :64] if key in ("Qdp", "qmin", "qmax") else x72[:, :64]
        x64 = x64[:, :, :64] if key in ("Qdp", "qmin", "qmax") else x64[:, :64]
        assert np.isfinite(x64).all(), key
        if not np.array_equal(cut, x64):
            bad = np.argwhere(cut != x64)
            lv = sorted(set(bad[:, 2 if key in ("Qdp", "qmin", "qmax") else 1].tolist()))
            raise AssertionError("%s%s differs at %d entries, levels %s" % (prefix, key, len(bad), lv[:20]))


ROUTES = ("stages", "whole", "whole_dss_per_stage")   # per-stage API; whole step with DSS on read; whole step, TSE_DSS_ON_READ=0
QSIZES = (1, 4, 5, 35)                                 # one tracer, whole pairs, an odd count, the reference's 35 (pads of 4)


@pytest.mark.parametrize("limiter", [8, 0])
def test_level_embedding_is_bit_for_bit(tmp_path, limiter):
    """levels 0..63 of the 72-level step == the 64-level step of the cut state, every route, tracer counts at the pair and pad edges"""
    base = dict(kind="embed", ne=4, world=1, limiter=limiter, routes=ROUTES, qsizes=QSIZES)
    a72 = _child(dict(base, nlev=72), tmp_path)
    a64 = _child(dict(base, nlev=64), tmp_path)
    for route in ROUTES:
        for qsize in QSIZES:
            pre = "%s/%d/" % (route, qsize)
            assert a64[pre + "Qdp"].shape[2] == 64 and a72[pre + "Qdp"].shape[2] == 72
            assert np.abs(a64[pre + "Qdp"]).max() > 0
            _assert_embedded(a72, a64, pre)


@pytest.mark.parametrize("limiter", [8, 0])
def test_level_embedding_on_three_emulated_ranks(tmp_path, limiter):
    """the same with the sphere cut into 3 ranks (remote columns, packed halos): equal to the 72-level 3-rank run and to the
    64-level one-context run"""
    base = dict(kind="embed", ne=4, limiter=limiter, routes=("stages", "whole"), qsizes=(5,))
    a72 = _child(dict(base, nlev=72, world=3), tmp_path)
    a64 = _child(dict(base, nlev=64, world=3), tmp_path)
    one = _child(dict(base, nlev=64, world=1), tmp_path)
    for route in ("stages", "whole"):
        _assert_embedded(a72, a64, "%s/5/" % route)
    assert sorted(a64) == sorted(one)
    for key in a64:
        assert np.array_equal(a64[key], one[key]), key


def _segment_tracers(qsize, nt=1):
    """remap_left (tse_kernels.h): the tracers k_remap hands to segment tasks -- with 16 tracer slots per block (256 threads, one
    tracer per thread), a remainder of 1..3 tracers after the whole rounds"""
    left = qsize % 16
    return left if nt == 1 and left <= 3 else 0


# tracer counts of the remap tests: segment tasks only (3: the whole column set is one partial round), a full round and one
# segment tracer (17), a full round and three (19), and a count with no segment tasks (7)
REMAP_QSIZES = (3, 7, 17, 19)


@pytest.mark.parametrize("alg", [0, 2])
@pytest.mark.parametrize("env", [{}, {"TSE_REMAP_GENERIC": "1"}], ids=["fast", "generic"])
def test_remap_q_ppm_at_64_levels_against_the_model(tmp_path, alg, env):
    """tse_remap_q_ppm at 64 levels vs tests/remap_model.py: 5e-13 of the field maximum, column mass to 1e-13 (the single-call
    tolerances of test_gpu_ops_golden.py).  (tse_remap_q_ppm always runs one tracer per thread: TSE_REMAP_NT is a switch of
    tse_vertical_remap, tested below.)"""
    from remap_model import remap_q_ppm
    assert [_segment_tracers(q) for q in REMAP_QSIZES] == [3, 0, 1, 3]
    res = _child(dict(kind="remap", qsizes=REMAP_QSIZES, env=env), tmp_path)
    for qsize in REMAP_QSIZES:
        r = {k: res["%d/%d/%s" % (alg, qsize, k)] for k in ("q", "dp1", "dp2", "out")}
        assert r["out"].shape[2] == 64
        for e in range(r["q"].shape[0]):
            ref = remap_q_ppm(r["q"][e], r["dp1"][e], r["dp2"][e], alg)
            got = r["out"][e]
            assert np.abs(got - ref).max() <= 5e-13 * np.abs(ref).max(), (e, np.abs(got - ref).max())
            m0 = r["q"][e].sum(1); m1 = got.sum(1)
            assert np.abs(m1 - m0).max() <= 1e-13 * np.abs(m0).max()


@pytest.mark.parametrize("alg", [0, 2])
@pytest.mark.parametrize("env", [{}, {"TSE_REMAP_NT": "2"}, {"TSE_REMAP_GENERIC": "1"}], ids=["fast", "nt2", "generic"])
def test_vertical_remap_at_64_levels_against_the_model(tmp_path, alg, env):
    """tse_vertical_remap at 64 levels (dp3d = dp - dt*divdp_proj, ps_v = hyai(1)*ps0 + sum(dp3d), target dp from hyai/hybi and ps_v:
    prim_advection_mod.F90:1313-1319) vs tests/remap_model.py on those grids: 5e-13 of the field maximum, column mass to 1e-13;
    one and two tracers per thread (k_remap<1,*> / k_remap<2,*>), the generic column loop, segment tasks (qsize 3, 17, 19)"""
    from remap_model import remap_q_ppm
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord(os.path.join(VC, "12k_top-64m.ascii"), os.path.join(VC, "12k_top-64i.ascii"))
    res = _child(dict(kind="vremap", qsizes=REMAP_QSIZES, env=env), tmp_path)
    for qsize in REMAP_QSIZES:
        r = {k: res["%d/%d/%s" % (alg, qsize, k)] for k in ("q", "dp", "divdp_proj", "dt", "out", "dp3d", "ps_v")}
        assert r["out"].shape[2] == 64
        dp3d = r["dp"] - r["dt"][0] * r["divdp_proj"]
        assert np.abs(r["dp3d"] - dp3d).max() <= 1e-15 * np.abs(dp3d).max()
        run = np.zeros_like(dp3d[:, 0])
        for k in range(64):                                          # the serial sum of the reference (and of k_remap's phase 1)
            run = run + dp3d[:, k]
        ps = hv.hyai[0] * hv.ps0 + run
        assert np.abs(r["ps_v"] - ps).max() <= 1e-15 * np.abs(ps).max()
        dp2 = np.diff(hv.hyai)[None, :, None, None] * hv.ps0 + np.diff(hv.hybi)[None, :, None, None] * ps[:, None]
        for e in range(r["q"].shape[0]):
            ref = remap_q_ppm(r["q"][e], dp3d[e], dp2[e], alg)
            got = r["out"][e]
            assert np.abs(got - ref).max() <= 5e-13 * np.abs(ref).max(), (qsize, e, np.abs(got - ref).max())
            m0 = r["q"][e].sum(1); m1 = got.sum(1)
            assert np.abs(m1 - m0).max() <= 1e-13 * np.abs(m0).max()


def _ranks(spec, world, tmp_path, timeout=600):
    """the primrank job on `world` ranks (torch.distributed.run): Qdp gathered by global element"""
    import socket
    out = str(tmp_path / ("w%d_%%d.npz" % world))
    spec = dict(spec, out=out)
    env = dict(os.environ, GLOO_SOCKET_IFNAME="lo")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.abspath(__file__), "--worker", json.dumps(spec)],
                         env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    parts = [np.load(out % r) for r in range(world)]
    nelem = 6 * spec["ne"] ** 2
    q = np.zeros((nelem,) + parts[0]["qdp"].shape[1:])
    seen = np.zeros(nelem, dtype=int)
    for p in parts:
        q[p["mine"]] = p["qdp"]; seen[p["mine"]] += 1
    assert (seen == 1).all()
    return q


def test_dcmip_end_to_end_on_the_12k_top_64_grid(tmp_path):
    """DCMIP 1-1 and 1-2 at ne4 and ne8 through PrimRun on the 64-level grid, 3 rsplit cycles: tracer mass kept to 1e-11, and
    prim_run_subcycle in one call or in pieces gives the same bits; the fused and unfused remap routes agree bit for bit"""
    for ne, test, qsize in ((4, 1, 4), (8, 2, 4), (4, 1, 19)):   # (19 tracers: the fused remap with segment tasks)
        base = dict(kind="prim", ne=ne, qsize=qsize, test=test)
        one = _child(dict(base, chunks=[9]), tmp_path)
        assert int(one["nstep"]) == 9 and one["qdp"].shape[2] == 64
        rel = np.abs(one["m1"] - one["m0"]) / np.abs(one["m0"])
        assert rel.max() < 1e-11, rel
        pieces = _child(dict(base, chunks=[3, 2, 4]), tmp_path)
        assert np.array_equal(one["qdp"], pieces["qdp"]) and np.array_equal(one["Q"], pieces["Q"])
        unfused = _child(dict(base, chunks=[9], env={"TSE_REMAP_FUSED": "0"}), tmp_path)
        assert np.array_equal(one["qdp"], unfused["qdp"])


@pytest.mark.parametrize("world", [2, 3])
def test_prim_run_on_emulated_ranks_is_bit_for_bit_at_64_levels(tmp_path, world):
    """PrimRun on the 12k_top-64 grid on 2 and 3 ranks (host-staged halo, ranks sharing the GPU) leaves the same Qdp bits as on one
    context; 19 tracers, so the fused remap runs segment tasks"""
    spec = dict(ne=4, qsize=19, test=1, chunks=[9])
    one = _child(dict(spec, kind="prim"), tmp_path)
    many = _ranks(dict(spec, kind="primrank"), world, tmp_path)
    assert many.shape == one["qdp"].shape and np.abs(many).max() > 0
    assert np.array_equal(many, one["qdp"])


NL64 = """
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
  vfile_mid = "vcoord/12k_top-64m.ascii"
  vfile_int = "vcoord/12k_top-64i.ascii"
/
"""


def test_preqx_on_the_12k_top_64_grid_same_digits_on_1_and_2_ranks(tmp_path):
    """bin/preqx with the commented-out 12k_top-64 lines of the reference's dcmip1-1.nl turned on, files in the working
    directory: norm lines printed, 64 levels in the rate line, string-identical on 1 and 2 staged ranks"""
    import shutil
    os.makedirs(tmp_path / "vcoord")
    for f in ("12k_top-64m.ascii", "12k_top-64i.ascii"):
        shutil.copy(os.path.join(VC, f), tmp_path / "vcoord" / f)

    def run(args, env_extra=None):
        env = dict(os.environ); env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
        env.update(env_extra or {})
        res = subprocess.run([os.path.join(ROOT, "bin", "preqx")] + args, input=NL64.encode(), cwd=str(tmp_path), env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = res.stdout.decode()
        assert res.returncode == 0, out[-3000:]
        return out

    def lines(out):
        return [l for l in out.splitlines() if l.startswith(("DCMIP", "Q", "qv= ")) and "wall" not in l]
    out1 = run([])
    one = lines(out1)
    assert any(l.startswith("DCMIP 1-1:") for l in one), out1[-2000:]
    for l in one:
        if "relative change" in l:
            assert abs(float(l.split("relative change")[1].strip(" )"))) < 1e-11, l
    two = lines(run(["--gpus", "2"], {"TSE_EXCHANGE": "staged"}))
    assert two == one, "\n".join(two + ["--"] + one)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    _worker(json.loads(sys.argv[2]))
