"""-m gpu: the halo-exchange timers (tse_comm_timing: comm_pack_*, comm_exchange_*, comm_unpack_*, comm_wait).

  * RCCL loopback (one rank's share of a 4-rank partition of ne8, every neighbour slot pointed at rank 0 of a one-rank communicator,
    as tools/rank_rehearsal.py): the groups have launches and time, the same launches on every tracer step and every prefetching
    remap cycle, and the bounds groups (*_mm) only with the limiter;
  * the timers are pure observation: Qdp bit for bit the same with comm timing on and off and with tse_timing on, on the split route
    (interior launch on its own stream, exchange on the communication stream) and on the routes that exchange on the compute stream;
    off means off (no comm_* launch), a one-rank context records nothing, and the kernel groups count the same launches either way;
  * two ranks sharing the GPU (host-staged exchange over gloo): PrimRun.comm_stats on both ranks, and bin/preqx's HommeTime_stats rows;
  * two devices, where two are visible: bench.py on 2 GPUs over RCCL against 1 GPU, and the groups on both ranks of a real RCCL run.
Every case runs in child processes of its own (this file with --worker), each under a time limit."""
import hashlib
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
COMM = ("comm_pack_q", "comm_pack_mm", "comm_exchange_q", "comm_exchange_mm", "comm_unpack_q", "comm_unpack_mm", "comm_wait")
KERNELS = ("advance0", "advance1", "advance2", "lap", "dss", "minmax", "remap", "level", "dcmip", "avg")


# ---------------------------------------------------------------------------------------------------------------------------
# worker side (a child process)
def _loopback(ne, qsize, world, rank, limiter=8):
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.driver import NU_Q, TSTEP, partition
    from transport_se_amd.hip_mod import HipMod
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord()
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    d = cm.edge_descriptors(topo, partition(ne, world), rank)
    mine = d["elems"]
    sched = dict(send=[(0, p, l) for (_, p, l) in d["send"]], recv=[(0, p, l) for (_, p, l) in d["recv"]])
    elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    h = HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), qsize, NU_Q[ne], device=0, schedule=sched, limiter_option=limiter)
    h.comm_init(HipMod.comm_unique_id(), 0, 1)
    h.dcmip_init(1, geo["lat"][mine], geo["lon"][mine], hv.hyam, hv.hybm)
    h.dcmip_set_initial()
    return h, int(mine.size), TSTEP[ne]


def _comm(h):
    return {k: list(h.kernel_time(k)) for k in COMM}


def _bits(h, n, qsize):
    h.synchronize()
    return [hashlib.sha256(h.fetch("qdp%d" % tl, (n, qsize, 72, 16)).tobytes()).hexdigest() for tl in (1, 2)]


def _groups_job(spec):
    """comm_* per tracer step (tse_advec_tracers_remap_rk2: no prefetch) and per remap cycle (tse_prim_run_subcycle)"""
    h, _, tstep = _loopback(8, 4, 4, 1, spec["limiter"])
    h.comm_timing(True)
    steps = []
    for n in range(3):
        n0 = 1 + n % 2
        h.dcmip_step_inputs(n, tstep)
        h.advec_tracers_remap_rk2(tstep, n0, 3 - n0)
        steps.append(_comm(h))
        h.comm_timing(True)                       # (resets the comm_* groups)
    h.vertical_remap(3 * tstep, 2)
    nstep, cycles = 3, []
    for _ in range(3):
        nstep = h.prim_run_subcycle(tstep, 1, nstep)
        cycles.append(_comm(h))
        h.comm_timing(True)
    h.close()
    return dict(steps=steps, cycles=cycles)


def _routes(h, n, qsize, tstep, comm_on, timing_on):
    """Qdp bits + comm_* / kernel-group launches of three routes from the initial state: the split route (tse_prim_run_subcycle, two
    cycles), the whole-step call with one DSS pass per stage (TSE_DSS_ON_READ=0) and the per-stage API; the switches stay as set"""
    out = {}

    def take(route):
        bits = _bits(h, n, qsize)
        out[route] = dict(bits=bits, comm=_comm(h), kernels={k: h.kernel_time(k)[1] for k in KERNELS})
        h.comm_timing(comm_on); h.timing(timing_on)   # (reset both)
    h.dcmip_set_initial()
    assert h.prim_run_subcycle(tstep, 2, 0) == 6
    take("split")
    h.dcmip_set_initial(); h.dcmip_step_inputs(0, tstep)
    os.environ["TSE_DSS_ON_READ"] = "0"
    try:
        h.advec_tracers_remap_rk2(tstep, 1, 2)
    finally:
        os.environ.pop("TSE_DSS_ON_READ")
    take("whole_step_per_stage_dss")
    h.dcmip_set_initial(); h.dcmip_step_inputs(0, tstep); h.compute_divdp()
    h.euler_step(2, 1, tstep / 2, 3, 0); h.euler_step(2, 2, tstep / 2, 1, 1); h.euler_step(2, 2, tstep / 2, 2, 2); h.qdp_time_avg(3, 1, 2)
    take("per_stage_api")
    return out


def _bits_job(spec):
    out = {}
    for mode in ("off", "comm", "comm+timing", "timing"):
        h, n, tstep = _loopback(8, 4, 4, 1, spec["limiter"])
        comm_on, timing_on = "comm" in mode, "timing" in mode
        h.comm_timing(comm_on); h.timing(timing_on)
        out[mode] = _routes(h, n, 4, tstep, comm_on, timing_on)
        h.close()
    # one rank: no halo, nothing to time
    from transport_se_amd.driver import PrimRun
    r = PrimRun(4, 2, world=1)
    r.hip.comm_timing(True); r.hip.timing(True)
    r.run(6)
    out["one_rank"] = dict(comm=_comm(r.hip), advance=r.hip.kernel_time("advance")[1])
    r.close()
    return out


def _ranks_job(spec):
    """one rank of a torch.distributed.run job: PrimRun with comm timing on; rank 0 writes every rank's comm_stats"""
    import torch
    import torch.distributed as dist
    from transport_se_amd.driver import PrimRun
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    local = int(os.environ.get("LOCAL_RANK", "0")) if spec["exchange"] == "rccl" else 0
    torch.cuda.set_device(local)
    dist.init_process_group("gloo")
    r = PrimRun(spec["ne"], spec["qsize"], rank=dist.get_rank(), world=dist.get_world_size(), device=local, dist_mod=dist, torch_mod=torch,
                exchange=spec["exchange"])
    r.hip.comm_timing(True)
    r.run(spec["steps"])
    st = r.comm_stats()
    if dist.get_rank() == 0:
        with open(spec["out"], "w") as f:
            json.dump(dict(exchange=r.exchange_kind, note=r.exchange_note, ranks=st["ranks"], max=st["max"]), f)
    r.close()
    dist.barrier()
    dist.destroy_process_group()
    return None


def _worker(spec):
    kind = spec["kind"]
    out = dict(groups=_groups_job, bits=_bits_job, ranks=_ranks_job)[kind](spec)
    if out is not None:
        with open(spec["out"], "w") as f:
            json.dump(out, f)


# ---------------------------------------------------------------------------------------------------------------------------
# test side
def _env():
    env = dict(os.environ, GLOO_SOCKET_IFNAME="lo")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def _child(spec, tmp_path, timeout=300):
    out = str(tmp_path / ("%s.json" % spec["kind"]))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(dict(spec, out=out))], env=_env(), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    return json.load(open(out))


def _ranks(spec, world, tmp_path, timeout=300):
    out = str(tmp_path / ("ranks_%s.json" % spec["exchange"]))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.abspath(__file__), "--worker", json.dumps(dict(spec, kind="ranks", out=out))],
                         env=_env(), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert res.returncode == 0, res.stdout.decode()[-4000:]
    return json.load(open(out))


def _launches(d):
    return {k: v[1] for k, v in d.items()}


@pytest.mark.parametrize("limiter", [8, 0])
def test_comm_groups_in_rccl_loopback(tmp_path, limiter):
    r = _child(dict(kind="groups", limiter=limiter), tmp_path)
    for d in r["steps"] + r["cycles"]:
        for k in ("comm_pack_q", "comm_exchange_q", "comm_unpack_q"):
            assert d[k][1] > 0 and d[k][0] > 0, (k, d)
        assert d["comm_wait"][1] > 0 and d["comm_wait"][0] >= 0, d
        for k in ("comm_pack_mm", "comm_exchange_mm", "comm_unpack_mm"):
            assert (d[k][1] > 0) == (limiter == 8), (k, limiter, d)
    # the same launches on every tracer step, and on every cycle whose bounds exchange the previous cycle's remap prefetched
    assert _launches(r["steps"][0]) == _launches(r["steps"][1]) == _launches(r["steps"][2]), r["steps"]
    assert _launches(r["cycles"][1]) == _launches(r["cycles"][2]), r["cycles"]
    # one tracer step: 4 tracer halo exchanges (3 main DSS messages + the Laplacian's), one exposed wait after each of the 4 split stages
    # and one where stage 1 consumes the bounds
    assert r["steps"][0]["comm_exchange_q"][1] == 4
    assert r["steps"][0]["comm_exchange_mm"][1] == (2 if limiter == 8 else 0)
    assert r["steps"][0]["comm_wait"][1] == (5 if limiter == 8 else 4)


def test_comm_timing_leaves_the_bits_and_the_kernel_groups_alone(tmp_path):
    r = _child(dict(kind="bits", limiter=8), tmp_path)
    routes = ("split", "whole_step_per_stage_dss", "per_stage_api")
    for route in routes:
        for mode in ("comm", "comm+timing", "timing"):
            assert r[mode][route]["bits"] == r["off"][route]["bits"], (route, mode)
        for mode in ("comm", "comm+timing"):
            # (the compute-stream routes have no bounds unpack: their neighbour min/max pass reads the received bounds in place)
            used = COMM if route == "split" else [k for k in COMM if k != "comm_unpack_mm"]
            assert all(r[mode][route]["comm"][k][1] > 0 for k in used), (route, mode, r[mode][route]["comm"])
            assert route == "split" or r[mode][route]["comm"]["comm_unpack_mm"][1] == 0
        for mode in ("off", "timing"):
            assert all(v == [0.0, 0] for v in r[mode][route]["comm"].values()), (route, mode, r[mode][route]["comm"])
        assert r["comm+timing"][route]["kernels"] == r["timing"][route]["kernels"], route
        assert r["timing"][route]["kernels"]["advance0"] > 0
        assert all(v == 0 for v in r["comm"][route]["kernels"].values()), route   # (comm timing alone starts no kernel timer)
    # on the compute-stream routes the whole exchange is exposed: one comm_wait per pack -> exchange -> unpack sequence
    pst = r["comm"]["per_stage_api"]["comm"]
    assert pst["comm_wait"][1] == pst["comm_exchange_q"][1] + pst["comm_exchange_mm"][1]
    assert pst["comm_wait"][0] >= pst["comm_exchange_q"][0] + pst["comm_exchange_mm"][0]
    assert all(v == [0.0, 0] for v in r["one_rank"]["comm"].values()) and r["one_rank"]["advance"] > 0, r["one_rank"]


def test_comm_stats_on_two_staged_ranks_sharing_the_gpu(tmp_path):
    r = _ranks(dict(exchange="staged", ne=8, qsize=4, steps=6), 2, tmp_path)
    assert r["exchange"] == "staged" and len(r["ranks"]) == 2
    for rank in r["ranks"]:
        assert all(rank[k][1] > 0 for k in COMM), rank
        assert rank["comm"][1] == sum(rank[k][1] for k in COMM)
    assert all(r["max"][k][1] == max(x[k][1] for x in r["ranks"]) for k in COMM)


NL = """
&ctl_nl
  test_case = "dcmip1-1"
  ne = 8
  qsize = 4
  nmax = 6
  statefreq = 3
  tstep = 400
  qsplit = 1, rsplit = 3
  nu_q = 6e16
  limiter_option = 8
  hypervis_order = 2
/
&vert_nl
  vfile_mid = "vcoord/acme-72m.ascii"
  vfile_int = "vcoord/acme-72i.ascii"
/
"""


def test_preqx_on_two_staged_ranks_writes_the_exchange_rows(tmp_path):
    def run(args, env_extra):
        env = _env(); env.update(env_extra)
        res = subprocess.run([os.path.join(ROOT, "bin", "preqx")] + args, input=NL.encode(), cwd=str(tmp_path), env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        out = res.stdout.decode()
        assert res.returncode == 0, out[-3000:]
        rows = [l.split() for l in open(os.path.join(str(tmp_path), "HommeTime_stats")).read().splitlines()[1:]]
        return [l for l in out.splitlines() if l.startswith(("DCMIP", "Q", "qv= ")) and "wall" not in l], rows
    four = ["prim_run", "prim_advance_exp", "prim_advec_tracers_remap_rk2", "vertical_remap"]
    one, rows1 = run([], {})
    assert [r[0] for r in rows1] == four
    two, rows2 = run(["--gpus", "2"], {"TSE_EXCHANGE": "staged"})
    assert two == one and len(one) >= 1 + 4 + 4
    assert [r[0] for r in rows2] == four + ["bndry_exchange", "bndry_exchange_wait"]
    for r in rows2:
        assert r[1] == "2" and int(r[3]) > 0 and float(r[4]) >= float(r[5]) >= float(r[6]) >= 0, r
    assert float(rows2[4][4]) > 0


def _device_count():
    res = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], env=_env(), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=120)
    return int(res.stdout.decode().strip().splitlines()[-1])


def test_two_devices_over_rccl(tmp_path):
    ndev = _device_count()
    if ndev < 2:
        pytest.skip("needs two visible GPUs (%d visible)" % ndev)

    def bench(gpus):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--ne", "30", "--qsize", "35", "--steps", "6",
                              "--warmup", "3", "--no-cpu-baseline"], env=_env(), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = res.stdout.decode()
        assert res.returncode == 0, out[-3000:]
        return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    b2, b1 = bench(2), bench(1)
    assert b2["exchange"] == "rccl" and b2["world_size"] == 2 and "exchange_note" not in b2, b2
    assert b2["state_checksum"] == b1["state_checksum"]
    r = _ranks(dict(exchange="rccl", ne=8, qsize=4, steps=6), 2, tmp_path)
    assert r["exchange"] == "rccl" and r["note"] is None
    for rank in r["ranks"]:
        assert all(rank[k][1] > 0 for k in COMM), rank


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--worker":
    sys.path.insert(0, ROOT)
    _worker(json.loads(sys.argv[2]))
