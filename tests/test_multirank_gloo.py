"""N>1 path on CPU: world_size-2 (and 3) torch.distributed/gloo runs of the bndry_exchangeV replacement
(transport_se_amd.driver.HaloExchange: one isend + one irecv per neighbour-rank slot) wrapped around a numpy emulation
of the library's pack (k_pack) and gather-DSS (k_dss) that uses the SAME host tables the library builds from the
reference-style descriptors (send_src and dss_tab of csrc/tse_tables.cpp, read through the hooks library in the parent
process).  Result must equal the single-rank DSS bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from host_tables import host_tables
from transport_se_amd import cube_mesh as cm
from transport_se_amd.driver import HaloExchange, check_schedules_match, partition

NE, NLYR = 4, 5


def _worker(rank, world, port, field, ref, send_src, dss_tab, ncol_recv, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    topo = cm.topology(NE)
    owner = partition(NE, world)
    desc = cm.edge_descriptors(topo, owner, rank)
    mine = desc["elems"]
    f = field[mine]                                               # [nelemd][NLYR][16]
    sendbuf = np.zeros((len(send_src), NLYR)); recvbuf = np.zeros((ncol_recv, NLYR))
    for c, (e, p) in enumerate(send_src):                         # k_pack
        sendbuf[c] = f[e, :, p]
    # entries of the compact min/max exchange per slot = (element, direction) pairs whose first column lies in the slot (tse_init)
    starts = sorted(int(c) for c in desc["putmapP"].reshape(-1) if c >= 0)
    mm = [sum(1 for c in starts if ptr - 1 <= c < ptr - 1 + ln) for (_, ptr, ln) in desc["send"]]
    check_schedules_match(desc, (mm, mm), rank, dist)            # raises on any asymmetry between the ranks' slot lists
    ex = HaloExchange(desc, "cpu", dist, torch)
    assert ex(sendbuf.ctypes.data, recvbuf.ctypes.data, NLYR) == 0
    out = f.copy()                                                # k_dss: gather in the reference's order (S, E, N, W, corners),
    for e in range(mine.size):                                    # which is the order of a point's contributions in dss_tab
        for p in range(16):
            for (x, y) in dss_tab[e, p]:                          # local {element, point}, -1 none, <= -2 received column -(x+2)
                if x != -1:
                    out[e, :, p] += recvbuf[-(x + 2)] if x <= -2 else f[x, :, y]
    ok = np.array_equal(out, ref[mine])
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_halo_exchange_gloo(world):
    topo = cm.topology(NE)
    rng = np.random.default_rng(3)
    field = rng.uniform(size=(6 * NE * NE, NLYR, 16))
    ref = np.stack([cm.dss_sum(field[:, l], topo) for l in range(NLYR)], 1)
    owner = partition(NE, world)
    tabs = [host_tables(cm.edge_descriptors(topo, owner, r)) for r in range(world)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 1000 + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, field, ref, tabs[r]["send_src"].copy(),
                                               tabs[r]["dss_tab"].reshape(-1, 16, 3, 2).copy(), tabs[r]["ncol_recv"], q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert res == [(r, True) for r in range(world)]
