"""The host tables of tse_init (csrc/tse_tables.cpp: build_tables) on the CPU, through the test entry of the -DTSE_AB_HOOKS library:
what the kernels rely on, for single- and multi-rank descriptors, with the regular tiling and with the boundary bands
(TSE_BOUNDARY_STRIPS)."""
import numpy as np
import pytest

from host_tables import host_tables
from transport_se_amd import cube_mesh as cm
from transport_se_amd.driver import partition

PS, NRMAX, NER = 16, 96, 48                    # tse_layout.h
LDS_SLOT = 20
LDS_RING = PS * LDS_SLOT
LDS_ZERO = LDS_RING + NRMAX

# (ne, ranks): every rank of each
CASES = [(2, 1), (4, 1), (8, 1), (8, 2), (8, 3), (30, 1), (30, 8)]


def restated_send_src(desc):
    """the send columns' sources restated from putmapP/reverse + the send slots: (element, point) per column in slot order"""
    put, rev = desc["putmapP"], desc["reverse"]
    own = {}
    for e in range(put.shape[0]):
        for d in range(8):
            if put[e, d] < 0:
                continue
            if d < 4:
                for k in range(4):
                    own[put[e, d] + (3 - k if rev[e, d] else k)] = (e, cm.edge_point(d, k))
            else:
                own[put[e, d]] = (e, cm.CORNER_POINT[d])
    return [own[ptr - 1 + i] for (_, ptr, ln) in desc["send"] for i in range(ln)]


def ppos(perm, p):
    return (perm >> np.uint64(4 * p)) & np.uint64(15)


def check(desc, t):
    n = desc["putmapP"].shape[0]
    nslots, npatch = t["nslots"], t["npatch"]
    assert nslots == npatch * PS and t["zero0"] == nslots * 16 and t["halo0"] == (nslots + 1) * 16
    assert t["cse"] == (nslots + 1) * 16 + t["ncol_recv"]
    assert (t["send_len"].sum(), t["recv_len"].sum()) == (t["ncol_send"], t["ncol_recv"])
    assert (t["mm_send_len"].sum(), t["mm_recv_len"].sum()) == (t["nmm_send"], t["nmm_recv"])
    send_src, mm_src, tab, nbr = t["send_src"], t["mm_send_src"], t["dss_tab"].reshape(n, 48, 2), t["nbr"].reshape(n, 8)

    # walk order and the boundary split
    assert np.array_equal(np.sort(t["order"]), np.arange(n))
    bnd, inn = t["ord_bnd"], t["ord_int"]
    assert (bnd.size, inn.size) == (t["n_bnd"], t["n_int"])
    assert np.array_equal(np.sort(np.concatenate([bnd, inn])), np.arange(n))
    owners = np.union1d(send_src[:, 0], mm_src[:, 0]) if send_src.size or mm_src.size else np.zeros(0, dtype=np.int32)
    assert np.array_equal(bnd, owners)
    isb = np.zeros(n, dtype=bool); isb[bnd] = True

    # one slot per element
    slot_of, pslots = t["slot_of"], t["pslots"]
    assert pslots.size == nslots and np.array_equal(pslots[slot_of], np.arange(n))
    assert np.count_nonzero(pslots >= 0) == n

    # point order: every word a permutation of 0..15
    pperm = t["pperm"]
    pos = np.stack([ppos(pperm, p) for p in range(16)], 1).astype(np.int64)   # [slot][p]
    assert np.array_equal(np.sort(pos, 1), np.broadcast_to(np.arange(16), pos.shape))

    # etab = dss_tab as entries within a chunk
    x, y = tab[..., 0].astype(np.int64), tab[..., 1].astype(np.int64)
    loc = x >= 0
    want = np.where(x == -1, t["zero0"], t["halo0"] + (-(x + 2)))
    want[loc] = slot_of[x[loc]] * 16 + pos[slot_of[x[loc]], y[loc]]
    etab = t["etab"].reshape(n, 48).astype(np.int64)
    assert np.array_equal(etab, want)
    assert np.all(-(x[x <= -2] + 2) < t["ncol_recv"])

    # halo rings: plds resolves (own -> lds_own_entry, ring -> pring, empty -> LDS_ZERO) to the entry etab names
    plds = t["plds"].reshape(npatch, PS, 48).astype(np.int64)
    pring = t["pring"].reshape(npatch, NRMAX).astype(np.int64)
    pi = np.arange(npatch)[:, None, None]
    own = plds < LDS_RING
    sl, w = plds // LDS_SLOT, plds % LDS_SLOT
    assert np.all(w[own] < 16)
    j = w >> 2
    p = 4 * j + (((w & 3) - j) & 3)
    oslot = np.where(own, pi * PS + sl, 0)
    got = np.full(plds.shape, -1, dtype=np.int64)
    got[own] = oslot[own] * 16 + pos[oslot[own], p[own]]
    ring = (plds >= LDS_RING) & (plds < LDS_ZERO)
    got[ring] = pring[np.broadcast_to(pi, plds.shape)[ring], plds[ring] - LDS_RING]
    got[plds == LDS_ZERO] = t["zero0"]
    assert np.all(plds <= LDS_ZERO)
    live = pslots.reshape(npatch, PS) >= 0
    assert np.all(plds[~live] == LDS_ZERO)
    assert np.array_equal(got[live], etab[pslots.reshape(npatch, PS)[live]])
    assert np.all(pslots[oslot[own]] >= 0)   # own entries name slots of the patch that hold an element
    for q in range(npatch):
        used = np.unique(plds[q][(plds[q] >= LDS_RING) & (plds[q] < LDS_ZERO)]) - LDS_RING
        assert used.size <= NRMAX and np.array_equal(used, np.arange(used.size))   # entries in order of first use
        assert np.all(pring[q, used.size:] == t["zero0"])

    # lines a slot must store: pexp covers every position a halo ring or a send column reads
    pexp = t["pexp"].astype(np.int64)
    assert pexp.size == nslots
    rd = pring[pring < nslots * 16]
    assert np.all(pexp[rd // 16] > (rd % 16) // 4)
    ss = t["send_src_s"].astype(np.int64)
    assert ss.shape == send_src.shape
    if ss.size:
        assert np.array_equal(ss[:, 0], slot_of[send_src[:, 0]])
        assert np.array_equal(ss[:, 1], pos[ss[:, 0], send_src[:, 1]])
        assert np.all(pexp[ss[:, 0]] > ss[:, 1] // 4)

    # neighbours: local links are mutual, remote ones index the received min/max entries
    for e, d in zip(*np.nonzero(nbr >= 0)):
        assert e in nbr[nbr[e, d]], (e, d)
    assert np.all(-(nbr[nbr <= -2] + 2) < t["nmm_recv"])
    # pnb / pering agree with nbr, and the element ring fits
    pnb = t["pnb"].reshape(npatch, PS, 8).astype(np.int64)
    pering = t["pering"].reshape(npatch, NER).astype(np.int64)
    ps2 = pslots.reshape(npatch, PS)
    for q in range(npatch):
        assert np.unique(pnb[q][(pnb[q] >= PS) & (pnb[q] != 255)]).size <= NER
        for i in np.flatnonzero(ps2[q] >= 0):
            e = ps2[q, i]
            for d in range(8):
                nb, v = nbr[e, d], pnb[q, i, d]
                if nb == -1:
                    assert v == 255
                elif v < PS:
                    assert ps2[q, v] == nb
                else:
                    assert PS <= v < PS + NER and pering[q, v - PS] == (nb if nb >= 0 else n + (-(nb + 2)))

    # boundary / interior patches, the remap's block lists in slot order
    hasb = np.array([isb[ps2[q][ps2[q] >= 0]].any() for q in range(npatch)], dtype=bool)
    assert np.array_equal(t["plist_bnd"], np.flatnonzero(hasb)) and np.array_equal(t["plist_int"], np.flatnonzero(~hasb))
    assert (t["np_bnd"], t["np_int"]) == (t["plist_bnd"].size, t["plist_int"].size)
    rl = t["rl_all"]
    assert np.array_equal(np.sort(rl), np.arange(n)) and np.all(np.diff(slot_of[rl]) > 0)
    assert np.array_equal(t["rl_bnd"], rl[isb[rl]]) and np.array_equal(t["rl_int"], rl[~isb[rl]])

    # the send columns, as the gloo test used to restate them
    assert [tuple(s) for s in send_src.tolist()] == restated_send_src(desc)


@pytest.mark.parametrize("strips", [False, True], ids=["regular", "bands"])
@pytest.mark.parametrize("ne,world", CASES)
def test_host_tables(ne, world, strips):
    topo = cm.topology(ne)
    owner = partition(ne, world)
    for rank in range(world):
        desc = cm.edge_descriptors(topo, owner, rank)
        check(desc, host_tables(desc, strips))


# ---- the guard of tse_remap_q_ppm: check_remap_grids (csrc/tse_tables.cpp) ----
def _grids(nlev=72, nelem=3, seed=3):
    rng = np.random.default_rng(seed)
    dp1 = 1000.0 * (1 + 0.2 * rng.random((nelem, nlev, 4, 4)))
    dp2 = dp1 * (1 + 0.05 * (rng.random(dp1.shape) - 0.5))
    dp2 *= dp1.sum(1, keepdims=True) / dp2.sum(1, keepdims=True)
    return dp1, dp2


def _serial_sum(x):
    run = np.zeros_like(x[0])
    for k in range(x.shape[0]):
        run = run + x[k]
    return run


@pytest.mark.parametrize("nlev", [72, 64, 16])
def test_remap_grid_guard_accepts_a_good_grid(nlev):
    from host_tables import check_remap_grids
    dp1, dp2 = _grids(nlev)
    assert check_remap_grids(dp1, dp2) is None
    assert check_remap_grids(dp1, dp1) is None                     # every interface a tie
    z = dp2.copy(); z[1, 5, 2, 3] = 0.0                            # an empty target layer is a grid the search ends on
    assert check_remap_grids(dp1, z) is None


@pytest.mark.parametrize("kind", ["dp1 zero", "dp1 negative", "dp1 nan", "dp2 negative", "dp2 nan", "dp2 inf", "dp2 too long"])
def test_remap_grid_guard_names_the_first_offender(kind):
    """element, column (4*j + i) and level of the first bad entry in scan order, all counted from 0, in the message as well"""
    from host_tables import check_remap_grids
    dp1, dp2 = _grids()
    e, k, j, i = 1, 40, 2, 1
    if kind.startswith("dp1"):
        dp1[e, k, j, i] = {"dp1 zero": 0.0, "dp1 negative": -3.0, "dp1 nan": np.nan}[kind]
        dp1[2, 3, 0, 0] = -1.0                                     # a later offender is not the one reported
    elif kind == "dp2 too long":
        dp2[e, k, j, i] += dp2[e, k + 1:, j, i].sum() + 2.0        # the partial sum at level k reaches sum(dp1) + 1
        dp2[e, 50, j, i] = -1.0                                    # (later in the same column)
    else:
        dp2[e, k, j, i] = {"dp2 negative": -1e-300, "dp2 nan": np.nan, "dp2 inf": np.inf}[kind]
    where, msg = check_remap_grids(dp1, dp2)
    assert where == (e, 4 * j + i, k), (where, msg)
    assert "element %d, column %d, level %d" % (e, 4 * j + i, k) in msg and kind.split()[0] in msg, msg


def test_remap_grid_guard_at_the_exact_boundary():
    """a partial sum of dp2 below the last level is refused from sum(dp1) + 1 on (both in fp64, serial order), not before"""
    from host_tables import check_remap_grids
    nlev = 72
    dp1 = np.full((1, nlev, 4, 4), 1024.0)                         # sums exact in fp64: sum(dp1) + 1 = 73729
    end = float(_serial_sum(dp1[0])[0, 0]) + 1.0
    assert end == 73729.0
    dp2 = dp1.copy()
    dp2[0, 10, 1, 1] = end - 10 * 1024.0                           # pin(12) == sum(dp1) + 1 exactly
    where, msg = check_remap_grids(dp1, dp2)
    assert where == (0, 5, 10) and "73729" in msg, (where, msg)
    dp2[0, 10, 1, 1] = np.nextafter(end, 0.0) - 10 * 1024.0        # pin(12) one ulp below it: the search ends (at pio(nlev+2))
    assert float(_serial_sum(dp2[0, :11])[1, 1]) == np.nextafter(end, 0.0)
    dp2[0, 11:, 1, 1] = 0.0
    assert check_remap_grids(dp1, dp2) is None
    dp2[0, nlev - 1, 1, 1] = 1e9                                   # the last level's sum is replaced by pio(nlev+1): never compared
    assert check_remap_grids(dp1, dp2) is None


def test_remap_grid_guard_refuses_a_column_whose_sentinel_is_absorbed():
    """from sum(dp1) = 2^53 on, sum(dp1) + 1 == sum(dp1): the last level searches for an entry above pin(nlev+1) = pio(nlev+1) and
    pio(nlev+2) is not one.  Refused with the column named, whatever dp2 is; one ulp-step below 2^53 the sentinel holds"""
    from host_tables import check_remap_grids
    nlev = 72
    dp1 = np.ones((2, nlev, 4, 4)); dp2 = np.ones((2, nlev, 4, 4))
    dp1[1, 0, 3, 2] = 2.0 ** 54; dp2[1, 0, 3, 2] = 2.0 ** 53
    where, msg = check_remap_grids(dp1, dp2)
    assert where == (1, 14, nlev - 1) and "element 1, column 14" in msg and "sum(dp1)" in msg, (where, msg)
    assert check_remap_grids(dp1, dp1)[0] == (1, 14, nlev - 1)
    dp1[1, 0, 3, 2] = 2.0 ** 53 - (nlev - 1)                      # sum(dp1) == 2^53 exactly: still absorbed
    assert float(_serial_sum(dp1[1])[3, 2]) == 2.0 ** 53
    assert check_remap_grids(dp1, dp1)[0] == (1, 14, nlev - 1)
    dp1[1, 0, 3, 2] = 2.0 ** 53 - nlev                            # sum(dp1) == 2^53 - 1: + 1 is exact and larger
    assert check_remap_grids(dp1, dp1) is None
