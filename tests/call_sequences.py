"""Call sequences against a fresh context: the harness and the vocabulary of tests/test_gpu_call_sequences.py.

The property:  THE VISIBLE STATE AFTER A CALL, AND EVERYTHING THE CALL RETURNS, DEPEND ONLY ON THE VISIBLE STATE BEFORE IT, NEVER ON HOW THE
CONTEXT GOT THERE.  tse_ctx (csrc/tse_ctx.h) carries hidden state that decides what the next call launches -- the cached element bounds and
their prefetched halo, the freshness of Q / lnps, dcmip_static, a deferred final DSS, T's zero slots, the forked step inputs, the twin level
buffers, the qmin/qmin2 swaps, the size of the view staging field (DESIGN.md section 5 tabulates who sets and who drops each) -- and every
public entry has to set or drop the right subset.  replay() walks a sequence of calls on one warm context A and repeats every single call on a
fresh context B that was given A's visible state (load: the writes through tse_device_ptr, then tse_invalidate_cache, which the header
prescribes for exactly this, then tse_dcmip_init); A and B must then agree in every bit of the visible state and of what the call returned.

Visible state = what include/transport_se_hip.h documents as state: the tse_device_ptr fields FIELDS (qmin / qmax are the module state of
prim_advection_mod a rhs_multiplier = 1 stage reads from the stage before) and the scalars only the host knows (SCALARS).

This module is plain Python: nothing of HIP, torch or the library is imported before a device context is made.  The CPU tests
(test_call_sequences_cpu.py) run replay() on a numpy stand-in with planted errors and hold the generator to full pair coverage."""
import contextlib
import ctypes as C
import functools
import os
import threading

import numpy as np

# ---- the vocabulary ----------------------------------------------------------------------------------------------------------------------
KINDS = ("S", "S0", "P", "P1", "R", "C", "C2", "CU", "H", "Q", "F", "FH", "VQ", "VD", "VO", "G", "RV", "DV", "M", "I", "X")
# kinds that change no bit of the visible state (only hidden state, or nothing)
NOOP_KINDS = ("VQ", "VD", "VO", "I", "M", "G", "DV")
FIELDS = ("qdp1", "qdp2", "vn0", "dp", "divdp", "divdp_proj", "eta_dot_dpdn", "omega_p", "dp3d", "ps_v", "qmin", "qmax")
SCALARS = ("dcmip_case", "nstep", "last")   # the prescribed case, tl%nstep, and the time level of Qdp last written (n0 / np1 follow from nstep)

# The hand-written list: today's pairwise tests restated (the test each comes from is named), then the regression cases of what the sequences
# exposed.  Every name is a test id; a sequence starts from the state dcmip_set_initial leaves.
HAND = {
    # test_gpu_bounds_probe.py part (c): cached against recomputed bounds
    "step-step": ("S", "S"),
    "cycle-invalidate-step": ("C", "I", "S"),
    "step-invalidate-step": ("S", "I", "S"),
    "cycle-step": ("C", "S"),
    # test_operator_call_does_not_leave_its_dp_behind (test_gpu_parity.py)
    "operator-cycle": ("C", "Q", "C"),
    "operator-step": ("S", "Q", "S", "R"),
    # test_put_has_the_side_effects_of_the_host_entries (test_gpu_views.py)
    "put-dp-cycle": ("S", "VD", "C"),
    "put-qdp-step": ("S", "VQ", "S", "G"),
    "put-omega-step": ("S", "VO", "S"),
    # the static-inputs test of test_gpu_dcmip_pointwise.py: dp / omega_p are rewritten after another writer
    "host-winds-cycle": ("S", "H", "C"),
    "cycle-host-winds": ("C", "H", "S"),
    # test_chunking_of_the_run_does_not_move_a_bit (test_gpu_parity.py): a cycle entered in its middle, two cycles in one call
    "chunked-run": ("S", "C", "S", "S", "C2", "C"),
    # the per-stage route beside the whole-step route: T's zero slots, the twin level buffers, the carried qmin / qmax
    "stages-step": ("P", "S"),
    "stages-cycle": ("P", "C", "P", "CU"),
    "stage2-after-step": ("S", "P1", "S"),
    "stage2-after-cycle": ("C", "P1", "C"),
    "per-stage-route-cycle": ("S0", "C", "S0", "S"),
    "unfused-remap": ("S", "CU", "S", "R", "S"),
    # forcing and the view entries that write or may write Qdp
    "forcing-step": ("S", "F", "S", "FH", "C"),
    "remap-view-step": ("S", "RV", "S", "RV", "C"),
    # reads and the entries that touch no state
    "reads": ("S", "M", "S", "G", "C", "M", "G", "DV", "S", "DV", "C"),
    "initial-again": ("C", "X", "S", "X", "C"),
    # Regression cases: what the sequences exposed.
    # tse_dcmip_step_inputs replacing a dp that is not the prescribed one (after set_derived / remap_q_ppm) kept the element bounds a step
    # or a remap had emitted with that other dp: the next step's first stage then limited against stale bounds.  host-winds-cycle and
    # cycle-host-winds above failed the same way (H C, H S; also H S0, H CU, H C2 in the random sequences).
    "foreign-dp-remap-step": ("S", "Q", "R", "M", "S0"),
    "foreign-dp-step-step": ("C", "H", "S0", "H", "CU", "H", "C2"),
}


def _random_sequence(seed, covered, length=20):
    """a seeded random walk over KINDS that prefers a successor whose ordered pair with the op before is not in `covered` yet (where every
    pair from that op is covered: one that still has uncovered successors of its own); the pairs it walks are added to `covered`"""
    rng = np.random.default_rng(seed)
    open_from = lambda a: [b for b in KINDS if (a, b) not in covered]   # noqa: E731
    starts = [a for a in KINDS if open_from(a)] or list(KINDS)
    seq = [starts[int(rng.integers(len(starts)))]]
    while len(seq) < length:
        pool = open_from(seq[-1]) or [b for b in KINDS if open_from(b)] or list(KINDS)
        nxt = pool[int(rng.integers(len(pool)))]
        covered.add((seq[-1], nxt))
        seq.append(nxt)
    return tuple(seq)


def pairs_of(seq):
    return set(zip(seq[:-1], seq[1:]))


@functools.lru_cache(maxsize=None)
def sequences():
    """{name: tuple of op kinds}: HAND, then seeded random sequences of 20 ops, seeds 0, 1, 2 ..., until every ordered pair of kinds is
    adjacent somewhere"""
    out = dict(HAND)
    covered = set()
    for s in out.values():
        covered |= pairs_of(s)
    seed = 0
    while len(covered) < len(KINDS) ** 2:
        out["random-%02d" % seed] = _random_sequence(seed, covered)
        seed += 1
        assert seed < 200, "the generator does not reach full pair coverage"
    return out


def pair_coverage(seqs):
    """[len(KINDS)][len(KINDS)] counts: how often kind b follows kind a directly, over all the sequences"""
    m = np.zeros((len(KINDS), len(KINDS)), dtype=int)
    for s in seqs:
        for a, b in zip(s[:-1], s[1:]):
            m[KINDS.index(a), KINDS.index(b)] += 1
    return m


# ---- snapshot, load, replay: over anything with the context surface ---------------------------------------------------------------------
# A context here is an object with
#   field_names() -> names;  read(name) -> float64 array in the field's logical shape;  write(name, array)
#   scalars() -> dict;  set_scalars(dict);  invalidate_cache();  dcmip_init();  start();  close()
# DeviceCtx below is the library's; the CPU tests bring a numpy stand-in.
def bits(x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.float64:
        return x.view(np.uint64)
    return np.ascontiguousarray(x, dtype=np.int64).view(np.uint64)


def snapshot(ctx):
    """the visible state, bit for bit: every field read afresh (the addresses behind a name move with the twin swaps)"""
    return dict(fields={n: bits(ctx.read(n)).copy() for n in ctx.field_names()}, scalars=dict(ctx.scalars()))


def load(ctx, snap):
    """give a context the visible state `snap`: the fields through their own addresses, then invalidate_cache (the header's rule for a caller
    that writes state behind the library's back), then the prescribed case as the snapshot's context had it"""
    for n, b in snap["fields"].items():
        ctx.write(n, b.view(np.float64))
    ctx.invalidate_cache()
    ctx.set_scalars(snap["scalars"])
    ctx.dcmip_init()


class SequenceMismatch(AssertionError):
    """what: "state" (warm and fresh context differ after the op), "returned" (in what the op returned), "noop" (an op of NOOP_KINDS changed
    the visible state); field: the field, scalar or returned name; index / kind / prev: the op, and the op before it"""

    def __init__(self, what, field, index, kind, prev, where, detail):
        self.what, self.field, self.index, self.kind, self.prev, self.where = what, field, index, kind, prev, where
        head = {"state": "warm and fresh context differ in", "returned": "warm and fresh context return different",
                "noop": "an op that changes no state changed"}[what]
        super().__init__("op %d (%s) after %s: %s %s: %s" % (index, kind, prev if prev is not None else "the start", head, field, detail))


def _first_difference(a, b):
    """(index tuple of the first differing entry, detail text) of two uint64 arrays, or None"""
    if a.shape != b.shape:
        return (), "shapes %s and %s" % (a.shape, b.shape)
    bad = np.argwhere(a != b)
    if bad.size == 0:
        return None
    i = tuple(int(x) for x in bad[0])
    names = {5: "(element, tracer, level, j, i)", 4: "(element, level, j, i)", 3: "(element, j, i)", 2: "(element, entry)"}.get(a.ndim, "index")
    if a.ndim == 5 and a.shape[2] == 2:
        names = "(element, level, component, j, i)"
    return i, "%d of %d entries differ, first at %s = %s: %016x != %016x" % (len(bad), a.size, names, list(i), int(a[i]), int(b[i]))


def _compare(what, got, want, index, kind, prev):
    if sorted(got) != sorted(want):
        raise SequenceMismatch(what, "names", index, kind, prev, (), "%s != %s" % (sorted(got), sorted(want)))
    for name in got:
        d = _first_difference(bits(got[name]), bits(want[name]))
        if d is not None:
            raise SequenceMismatch(what, name, index, kind, prev, d[0], d[1])


def run_op(ctx, kind, ops):
    """-> {name: array or scalar} the op returned (an op that returns nothing: {})"""
    ret = ops[kind](ctx)
    return dict(ret or {})


def replay(make_ctx, seq, ops, keep=False):
    """the sequence on one warm context, every op repeated on a fresh context loaded with the warm one's visible state before the op: both
    must leave the same bits and return the same bits; an op of NOOP_KINDS must besides leave the warm context's state alone.  Raises
    SequenceMismatch.  keep: -> [(snapshot after the op, what it returned)] of the warm context."""
    A = make_ctx()
    kept = []
    try:
        A.start()
        for k, kind in enumerate(seq):
            prev = seq[k - 1] if k else None
            before = snapshot(A)
            ret_a = run_op(A, kind, ops)
            after_a = snapshot(A)
            if kind in NOOP_KINDS:
                _compare("noop", after_a["fields"], before["fields"], k, kind, prev)
            B = make_ctx()
            try:
                load(B, before)
                ret_b = run_op(B, kind, ops)
                after_b = snapshot(B)
            finally:
                B.close()
            _compare("state", after_a["fields"], after_b["fields"], k, kind, prev)
            _compare("state", {n: np.array(v) for n, v in after_a["scalars"].items()}, {n: np.array(v) for n, v in after_b["scalars"].items()},
                     k, kind, prev)
            _compare("returned", ret_a, ret_b, k, kind, prev)
            if keep:
                kept.append((after_a, ret_a))
    finally:
        A.close()
    return kept


def run_warm(ctx, seq, ops, between=None):
    """the sequence on one context alone -> [(snapshot after the op, what it returned)]; between(k): called before and after op k (the
    emulated ranks meet there)"""
    out = []
    ctx.start()
    for k, kind in enumerate(seq):
        if between:
            between(k)
        ret = run_op(ctx, kind, ops)
        if between:
            between(k)
        out.append((snapshot(ctx), ret))
    return out


# ---- the library's context -------------------------------------------------------------------------------------------------------------
NE, QSIZE, NU_Q, RSPLIT = 2, 5, 1e19, 3
# the time step by prescribed case: DCMIP 1-2's vertical motion empties layers within a remap cycle at the 1-1 step (as test_gpu_nlev80.py's TSTEP)
TSTEP = {1: 1800.0, 2: 300.0}

_env_lock = threading.Lock()
_env_depth = {}


@contextlib.contextmanager
def route_env(**switches):
    """the library's route switches for the calls inside (it reads them per call).  Counted, so that the emulated ranks, which all make the
    same call between two meeting points, set a switch once and take it back once."""
    with _env_lock:
        for k, v in switches.items():
            d = _env_depth.setdefault(k, [0, None])
            if d[0] == 0:
                d[1] = os.environ.get(k)
                os.environ[k] = v
            d[0] += 1
    try:
        yield
    finally:
        with _env_lock:
            for k in switches:
                d = _env_depth[k]
                d[0] -= 1
                if d[0] == 0:
                    if d[1] is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = d[1]


@functools.lru_cache(maxsize=None)
def inputs(ne=NE, qsize=QSIZE, nlev=72):
    """every array an op feeds the library, by GLOBAL element (a rank takes its rows): deterministic, made once, never written"""
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.hybvcoord import HvCoord
    hv = HvCoord()
    topo = cm.topology(ne); geo = cm.geometry(ne, topo)
    n, K = 6 * ne * ne, nlev
    lat, lon = np.asarray(geo["lat"]).reshape(n, 4, 4), np.asarray(geo["lon"]).reshape(n, 4, 4)
    dA, dB = np.diff(np.asarray(hv.hyai, dtype=np.float64)), np.diff(np.asarray(hv.hybi, dtype=np.float64))
    lev = np.arange(K) / K
    d = dict(hv=hv, topo=topo, geo=geo, lat=lat, lon=lon)
    # H: smooth winds and layers that are not the prescribed case's (omega_p != 0)
    u = 20.0 * np.cos(lat)[:, None] * (1.0 + 0.1 * lev)[None, :, None, None]
    v = np.broadcast_to((4.0 * np.sin(2 * lon) * np.cos(lat) ** 2)[:, None], u.shape)
    ps = hv.ps0 * (1.0 + 0.01 * np.sin(lon) * np.cos(lat))
    dp = dA[None, :, None, None] * hv.ps0 + dB[None, :, None, None] * ps[:, None]
    ilev = np.arange(K + 1) / K
    d["H"] = dict(vn0=np.ascontiguousarray(np.stack([u, v], axis=2)), dp=np.ascontiguousarray(dp),
                  eta_dot_dpdn=np.ascontiguousarray(1e-2 * np.sin(np.pi * ilev)[None, :, None, None] * (np.cos(lat) * np.cos(lon))[:, None]),
                  omega_p=np.ascontiguousarray(1e-4 * (1.0 + lev)[None, :, None, None] * (np.cos(lat) * np.sin(lon))[:, None]),
                  divdp=np.ascontiguousarray(1e-7 * dp * np.sin(lat)[:, None]), divdp_proj=np.ascontiguousarray(0.9e-7 * dp * np.sin(lat)[:, None]))
    # Q, RV: the grids of test_operator_call_does_not_leave_its_dp_behind
    rng = np.random.default_rng(11)
    dp1 = 1000.0 * (1 + 0.2 * rng.random((n, K, 4, 4)))
    dp2 = dp1 * (1 + 0.05 * (rng.random(dp1.shape) - 0.5)); dp2 *= dp1.sum(1, keepdims=True) / dp2.sum(1, keepdims=True)
    d["Q"] = dict(qdp=rng.random((n, qsize, K, 4, 4)) * dp1[:, None], dp1=dp1, dp2=dp2)
    # F, FH: a tendency of either sign, large enough for the zero clip to act where the tracer is small
    d["F"] = 0.05 * np.random.default_rng(5).standard_normal((n, qsize, K, 4, 4))
    # DV: a host's own interface field and surface field
    rng = np.random.default_rng(7)
    d["DV"] = (rng.standard_normal((n, K + 1, 4, 4)), rng.standard_normal((n, 4, 4)))
    for x in d["H"].values():
        x.setflags(write=False)
    return d


_hip_rt = None


def _hipMemcpy(dst, src, nbytes, kind):
    global _hip_rt
    if _hip_rt is None:
        _hip_rt = C.CDLL("libamdhip64.so")
    rc = _hip_rt.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), C.c_int(kind))
    assert rc == 0, "hipMemcpy (kind %d) failed: %d" % (kind, rc)


class DeviceCtx:
    """one tse_ctx (a whole ne2 mesh, or the rows `mine` of it) with the host's bookkeeping of driver.PrimRun: nstep and the time level
    last written"""

    def __init__(self, hip, mine, case, limiter, inp=None):
        self.hip, self.mine, self.case, self.limiter = hip, np.asarray(mine), int(case), int(limiter)
        self.inp = inp or inputs()
        self.nstep, self.last = 0, 1
        n, q, K = hip.nelemd, hip.qsize, hip.nlev
        self.shapes = dict(qdp1=(n, q, K, 4, 4), qdp2=(n, q, K, 4, 4), vn0=(n, K, 2, 4, 4), eta_dot_dpdn=(n, K + 1, 4, 4), ps_v=(n, 4, 4),
                           qmin=(n, -1), qmax=(n, -1))

    # -- the context surface --
    def field_names(self):
        return FIELDS

    def read(self, name):
        p, nbytes = self.hip.device_ptr(name)
        assert p and nbytes, name
        out = np.empty(nbytes // 8)
        self.hip.synchronize()
        _hipMemcpy(out.ctypes.data, p, nbytes, 2)
        return out.reshape(self.shapes.get(name, (self.hip.nelemd, self.hip.nlev, 4, 4)))

    def write(self, name, x):
        p, nbytes = self.hip.device_ptr(name)
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert p and x.nbytes == nbytes, (name, x.nbytes, nbytes)
        self.hip.synchronize()
        _hipMemcpy(p, x.ctypes.data, nbytes, 1)

    def scalars(self):
        return dict(dcmip_case=self.case, nstep=self.nstep, last=self.last)

    @property
    def tstep(self):
        return TSTEP[self.case]

    def set_scalars(self, s):
        self.case, self.nstep, self.last = int(s["dcmip_case"]), int(s["nstep"]), int(s["last"])

    def invalidate_cache(self):
        self.hip.invalidate_cache()

    def dcmip_init(self):
        i = self.inp
        self.hip.dcmip_init(self.case, i["lat"][self.mine], i["lon"][self.mine], i["hv"].hyam, i["hv"].hybm)

    def start(self):
        self.dcmip_init()
        self.hip.dcmip_set_initial()
        self.nstep, self.last = 0, 1

    def close(self):
        self.hip.close()

    # -- helpers of the ops --
    def levels(self):
        """(n0_qdp, np1_qdp) of the step that starts at nstep (TimeLevel_Qdp, time_mod.F90:85-109)"""
        n0 = 1 if self.nstep % 2 == 0 else 2
        return n0, 3 - n0

    def stepped(self):
        self.last = self.levels()[1]
        self.nstep += 1

    def cycled(self, n):
        self.nstep = n
        self.last = 2 if (n - 1) % 2 == 0 else 1

    def device(self, x):
        """a host array as a device array of its own (torch owns the memory)"""
        import torch
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
        torch.cuda.synchronize()
        return t


def make_hip(limiter, mine=None, schedule=None, exchange=None, descs=None, rsplit=RSPLIT, inp=None):
    """a HipMod of the test's shape on cube_mesh's geometry: the whole mesh, or the rows `mine` with a rank's edge descriptors"""
    from transport_se_amd import cube_mesh as cm
    from transport_se_amd.hip_mod import HipMod
    inp = inp or inputs()
    geo, hv = inp["geo"], inp["hv"]
    d = descs or cm.edge_descriptors(inp["topo"])
    mine = np.arange(geo["metdet"].shape[0]) if mine is None else mine
    elem = dict(Dinv=geo["Dinv"][mine], metdet=geo["metdet"][mine], rmetdet=geo["rmetdet"][mine], spheremp=geo["spheremp"][mine],
                rspheremp=geo["rspheremp"][mine], putmapP=d["putmapP"], getmapP=d["getmapP"], reverse=d["reverse"])
    return HipMod(elem, cm.dvv(), (hv.hyai, hv.hybi, hv.ps0), QSIZE, NU_Q, limiter_option=limiter, rsplit=rsplit, device=0,
                  schedule=schedule or dict(send=d["send"], recv=d["recv"]), exchange=exchange)


def make_device_ctx(limiter, case=1):
    return DeviceCtx(make_hip(limiter), np.arange(6 * NE * NE), case, limiter)


# ---- the ops on a DeviceCtx ------------------------------------------------------------------------------------------------------------
def _step(c):
    n0, np1 = c.levels()
    c.hip.dcmip_step_inputs(c.nstep, c.tstep)
    c.hip.advec_tracers_remap_rk2(c.tstep, n0, np1)
    c.stepped()


def op_S(c):
    _step(c)


def op_S0(c):
    with route_env(TSE_DSS_ON_READ="0"):
        _step(c)


def op_P(c):
    n0, np1 = c.levels()
    h = c.hip
    h.compute_divdp()
    h.euler_step(np1, n0, c.tstep / 2, 3, 0)
    h.euler_step(np1, np1, c.tstep / 2, 1, 1)
    h.euler_step(np1, np1, c.tstep / 2, 2, 2)
    h.qdp_time_avg(3, n0, np1)
    c.stepped()


def op_P1(c):
    c.hip.euler_step(c.last, c.last, c.tstep / 2, 1, 1)


def op_R(c):
    c.hip.vertical_remap(c.tstep * RSPLIT, c.last)


def _cycles(c, nsub):
    n = c.hip.prim_run_subcycle(c.tstep, nsub, c.nstep)
    c.cycled(n)
    return dict(nstep=n)


def op_C(c):
    return _cycles(c, 1)


def op_C2(c):
    return _cycles(c, 2)


def op_CU(c):
    with route_env(TSE_REMAP_FUSED="0"):
        return _cycles(c, 1)


def op_H(c):
    n0, np1 = c.levels()
    f = {k: np.ascontiguousarray(x[c.mine]) for k, x in c.inp["H"].items()}
    c.hip.set_derived(f)
    c.hip.set_divdp(f)
    c.hip.advec_tracers_remap_rk2(c.tstep, n0, np1)
    c.stepped()


def op_Q(c):
    q = c.inp["Q"]
    return dict(qdp=c.hip.remap_q_ppm(q["qdp"][c.mine], q["dp1"][c.mine], q["dp2"][c.mine]))


def op_F(c):
    fq = c.device(c.inp["F"][c.mine])
    return dict(budget=c.hip.apply_forcing(fq, "eqkji", c.last, dt=c.tstep, mode="tendency", budget=True))


def op_FH(c):
    return dict(budget=c.hip.apply_forcing_host(np.ascontiguousarray(c.inp["F"][c.mine]), c.last, c.tstep, "tendency", budget=True))


def op_VQ(c):
    c.hip.put("qdp", c.device(c.read("qdp%d" % c.last)), "eqkji", nt=c.last)


def op_VD(c):
    c.hip.put("dp", c.device(c.read("dp")), "ekji")


def op_VO(c):
    c.hip.put("omega_p", c.device(c.read("omega_p")), "ekji")


def op_G(c):
    h = c.hip
    h.state_q(c.last)
    q = c.device(np.zeros((h.nelemd, h.qsize, h.nlev, 4, 4)))
    lnps = c.device(np.zeros((h.nelemd, 4, 4)))
    h.get("q", q, "eqkji")
    h.get("lnps", lnps, "eji")
    return dict(q=q.cpu().numpy(), lnps=lnps.cpu().numpy())


class _Raw:
    """a dense device array at a raw address, for a view inside the library's own Qdp"""

    def __init__(self, shape, ptr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f8", data=(int(ptr), False), strides=None, version=3)


def op_RV(c):
    h, q = c.hip, c.inp["Q"]
    src, tgt = c.device(q["dp1"][c.mine]), c.device(q["dp2"][c.mine])
    p, _ = h.device_ptr("qdp1")
    rc = h.remap_view(_Raw((h.nelemd, h.qsize, h.nlev, 4, 4), p), "eqkji", src, "ekji", tgt, "ekji", mode="mass", alg=0)
    return dict(rc=rc)


def op_DV(c):
    out = {}
    for name, x in zip(("interfaces", "surface"), c.inp["DV"]):
        x = x[c.mine]
        axes = "ekji" if x.ndim == 4 else "eji"
        a, b = c.device(x), c.device(x)
        c.hip.dss_view(a, axes, mode="average")
        c.hip.biharmonic_view(b, axes, order="biharmonic")
        out["dss_" + name], out["biharmonic_" + name] = a.cpu().numpy(), b.cpu().numpy()
    return out


def op_M(c):
    h = c.hip
    n, K = h.nelemd, h.nlev
    out = {}
    if c.limiter:
        out["qmin"], out["qmax"] = h.get_qminmax()
    out["mass"] = h.element_mass(c.last)
    out["qd_mass"], out["qd_var"], out["qd_min"], out["qd_max"] = h.element_qdiag(c.last)
    d = dict(divdp_proj=np.zeros((n, K, 4, 4)), eta_dot_dpdn=np.zeros((n, K, 4, 4)), omega_p=np.zeros((n, K, 4, 4)), divdp=np.zeros((n, K, 4, 4)),
             dp3d=np.zeros((n, K, 4, 4)), ps_v=np.zeros((n, 4, 4)))
    h.get_derived(d)
    out.update(("derived_" + k, v) for k, v in d.items())
    return out


def op_I(c):
    c.hip.invalidate_cache()


def op_X(c):
    c.hip.dcmip_set_initial()
    c.nstep, c.last = 0, 1


OPS = dict(S=op_S, S0=op_S0, P=op_P, P1=op_P1, R=op_R, C=op_C, C2=op_C2, CU=op_CU, H=op_H, Q=op_Q, F=op_F, FH=op_FH, VQ=op_VQ, VD=op_VD,
           VO=op_VO, G=op_G, RV=op_RV, DV=op_DV, M=op_M, I=op_I, X=op_X)
assert tuple(OPS) == KINDS
