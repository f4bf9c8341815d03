"""-m gpu: every call sequence of tests/call_sequences.py held to the bits of a fresh context.

The visible state after a call, and everything the call returns, depend only on the visible state before it, never on how the context got
there: call_sequences.replay runs a sequence on one warm context and repeats every op on a fresh context that was loaded with the warm one's
visible state (the tse_device_ptr fields, qmin / qmax, the host's nstep and time level; then tse_invalidate_cache and tse_dcmip_init).  Warm
and fresh must agree in every bit of the state and of what the op returned; the kinds that change no state must besides leave the warm
context's state alone.  This holds the context's hidden state (the cached bounds and their halo, the freshness of Q /
lnps, dcmip_static, the deferred final DSS, T's zero slots, the forked inputs, the twin level buffers, the qmin / qmin2 swaps, the staging
field's size) over every ordered pair of the 21 op kinds (test_call_sequences_cpu.py holds the generator to that).

Shape: ne2 (24 elements, the cube's corner elements among them), qsize 5 (a pad tracer in the bounds layout, the odd tail of the tracer
pairs), 72 levels, nu_q 1e19, DCMIP 1-1, tstep 1800, rsplit 3 (DCMIP 1-2: tstep 300, the step the case is run at: at 1800 its
vertical motion empties layers inside one remap cycle); TSE_PLACEMENT=0, so that a fresh context costs milliseconds.
 - one test per (sequence, limiter_option 8 | 9 | 0);
 - the hand-written list with DCMIP 1-2 (eta_dot_dpdn != 0);
 - three emulated ranks (test_gpu_multirank_emulated._run_ne), warm contexts only: after every op the visible state, gathered by global
   element, is the one-context warm run's, bit for bit -- with warm == fresh on one context this covers mm_halo and the prefetched bounds
   exchange.  No op kind is left out there: Q, FH, RV and DV need no set-up the rank's body cannot give (their inputs are rows of global
   arrays; DV is collective and every rank makes it).
 - tse_prim_run_subcycle on a context initialised with rsplit = 0 is refused with a message, and the context goes on working."""
import threading

import numpy as np
import pytest

import call_sequences as cs

pytestmark = pytest.mark.gpu
LIMITERS = (8, 9, 0)
RANK_SEQUENCES = tuple(cs.HAND) + ("random-00", "random-01")


@pytest.fixture(autouse=True)
def _no_placement_search(monkeypatch):
    monkeypatch.setenv("TSE_PLACEMENT", "0")
    for k in ("TSE_DSS_ON_READ", "TSE_REMAP_FUSED", "TSE_BOUNDARY_STRIPS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("limiter", LIMITERS)
@pytest.mark.parametrize("name", list(cs.sequences()))
def test_sequence_leaves_the_bits_of_a_fresh_context(name, limiter):
    cs.replay(lambda: cs.make_device_ctx(limiter), cs.sequences()[name], cs.OPS)


@pytest.mark.parametrize("name", list(cs.HAND))
def test_hand_written_sequences_with_dcmip_1_2(name):
    cs.replay(lambda: cs.make_device_ctx(8, case=2), cs.HAND[name], cs.OPS)


def _one_context_warm(name):
    c = cs.make_device_ctx(8)
    try:
        return cs.run_warm(c, cs.sequences()[name], cs.OPS)
    finally:
        c.close()


@pytest.mark.parametrize("name", RANK_SEQUENCES)
def test_three_ranks_leave_the_bits_of_one_context(name):
    import test_gpu_multirank_emulated as me
    world, seq = 3, cs.sequences()[name]
    one = _one_context_warm(name)
    meet = threading.Barrier(world)

    def body(r, h, mine, geo, hv):
        c = cs.DeviceCtx(h, mine, 1, 8)         # (_run_ne closes the context)
        try:
            return cs.run_warm(c, seq, cs.OPS, between=lambda k: meet.wait(timeout=120))
        except BaseException:
            meet.abort()
            raise
    res = me._run_ne(world, ne=cs.NE, qsize=cs.QSIZE, nu_q=cs.NU_Q, limiter_option=8, rsplit=cs.RSPLIT, body=body)
    nelem = 6 * cs.NE * cs.NE
    seen = np.zeros(nelem, dtype=int)
    for mine, _ in res:
        seen[mine] += 1
    assert (seen == 1).all()
    for k, kind in enumerate(seq):
        prev = seq[k - 1] if k else None
        want, want_ret = one[k]
        got = {n: np.zeros_like(x) for n, x in want["fields"].items()}
        got_ret = {}
        for mine, out in res:
            snap, ret = out[k]
            assert snap["scalars"] == want["scalars"], (k, kind, snap["scalars"], want["scalars"])
            for n, x in snap["fields"].items():
                got[n][mine] = x
            assert sorted(ret) == sorted(want_ret), (k, kind)
            for n, x in ret.items():
                x, w = cs.bits(x), cs.bits(want_ret[n])
                if x.ndim and x.shape[0] == len(mine) and w.shape[0] == nelem:
                    got_ret.setdefault(n, np.zeros_like(w))[mine] = x      # an array by local element
                else:
                    cs._compare("returned", {n: x}, {n: w}, k, kind, prev)    # a scalar: every rank returns the one context's
        cs._compare("state", got, want["fields"], k, kind, prev)
        cs._compare("returned", got_ret, {n: want_ret[n] for n in got_ret}, k, kind, prev)


def test_prim_run_subcycle_refuses_rsplit_0():
    """the reference's default rsplit = 0 used to reach `nstep % rsplit` on the host: now refused before anything is launched"""
    from transport_se_amd.hip_mod import TseError
    c = cs.DeviceCtx(cs.make_hip(8, rsplit=0), np.arange(6 * cs.NE * cs.NE), 1, 8)
    try:
        c.start()
        before = cs.snapshot(c)
        with pytest.raises(TseError, match="rsplit = 0") as ei:
            c.hip.prim_run_subcycle(c.tstep, 1, 0)
        assert ei.value.rc == 1 and ei.value.nstep == 0
        cs._compare("noop", cs.snapshot(c)["fields"], before["fields"], 0, "C", None)     # nothing was launched
        cs.op_S(c); cs.op_R(c)                                                            # the step-by-step entries do not need rsplit
        q = c.read("qdp2")
        assert np.isfinite(q).all() and q.max() > 0
    finally:
        c.close()
