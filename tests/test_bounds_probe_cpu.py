"""The dye fields of bounds_probe.py leave no neighbour of the limiter's bounds untested -- shown without a GPU.

* The census is full: on ne2, ne3, ne4 and ne5 (limiter 8; limiter 9 on ne2 and ne3, its model being Python) every (element, direction)
  that has a neighbour has at least MIN_WITNESSES witness slabs in stage 1 and in stage 3 of the first tracer step, every element has as
  many stage-2 witnesses, and stage 1 of the second step (the route that starts from cached bounds) and of the first step after a
  vertical_remap (the remap's emission) have them too.  Measured minima over all (e, d) and elements, limiter 8 / 9:
      ne2: stage 1 81 / 81, stage 2 25 / 20, stage 3 16 / 18, cached 20 / 21, after the remap 28 / 26
      ne3: stage 1 64 / 64, stage 2 21 / 15, stage 3 12 / 16, cached 12 / 13, after the remap 19 / 12
      ne4: stage 1 57,      stage 2 19,      stage 3 14,      cached 18,      after the remap 16
      ne5: stage 1 53,      stage 2 17,      stage 3 10,      cached 18,      after the remap 16
  (ne4 is here because the rank tests of test_gpu_bounds_probe.py cut ne4 into 2 and 3 ranks.)
* The witness predicate predicts a visible error: 22 runs of the model with one neighbour dropped from the bounds (all eight directions;
  an element at a cube vertex, one at a face seam, one interior of ne5; stages 1 and 3; the cached stage 1) each move the step's final
  Qdp by >= 1e6 x Q_TOL at a witness slab of the dropped pair (measured: 5.5e-3 to 0.14).
* Negative control: on the DCMIP 1-1 tracers at ne5 more than half of the (e, d) pairs have no witness at all -- the gap the dye fields
  close.

The states are advanced by the checker where a whole step is needed (the model with Probe8 is the checker bit for bit: asserted here
at every mesh; with Probe9 it is the model with Limiter9 bit for bit: asserted at ne2); the Python model runs the stages whose
pre-limiter values are recorded."""
import functools

import numpy as np
import pytest

import bounds_probe as bp
import pyoracle as po
import unlimited_model as um
from limiter9_model import Limiter9
from tracer_fields import q_err

Q_TOL = 1e-13                    # the project's per-step allowance (test_gpu_tracer_invariance.py)
VISIBLE = 1e6 * Q_TOL
STATE = ("qdp", "vn0", "dp", "divdp", "divdp_proj", "eta_dot_dpdn", "omega_p", "dp3d", "ps_v")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _oracle(ne, qsize=bp.QSIZE, tracer=None):
    """checker context at the start of the first tracer step on the dye fields (all tracers, or tracer `tracer` alone)"""
    nu, _ = bp.PARAMS[ne]
    o = po.Oracle(ne, qsize, nu_q=nu, rsplit=bp.RSPLIT, threads=8)
    o.dcmip_init(1)
    q = bp.dye(o) if tracer is None else bp.dye(o)[:, tracer:tracer + 1]
    o.qdp[0] = q; o.qdp[1] = q
    return o


@functools.lru_cache(maxsize=None)
def _probe(ne, limiter):
    """witness arrays of every route: dict(stage1, stage2, stage3, cached1, remap1) -> W, plus nbr_elem and face"""
    _, dt = bp.PARAMS[ne]
    o = _oracle(ne)
    try:
        lim = (bp.Probe9 if limiter == 9 else bp.Probe8)(o)
        W = {}
        o.dcmip_step_inputs(1, 0, dt)
        bp.model_step(o, dt, 0, lim, on_stage=lambda rhs, l: W.__setitem__("stage%d" % (rhs + 1), bp.witnesses(o, l.rec)))
        if limiter == 8:   # the model with the recording limiter is the checker
            c = _oracle(ne)
            c.dcmip_step_inputs(1, 0, dt); c.advec_tracers_remap_rk2(dt, 0)
            same = np.array_equal(_bits(c.qdp), _bits(o.qdp))
            c.close()
            assert same
        elif ne == 2:      # and with Probe9 it is the model test_gpu_bounds_probe.py holds the device to
            c = _oracle(ne)
            c.dcmip_step_inputs(1, 0, dt); um.advec_tracers_remap_rk2(c, dt, 0, Limiter9(c))
            same = np.array_equal(_bits(c.qdp), _bits(o.qdp))
            c.close()
            assert same
        keep = {k: getattr(o, k).copy() for k in STATE}
        # the first step after the remap that closes the cycle (RSPLIT = 1: the step above was the whole cycle)
        assert o.vertical_remap(dt * bp.RSPLIT, 2) == 0
        o.dcmip_step_inputs(1, 1, dt)
        bp.model_step(o, dt, 1, lim, stages=(0,), on_stage=lambda rhs, l: W.__setitem__("remap1", bp.witnesses(o, l.rec)))
        # the second step without a remap in between: on the device it starts from the bounds the first step's final DSS emitted
        for k in STATE:
            getattr(o, k)[...] = keep[k]
        o.dcmip_step_inputs(1, 1, dt)
        bp.model_step(o, dt, 1, lim, stages=(0,), on_stage=lambda rhs, l: W.__setitem__("cached1", bp.witnesses(o, l.rec)))
        W["nbr_elem"], W["face"] = np.array(o.nbr_elem), np.array(o.face)
        return W
    finally:
        o.close()


CENSUS = [(2, 8), (3, 8), (4, 8), (5, 8), (2, 9), (3, 9)]


@pytest.mark.parametrize("ne,limiter", CENSUS)
def test_census_is_full(ne, limiter):
    W = _probe(ne, limiter)
    has = W["nbr_elem"] >= 0
    assert has.sum() == 8 * 6 * ne * ne - 24          # (every element has eight neighbours but the 24 at the cube's vertices)
    for e in range(has.shape[0]):
        n = W["nbr_elem"][e][has[e]]
        assert len(set(n.tolist())) == n.size and e not in n, e       # (no neighbour twice: "alone" means one direction)
    mins = {}
    for route in ("stage1", "stage3", "cached1", "remap1"):
        c = bp.census(W["nbr_elem"], W[route])
        assert ((c == -1) == ~has).all()
        mins[route] = int(c[has].min())
        short = [(int(e), int(d), int(c[e, d])) for e, d in np.argwhere(has & (c < bp.MIN_WITNESSES))]
        assert not short, (route, short[:20])
    c = bp.census(W["nbr_elem"], W["stage2"])
    assert c.shape == (has.shape[0],)
    mins["stage2"] = int(c.min())
    assert c.min() >= bp.MIN_WITNESSES, np.argwhere(c < bp.MIN_WITNESSES).ravel().tolist()
    print("census ne%d limiter %d: smallest witness counts %s" % (ne, limiter, mins))


def _kinds(W):
    """one element at a cube vertex (a direction without neighbour), one at a face seam, one interior (the nine on one face; None at ne2)"""
    nbr, face = W["nbr_elem"], W["face"]
    vertex = seam = interior = None
    for e in range(nbr.shape[0]):
        if (nbr[e] < 0).any():
            vertex = e if vertex is None else vertex
        elif (face[nbr[e]] != face[e]).any():
            seam = e if seam is None else seam
        else:
            interior = e if interior is None else interior
    return vertex, seam, interior


def _plants():
    """(ne, element kind, direction, route): 22 runs (the first vertex element of ne3 has no neighbour in direction 4)"""
    runs = [(3, "seam", d, "stage1") for d in range(8)]
    runs += [(3, "vertex", d, "stage3") for d in range(8) if d != 4]
    runs += [(5, "interior", 1, "stage1"), (5, "interior", 6, "stage3"), (5, "interior", 4, "cached1")]
    runs += [(3, "seam", 2, "cached1"), (3, "seam", 7, "cached1"), (2, "vertex", 0, "cached1"), (2, "vertex", 5, "cached1")]
    return runs


CALL = dict(stage1=0, stage3=1, cached1=2)      # the index of the route's bounds() among those with a neighbour pass


@functools.lru_cache(maxsize=None)
def _reference(ne, tracer, nsteps):
    """the checker's Qdp of tracer `tracer` alone after nsteps tracer steps, and the dp of q_err"""
    _, dt = bp.PARAMS[ne]
    o = _oracle(ne, 1, tracer)
    try:
        for nstep in range(nsteps):
            o.dcmip_step_inputs(1, nstep, dt); o.advec_tracers_remap_rk2(dt, nstep)
        _, np1 = um.qdp_levels(nsteps - 1)
        return o.qdp[np1 - 1].copy(), (o.dp - dt * o.divdp_proj).copy()
    finally:
        o.close()


def test_plants_cover_what_they_should():
    runs = _plants()
    assert {d for _, _, d, _ in runs} == set(range(8))
    assert {k for _, k, _, _ in runs} == {"vertex", "seam", "interior"} and (5, "interior") in {(ne, k) for ne, k, _, _ in runs}
    assert {r for _, _, _, r in runs} == {"stage1", "stage3", "cached1"}
    assert len(runs) >= 16 and len(set(runs)) == len(runs)
    vertex = _kinds(_probe(3, 8))[0]
    assert np.flatnonzero(_probe(3, 8)["nbr_elem"][vertex] < 0).tolist() == [4]       # (the one direction _plants leaves out)


@pytest.mark.parametrize("ne,kind,d,route", _plants())
def test_a_dropped_neighbour_is_visible(ne, kind, d, route):
    """the model with neighbour d of element e left out of one bounds() differs from the checker by >= 1e6 x Q_TOL at a witness slab"""
    W = _probe(ne, 8)
    e = dict(zip(("vertex", "seam", "interior"), _kinds(W)))[kind]
    assert e is not None
    assert W["nbr_elem"][e, d] >= 0
    w = W[route][e, d]              # [q][k]
    tracer = int(np.argmax(w.sum(axis=1)))
    levels = np.flatnonzero(w[tracer])
    assert levels.size >= 1
    nsteps = 2 if route == "cached1" else 1
    ref, dp = _reference(ne, tracer, nsteps)
    _, dt = bp.PARAMS[ne]
    o = _oracle(ne, 1, tracer)
    try:
        lim = bp.Probe8(o, drop=(CALL[route], e, d))
        for nstep in range(nsteps):
            o.dcmip_step_inputs(1, nstep, dt)
            bp.model_step(o, dt, nstep, lim)
        _, np1 = um.qdp_levels(nsteps - 1)
        got = o.qdp[np1 - 1].copy()
    finally:
        o.close()
    err, _ = q_err(got, ref, dp)
    scale = np.abs(ref / dp[:, None]).max()
    at = np.abs((got[e, 0, levels] - ref[e, 0, levels]) / dp[e, levels]).max() / scale
    print("ne%d %s e=%d d=%d %s: q_err %.2e, at its witness slabs %.2e" % (ne, kind, e, d, route, err[0], at))
    assert err[0] >= VISIBLE and at >= VISIBLE, (err[0], at)


def test_unplanted_probe_on_one_tracer_is_the_checker():
    """the planted runs' set-up without a plant gives the reference's bits (so their difference is the plant's alone)"""
    ref, _ = _reference(2, 3, 2)
    _, dt = bp.PARAMS[2]
    o = _oracle(2, 1, 3)
    try:
        lim = bp.Probe8(o)
        for nstep in range(2):
            o.dcmip_step_inputs(1, nstep, dt)
            bp.model_step(o, dt, nstep, lim)
        assert np.array_equal(_bits(o.qdp[0]), _bits(ref))
    finally:
        o.close()


def test_dcmip_tracers_fail_the_census():
    """negative control: the DCMIP 1-1 tracers at ne5, the inputs of the rank and odd-mesh tests, leave more than half of the (e, d)
    pairs without a single witness in stage 1 and in stage 3"""
    nu, dt = bp.PARAMS[5]
    o = po.Oracle(5, 4, nu_q=nu, rsplit=bp.RSPLIT, threads=8)
    try:
        o.dcmip_init(1); o.dcmip_step_inputs(1, 0, dt)
        lim, W = bp.Probe8(o), {}
        bp.model_step(o, dt, 0, lim, on_stage=lambda rhs, l: W.__setitem__(rhs, bp.witnesses(o, l.rec)))
        has = np.asarray(o.nbr_elem) >= 0
        for rhs in (0, 2):
            none = (bp.census(o.nbr_elem, W[rhs]) == 0) & has
            print("DCMIP 1-1 at ne5, rhs_multiplier %d: %d of %d (e, d) pairs without a witness" % (rhs, none.sum(), has.sum()))
            assert none.sum() > has.sum() // 2, (rhs, int(none.sum()))
    finally:
        o.close()
