"""Inputs for which a wrong neighbour in the limiter's bounds cannot pass: dye fields, witnesses and their census (plain numpy; no HIP import).

The limiters clip a slab (the 16 points of one element, level and tracer) to the extremes of Q = Qdp/dp over the element and its up to
eight neighbours.  A missing or swapped neighbour changes a result only where that neighbour alone held the extreme AND the limiter
clipped against it.  This module builds fields where both happen, for every (element, direction), many times:

dye(o, qsize, seed)
    Qdp[e][q][k][j][i] = Q * dp with Q = BASE + OFF * u_elem + AMP * b_point: u_elem uniform(0, 1) drawn independently per (element,
    tracer, level), b_point 0 or 1 drawn independently per point.  Positive, O(1), discontinuous between elements on purpose; the
    offset orders the elements strictly, so over 72 levels x qsize slabs each of the nine members of an element's neighbourhood
    alone holds the minimum, and the maximum, many times.  The point noise has two levels, not a continuum: a stage-2 witness needs
    the values on both sides of an element edge near their elements' extremes at once, and with uniform point noise the elements next
    to the poles (where the DCMIP 1-1 winds vanish) were left with none; with two levels a quarter of all edge points qualify.

Probe8 / Probe9
    tests' Limiter8 / Limiter9 (bit for bit the checker's bounds; test_unlimited_cpu.py) that record, per euler_step, the pre-limiter
    x = Qtens/dp_star extremes of every slab, the element extremes of Q and the bounds used.  drop=(call, e, d) plants a defect: the
    `call`-th bounds() with a neighbour pass (stages 1 and 3 of every step, counted from 0) skips neighbour d of element e.

witnesses(o, rec)
    slab (e, q, k) is a witness for (e, d) of a stage with a neighbour pass (rhs_multiplier 0 and 2) when, with G = GAP * max|Q| of the
    tracer at that stage, on the minimum side
      * neighbour d's element minimum lies >= G below the minimum of the other members of {e} u nbr_elem[e], and
      * the slab's smallest pre-limiter value lies >= G below that runner-up minimum
    (with d left out the limiter would clip at least G more), or the mirrored pair holds on the maximum side.  For rhs_multiplier 1
    there is no neighbour pass: the slab is a witness for e when the element's own new extreme lies >= G beyond the inherited bound
    and the slab's pre-limiter values go beyond that new extreme (the limiter clips against it).
    G = 1e-3 is a condition (1e10 x the project's Q_TOL of 1e-13), not a measurement.

census(nbr_elem, W) -> witness count per (e, d) ([nelem][8]; -1 where there is no neighbour) or per e (rhs_multiplier 1).

The neighbour sets are the checker's o.nbr_elem (validated against the reference, independent of cube_mesh).
"""
import numpy as np

import unlimited_model as um
from limiter9_model import Limiter9
from test_unlimited_cpu import Limiter8
from tracer_fields import layer_dp

NLEV = 72
GAP = 1e-3            # witness gap G, relative to the tracer's max|Q|
# ---- the dye constants (chosen on the CPU until the census of test_bounds_probe_cpu.py is full; that test asserts it) ----
BASE, OFF, AMP = 0.5, 0.25, 1.0
QSIZE = 6
SEED = 20261019
MIN_WITNESSES = 3
PARAMS = {2: (2.4e18, 19200.0), 3: (6.5e17, 19200.0), 4: (2.6e17, 14400.0), 5: (1.3e17, 11520.0)}   # ne -> (nu_q, tracer time step) on the DCMIP 1-1 winds
RSPLIT = 1             # tracer steps per vertical remap in the probes' prim_run_subcycle cycles


def dye(o, qsize=QSIZE, seed=SEED, nlev=NLEV):
    """Qdp[e][q][k][j][i] of the dye family on oracle o's grid at its current ps_v (call after o.dcmip_init)"""
    return dye_q(o.nelem, qsize, seed, nlev) * layer_dp(o.hyai, o.hybi, o.ps_v)[:, None]


def dye_q(nelem, qsize=QSIZE, seed=SEED, nlev=NLEV):
    """the mixing ratios Q[e][q][k][j][i] alone (element order = the checker's / cube_mesh's global order)"""
    rng = np.random.default_rng(seed)
    off = rng.uniform(size=(nelem, qsize, nlev, 1, 1))
    noise = rng.integers(0, 2, size=(nelem, qsize, nlev, 4, 4)).astype(np.float64)
    return BASE + OFF * off + AMP * noise


def elem_extremes(Q):
    """element min / max of Q[..., j, i] in the checker's comparison order"""
    mn, mx = Q[..., 0, 0].copy(), Q[..., 0, 0].copy()
    for p in range(1, 16):
        x = Q[..., p // 4, p % 4]
        mn = np.where(x < mn, x, mn); mx = np.where(x > mx, x, mx)
    return mn, mx


def nbr_extremes(nbr_elem, m0, x0, skip=None):
    """min / max over {e} u nbr_elem[e] of the element extremes m0, x0 [e][...], in the checker's order; skip = (e, d) leaves one out"""
    mn, mx = m0.copy(), x0.copy()
    for e in range(nbr_elem.shape[0]):
        for d in range(8):
            n = nbr_elem[e, d]
            if n < 0 or skip == (e, d):
                continue
            mn[e] = np.where(m0[n] < mn[e], m0[n], mn[e])
            mx[e] = np.where(x0[n] > mx[e], x0[n], mx[e])
    return mn, mx


class _Probe:
    """mixin in front of Limiter8 / Limiter9: the same bounds, recorded; see the module text"""

    def __init__(self, o, drop=None):
        super().__init__(o)
        self.drop, self.calls, self.rec = drop, 0, None

    def bounds(self, Q, rhs):
        m0, x0 = elem_extremes(Q)
        scale = np.abs(Q).max(axis=(0, 2, 3, 4))
        inh = (self.mn.copy(), self.mx.copy()) if rhs == 1 else None
        super().bounds(Q, rhs)                    # Limiter8's / Limiter9's own bounds
        if rhs != 1:
            mn, mx = nbr_extremes(self.o.nbr_elem, m0, x0)
            assert np.array_equal(mn, self.mn) and np.array_equal(mx, self.mx)       # (what a plant leaves a neighbour out of)
            if self.drop is not None and self.drop[0] == self.calls:
                self.mn, self.mx = nbr_extremes(self.o.nbr_elem, m0, x0, tuple(self.drop[1:]))
            self.calls += 1
        self.rec = dict(rhs=rhs, m0=m0, x0=x0, mn=self.mn.copy(), mx=self.mx.copy(), inh=inh, scale=scale,
                        xlo=np.full(m0.shape, np.nan), xhi=np.full(m0.shape, np.nan))

    def apply(self, e, q, k, qt, dp_star):
        x = qt / dp_star
        self.rec["xlo"][e, q, k] = x.min(); self.rec["xhi"][e, q, k] = x.max()
        return super().apply(e, q, k, qt, dp_star)


class Probe8(_Probe, Limiter8):
    pass


class Probe9(_Probe, Limiter9):
    pass


def witnesses(o, rec, gap=GAP):
    """rec of a Probe after one euler_step -> bool W[e][d][q][k] (rhs_multiplier 0, 2) or W[e][q][k] (rhs_multiplier 1)"""
    G = (gap * rec["scale"])[None, :, None]
    xlo, xhi = rec["xlo"], rec["xhi"]
    assert np.isfinite(xlo).all() and np.isfinite(xhi).all()
    if rec["rhs"] == 1:
        imn, imx = rec["inh"]
        lo = (rec["m0"] <= imn - G) & (xlo < rec["m0"])
        hi = (rec["x0"] >= imx + G) & (xhi > rec["x0"])
        return lo | hi
    m0, x0 = rec["m0"], rec["x0"]
    n = o.nelem
    W = np.zeros((n, 8) + m0.shape[1:], dtype=bool)
    for e in range(n):
        mem = [e] + [int(o.nbr_elem[e, d]) for d in range(8) if o.nbr_elem[e, d] >= 0]
        dirs = [d for d in range(8) if o.nbr_elem[e, d] >= 0]
        M, X = m0[mem], x0[mem]
        for j, d in enumerate(dirs, start=1):
            rest = [i for i in range(len(mem)) if i != j]
            rmn, rmx = M[rest].min(axis=0), X[rest].max(axis=0)    # the runner-up bounds: what is left without neighbour d
            lo = (M[j] <= rmn - G[0]) & (xlo[e] <= rmn - G[0])
            hi = (X[j] >= rmx + G[0]) & (xhi[e] >= rmx + G[0])
            W[e, d] = lo | hi
    return W


def census(nbr_elem, W):
    """witness count per (e, d), -1 where nbr_elem has no neighbour -- or per e for a stage-2 W"""
    if W.ndim == 3:
        return W.sum(axis=(1, 2)).astype(np.int64)
    c = W.sum(axis=(2, 3)).astype(np.int64)
    assert not c[np.asarray(nbr_elem) < 0].any()          # (a witness needs a neighbour)
    c[np.asarray(nbr_elem) < 0] = -1
    return c


def form_divdp(o):
    for e in range(o.nelem):
        for k in range(NLEV):
            d = o.divergence_sphere(e, o.vn0[e, k])
            o.divdp[e, k] = d; o.divdp_proj[e, k] = d


def model_step(o, dt, nstep, lim, stages=(0, 1, 2), on_stage=None):
    """unlimited_model.advec_tracers_remap_rk2 with limiter lim, stage by stage (o.dcmip_step_inputs called by the caller);
    on_stage(rhs, lim) after each stage; stages: which rhs_multipliers to run (a prefix: the step is left unfinished otherwise)"""
    n0, np1 = um.qdp_levels(nstep)
    form_divdp(o)
    for rhs, (a, b, dss) in enumerate(((np1, n0, 3), (np1, np1, 1), (np1, np1, 2))):
        if rhs not in stages:
            return
        um.euler_step(o, a, b, dt / 2, dss, rhs, lim)
        if on_stage is not None:
            on_stage(rhs, lim)
    o.qdp[np1 - 1] = (o.qdp[n0 - 1] + 2.0 * o.qdp[np1 - 1]) / 3.0
