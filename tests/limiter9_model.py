"""Reference model of the clip-and-sum limiter (limiter_option = 9), for unlimited_model.euler_step(..., limiter=).

Per slab (the 16 points of one element, level and tracer), on the inputs of limiter_optim_iter_full (Qtens, spheremp, dp_star, minp, maxp):
  1. c = spheremp*dp_star, x = Qtens/dp_star, sumc = sum c, mass = sum c*x; sumc <= 0 leaves the slab alone;
  2. the bounds are relaxed as limiter 8 relaxes them: mass < minp*sumc -> minp = mass/sumc, mass > maxp*sumc -> maxp = mass/sumc;
  3. clip: xc = min(max(x, minp), maxp), addmass = sum (x - xc)*c;
  4. redistribute in proportion to the room left: v = maxp - xc if addmass > 0 else xc - minp, den = sum v*c,
     x = xc + (addmass/den)*v if den > 0 else xc;
  5. Qtens = x*dp_star (Qtens itself where step 3 clipped nothing).
The sums are serial over the 16 points, first index fastest, as the reference's limiters sum.  The bounds before the relaxation are
those of limiter 8 (the Limiter8 class of test_unlimited_cpu.py: element min/max, neighbour min/max, the stage-2 update); qmin is not
clamped at 0.  Everything else of the tracer step is unlimited_model's."""
import numpy as np

import unlimited_model as um
from test_unlimited_cpu import Limiter8


def limiter9(ptens, sphweights, minp, maxp, dpmass):
    """-> (ptens, minp, maxp, clipped, relaxed): one slab, arrays [j][i]"""
    c = (sphweights * dpmass).ravel()
    x = (ptens / dpmass).ravel()
    sumc, mass = 0.0, 0.0
    for i in range(16):
        sumc = sumc + c[i]
        mass = mass + c[i] * x[i]
    if sumc <= 0:
        return ptens, minp, maxp, False, False
    relaxed = False
    if mass < minp * sumc:
        minp = mass / sumc; relaxed = True
    if mass > maxp * sumc:
        maxp = mass / sumc; relaxed = True
    xc = np.minimum(np.maximum(x, minp), maxp)
    if np.array_equal(xc, x):
        return ptens, minp, maxp, False, relaxed
    addmass = 0.0
    for i in range(16):
        addmass = addmass + (x[i] - xc[i]) * c[i]
    v = maxp - xc if addmass > 0 else xc - minp
    den = 0.0
    for i in range(16):
        den = den + v[i] * c[i]
    xn = xc + (addmass / den) * v if den > 0 else xc
    return (xn * dpmass.ravel()).reshape(ptens.shape), minp, maxp, True, relaxed


class Limiter9(Limiter8):
    """limiter 8's bounds, limiter9 per slab.  Counts per euler_step (reset by bounds()): slabs, clipped, relaxed; `watch`, if set, is
    called with (x_out, minp, maxp) of every slab after the limiter (x_out = Qtens/dp_star, the relaxed bounds)."""

    def __init__(self, o, watch=None):
        super().__init__(o)
        self.slabs = self.clipped = self.relaxed = 0
        self.watch = watch

    def bounds(self, Q, rhs):
        super().bounds(Q, rhs)
        self.slabs = self.clipped = self.relaxed = 0

    def apply(self, e, q, k, qt, dp_star):
        out, mn, mx, clipped, relaxed = limiter9(qt, self.o.spheremp[e], self.mn[e, q, k], self.mx[e, q, k], dp_star)
        self.mn[e, q, k], self.mx[e, q, k] = mn, mx
        self.slabs += 1; self.clipped += bool(clipped); self.relaxed += bool(relaxed)
        if self.watch is not None:
            self.watch(out / dp_star, mn, mx)
        return out


def prim_run(o, test, tstep, nsub, limiter, nstep=0):
    """unlimited_model.prim_run with the limiter passed through every tracer step: rsplit steps, then the checker's vertical_remap.
    Returns (tracer steps done, next nstep)."""
    done = 0
    for _ in range(nsub):
        np1 = 2
        for _ in range(o.rsplit):
            o.dcmip_step_inputs(test, nstep, tstep)
            um.advec_tracers_remap_rk2(o, tstep, nstep, limiter)
            _, np1 = um.qdp_levels(nstep)
            nstep += 1
            done += 1
        if o.vertical_remap(tstep * o.rsplit, np1):
            raise RuntimeError("negative layer thickness")
    return done, nstep
