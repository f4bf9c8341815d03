"""The slab limiters (csrc/tse_device.h: limiter8_quad, limiter9_quad) as functions of 34 numbers: input families, the references, a
float64 restatement of the device's order, the device entry of the -DTSE_AB_HOOKS library, and the predicates the tests assert.

A slab is x[4][4] (rows j = lanes of a quad, i in-lane), weights c[4][4] = spheremp*dp_star, and the bounds minp, maxp.  Every predicate
is evaluated in numpy longdouble from the inputs and ONE implementation's output, and holds whichever way a near-tie of that
implementation falls (any summation order, with or without FMA contraction).  u = 2^-53, gamma_m = m*u; S = sum c*|x_in|,
mass = sum c*x_in, sumc = sum c, tol = (double)5e-14f.  Within a slab the weights have one sign (sumc <= 0: all <= 0).

 (a) No-op.  sumc <= 0, or every point inside [minp, maxp] and both relaxation tests decided false: x, minp, maxp come back bit for bit
     and `changed` is false.  (No -0.0 among the inputs: limiter 9's fma(0, v, -0.0) is +0.0.)
 (b) Relaxation.  The device tests fl(mass) < fl(minp*fl(sumc)).  fl(mass) is a 16-term sum of products (m = 16, magnitude S), the right
     side two roundings and a 15-term sum (m = 17, magnitude |minp|*sumc); with one more for the longdouble evaluation the test is DECIDED
     when |mass - minp*sumc| > gamma_17*S + gamma_18*|minp|*sumc.  Decided false: the bound comes back bit for bit.  Decided true: the
     bound is mass/sumc (limiter 9: mass*(1/sumc)) to RELAX_ULPS*u*S/sumc -- 16 roundings of the mass, 15 of sumc, the division or the
     reciprocal and product, relative to S/sumc >= |mass/sumc|: 34, asserted as 40.  The allowance is relative to S/sumc, not to the
     bound: on a slab whose mass cancels (the +-50 spikes: S far above |mass|) the roundings of the sum are that large against mass/sumc,
     and "a few ulps of the bound" holds only where S = |mass|.  Undecided: either outcome.
 (c) Bounds.  Limiter 8: a slab that converged ends on a clip, so minp' <= x <= maxp' exactly (the reference must need <= 14 of the 15
     iterations on every slab of the families; an implementation may stop one later).  Limiter 9 ends on x = fma(inc, v, xc), v = maxp' - xc
     (up) or xc - minp' (down), inc = addmass/den.  Feasibility after the relaxation gives addmass <= den up to rounding:
       addmass* = mass - sum c*xc <= maxp'*sumc + F - sum c*xc = den* + F,   F = u*(17*S + 18*B), B = max(|minp'|,|maxp'|)*sumc
     and fl(addmass) adds 17*u*V, V = sum c*|x - xc| (difference, product, 15 additions), fl(den) 17*u*den*, the division and v one each:
       inc*v_i <= v_i*(1 + eta),  eta = u*(20 + (17*V + 17*S + 18*B)/den*)
     so a point overshoots its bound by at most 2*u*max(|minp'|,|maxp'|) (the final rounding, doubled) + v_i*eta.  A wrong sign of an
     addmass within its own error moves the points by no more than the same terms, so both sides get the allowance of their direction.
 (d) Mass.  |sum c*x_out - mass| <= tol*|mass| + K*u*S.  After the relaxation minp' <= mass/sumc <= maxp' (to rounding), so a clipped
     point satisfies |xc_i| <= max(|x_i|, |mass/sumc|): sum c*|xc| <= 2S, V <= 2S, |addmass| <= 2S, and after a redistribution
     sum c*|x| <= sum c*|xc| + |addmass| <= 4S; later iterations only shrink V and addmass.  One iteration of limiter 8 changes the exact
     mass by (fl(addmass) - addmass*) + addmass*(error of w and of the division) + the rounding of x + inc:
       17*u*V + 17*u*|addmass| + u*sum c*|x_new| <= (34 + 34 + 4)*u*S = 72*u*S
     (a contraction only removes roundings).  The converged iteration discards |addmass*| <= tol*|fl(mass)| + 17*u*V.  A slab whose points
     are all pinned discards addmass*, which feasibility bounds by F + 17*u*S <= 52*u*S.  With T iterations in the reference and at most
     T + 1 in any other evaluation (a second flipped convergence test would need addmass to stay within rounding of tol*|mass| over two
     iterations, each of which shrinks it by orders of magnitude): K8(T) = 72*(T + 1) + 34 + 52 + 2 (tol*|fl(mass)|, longdouble) -> 72*(T+1) + 96.
     Limiter 9 has one clip and one redistribution, no tolerance: (fl(addmass) - addmass*) 34*u*S, addmass*(17 den + division + v) 38*u*S,
     the final fma 4*u*S, all pinned (den <= 0) 52*u*S, longdouble 1: K9 = 129 -> 136.
 (e) Against the reference (pyoracle.limiter8, limiter9_model.limiter9), weighted: sum c*|x - x_ref| <= 2*tol*|mass| + K'*u*S.  Both
     evaluations end on clip(xc + lambda) of the same clipped slab, lambda fixed by the mass each conserves: they differ by the two
     discarded addmasses (2*tol*|mass|), by both (d) errors, by the pointwise roundings of x + inc (u*4S per iteration and evaluation)
     and by a bound relaxed by one and not the other (undecided (b): the bounds then differ by <= 35*u*S/sumc, 35*u*S in the weighted
     norm, doubled for the redistribution it causes): K8'(T) = 2*K8(T) + 8*(T + 1) + 70, K9' = 2*K9 + 8 + 70 = 350.
 (f) Scaling x and the bounds by 2^+-200 scales the output by exactly that.
"""
import ctypes as C

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TOL_LIMITER = float(np.float32(5e-14))   # (double)5e-14f
N_PER_FAMILY = 256
SEED = 20240817
RELAX_ULPS = 40
K9, K9E = 136, 350
GLLW = np.array([1.0 / 6, 5.0 / 6, 5.0 / 6, 1.0 / 6])
FAMILIES = ("inside", "clip", "checker", "relax", "spike", "flat", "pinned", "noweight", "negmass")
SLOW = ("relax", "spike")          # iterate most
IDLE = ("inside", "noweight")      # no-op slabs and sumc <= 0 slabs
# families whose last CANCEL_SLABS slabs are the cancelling slabs of families() (2 of 256: under the 1 % cap on undecided slabs).  A slab
# takes the all-pinned path in 65 % of independent evaluations (another summation order, a contraction), so 10 slabs leave an evaluation
# that never meets its `w <= 0` guard a chance of 3e-5
CANCEL, CANCEL_SLABS = ("clip", "checker", "flat", "pinned", "negmass"), 2


def k8(iters):
    return 72 * (np.minimum(iters, 15) + 1) + 96


def k8e(iters):
    return 2 * k8(iters) + 8 * (np.minimum(iters, 15) + 1) + 70


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _weights(rng, n, spheremp):
    """c = spheremp*dp: even slabs a real element of the ne2 grid, odd slabs a GLL weight outer product (same total area); dp from 5 to
    4000 (log-uniform) with 3 % point-to-point variation"""
    dp = np.exp(rng.uniform(np.log(5.0), np.log(4000.0), n))[:, None, None] * (1.0 + 0.03 * rng.uniform(-1, 1, (n, 4, 4)))
    sm = np.empty((n, 4, 4))
    sm[0::2] = spheremp[rng.integers(0, spheremp.shape[0], sm[0::2].shape[0])]
    sm[1::2] = np.outer(GLLW, GLLW) * (spheremp[0].sum() / 4.0)
    return sm * dp


def _mirror(x, mn, mx, which):
    w3 = which[:, None, None]
    return np.where(w3, -x, x), np.where(which, -mx, mn), np.where(which, -mn, mx)


def families(spheremp, n=N_PER_FAMILY, seed=SEED):
    """{family: (x[n][4][4], c[n][4][4], minp[n], maxp[n])}; both signs of x (a slab and its bounds mirrored) in every family"""
    out = {}
    for fi, name in enumerate(FAMILIES):
        rng = np.random.default_rng(seed + fi)
        c = _weights(rng, n, spheremp)
        one = np.ones(n)
        pick = rng.integers(0, 3, n)
        if name == "inside":
            x, mn, mx = rng.uniform(0.2, 0.9, (n, 4, 4)), 0.1 * one, 1.0 * one
        elif name in ("clip", "negmass"):   # clipped above, below, on both sides
            x = rng.uniform(0.0, 1.0, (n, 4, 4))
            mn, mx = np.choose(pick, [-1.0, 0.3, 0.2]) * one, np.choose(pick, [0.7, 2.0, 0.8]) * one
        elif name == "checker":
            x = ((np.arange(4)[:, None] + np.arange(4)[None, :]) % 2)[None] + rng.uniform(-0.3, 0.3, (n, 4, 4))
            mn, mx = 0.0 * one, 1.0 * one
        elif name == "relax":   # mean above maxp (even) / below minp (odd)
            x = rng.uniform(0.0, 1.0, (n, 4, 4))
            ev = np.arange(n) % 2 == 0
            mn, mx = np.where(ev, -0.5, 0.7), np.where(ev, 0.3, 1.5)
        elif name == "spike":   # one spike of 50 (bounds [-0.01, 10]) or +50 and -50 (bounds [-1, 1]) on a field of +-1e-3
            x = rng.uniform(-1e-3, 1e-3, (n, 4, 4))
            p = rng.integers(0, 16, n); p2 = (p + 1 + rng.integers(0, 15, n)) % 16
            two = np.arange(n) % 2 == 1
            x.reshape(n, 16)[np.arange(n), p] = 50.0
            x.reshape(n, 16)[np.arange(n)[two], p2[two]] = -50.0
            mn, mx = np.where(two, -1.0, -0.01), np.where(two, 1.0, 10.0)
        elif name == "flat":   # uniform to 1e-13, minp == maxp 1e-13 to one side (the relaxation test stays decided)
            x0 = rng.uniform(0.5, 2.0, n)
            x = x0[:, None, None] * (1.0 + 1e-13 * rng.uniform(-1, 1, (n, 4, 4)))
            mn = x0 * (1.0 + 1e-13 * np.where(rng.random(n) < 0.5, -1.0, 1.0)); mx = mn.copy()
        elif name == "pinned":   # exactly uniform beyond a bound: the bound relaxes to the mean and pins every point (w == 0, den == 0)
            x0 = rng.uniform(0.5, 2.0, n)
            x = np.repeat(x0, 16).reshape(n, 4, 4)
            t = rng.uniform(0.01, 0.5, n); up = np.arange(n) % 2 == 0
            mn, mx = np.where(up, x0 * (1 - t) - 1.0, x0 * (1 + t)), np.where(up, x0 * (1 - t), x0 * (1 + t) + 1.0)
        elif name == "noweight":   # c all zero (even) / all negative (odd); the values would be clipped
            x = rng.uniform(0.0, 1.0, (n, 4, 4)); mn, mx = 0.2 * one, 0.8 * one
            c = np.where((np.arange(n) % 2 == 0)[:, None, None], 0.0, -c)
        if name in CANCEL:
            # the last CANCEL_SLABS slabs: minp == maxp == 0 and mixed signs whose mass cancels to rounding, so that tol*|mass| is far below
            # the rounding noise of addmass.  One bound relaxes to mass/sumc (a relaxation test within its own error: undecided in (b), under
            # the 1 % cap), the first redistribution moves the points at the other bound by that noise, the second clip pins every point
            # with addmass != 0 and done false: limiter 8's `w <= 0` guard decides inc.  Limiter 9 gets inc = addmass/den far above 1 there.
            # (Whether the noise takes that path depends on its last bits: of 16 candidates the first CANCEL_SLABS that do, by the
            # restatement's count, are kept.)
            k, m = CANCEL_SLABS, 16
            xs = rng.uniform(0.5, 1.0, (m, 16)) * np.where(np.arange(16) % 2 == 0, 1.0, -1.0)[rng.permuted(np.tile(np.arange(16), (m, 1)), axis=1)]
            cs = np.tile(c[-k:].reshape(k, 16), (m // k, 1))
            xs[:, 0] = -(cs[:, 1:] * xs[:, 1:]).sum(1) / cs[:, 0]
            st = {}
            restate8(xs.reshape(m, 4, 4), cs.reshape(m, 4, 4), np.zeros(m), np.zeros(m), stats=st)
            keep = np.nonzero(st["w_guard"])[0][:k]
            assert keep.size == k, name
            x[-k:] = xs[keep].reshape(k, 4, 4); c[-k:] = cs[keep].reshape(k, 4, 4); mn[-k:] = 0.0; mx[-k:] = 0.0
        which = np.ones(n, bool) if name == "negmass" else rng.random(n) < 0.5
        x, mn, mx = _mirror(x, mn, mx, which)
        x = x + 0.0   # (no -0.0)
        out[name] = (np.ascontiguousarray(x), np.ascontiguousarray(c), np.ascontiguousarray(mn + 0.0), np.ascontiguousarray(mx + 0.0))
    return out


def scaled(inp, e):
    x, c, mn, mx = inp
    return np.ldexp(x, e), c, np.ldexp(mn, e), np.ldexp(mx, e)


def concat(inputs):
    return tuple(np.concatenate([i[k] for i in inputs]) for k in range(4))


def take(inp, idx):
    return tuple(np.ascontiguousarray(a[idx]) for a in inp)


def ne2_spheremp():
    import pyoracle as po
    o = po.Oracle(2, 1)
    try:
        return o.spheremp.copy()
    finally:
        o.close()


# ---- implementations: (x, c, minp, maxp) -> (x, minp, maxp, changed, iterations or None) ---------------------------------------------
def oracle8(x, c, mn, mx):
    """pyoracle.limiter8 per slab (dpmass = 1: x and c pass through exactly)"""
    import pyoracle as po
    n = x.shape[0]
    xo, mno, mxo, it = np.empty_like(x), np.empty(n), np.empty(n), np.zeros(n, int)
    ones = np.ones((4, 4))
    for s in range(n):
        xo[s], mno[s], mxo[s], it[s] = po.limiter8(x[s], c[s], mn[s], mx[s], ones)
    return xo, mno, mxo, ~(_same(mno, mn) & _same(mxo, mx)), it


def model9(x, c, mn, mx):
    """limiter9_model.limiter9 per slab (dpmass = 1)"""
    from limiter9_model import limiter9
    n = x.shape[0]
    xo, mno, mxo, ch = np.empty_like(x), np.empty(n), np.empty(n), np.zeros(n, bool)
    ones = np.ones((4, 4))
    for s in range(n):
        xo[s], mno[s], mxo[s], _, ch[s] = limiter9(x[s].copy(), c[s], mn[s], mx[s], ones)
    return xo, mno, mxo, ch, None


def _lane(t):
    """the in-lane serial sum over i of t[n][j][i]"""
    return ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]


def _quad(a):
    """quad_sum of a[n][j]: the (j0+j1)+(j2+j3) butterfly"""
    return (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])


def _clip(x, mn, mx):
    return np.minimum(np.maximum(x, mn[:, None, None]), mx[:, None, None])


def restate8(x, c, mn, mx, guard=True, stats=None):
    """limiter8_quad in float64 numpy, in the device's order without contraction; every slab leaves the loop on its own convergence.
    The pinned-point selection is the device's 0.0/1.0 factor (x + m*inc), so an infinite increment reaches a pinned point as NaN.
    guard=False: without the device's `w <= 0` guard.  stats: a dict that receives "w_guard", the slabs in which a not yet converged
    iteration found every point pinned (w <= 0 with done false: the guard decides inc)"""
    x, mn, mx = x.copy(), mn.copy(), mx.copy()
    with np.errstate(all="ignore"):
        sumc = _quad(_lane(c)); live = sumc > 0
        mass = _quad(_lane(c * x))
        lo, hi = live & (mass < mn * sumc), live & (mass > mx * sumc)
        r = mass / sumc
        mn, mx = np.where(lo, r, mn), np.where(hi, r, mx)
        tolm = TOL_LIMITER * np.abs(mass)
        active, it = live.copy(), np.zeros(x.shape[0], int)
        hit = np.zeros(x.shape[0], bool)
        for iteration in range(1, 16):
            if not active.any():
                break
            a3 = active[:, None, None]
            xc = _clip(x, mn, mx)
            add = _quad(_lane((x - xc) * c))
            x = np.where(a3, xc, x)
            it[active] = iteration
            active = active & ~(np.abs(add) <= tolm)
            a3 = active[:, None, None]
            m = x != np.where(add > 0, mx, mn)[:, None, None]
            w = _quad(_lane(np.where(m, c, 0.0)))
            hit |= active & ~(w > 0)
            inc = np.where(active & ((w > 0) | (not guard)), add / w, 0.0)
            x = np.where(a3, x + np.where(m, 1.0, 0.0) * inc[:, None, None], x)
    if stats is not None:
        stats["w_guard"] = hit
    return x, mn, mx, lo | hi, it


def restate9(x, c, mn, mx, guard=True, stats=None):
    """limiter9_quad in float64 numpy, in the device's order.  guard=False: without the device's `den > 0` guard.  stats: a dict that
    receives "den_guard", the slabs with den <= 0 (every point at the bound the mass moves towards, or nothing clipped on a flat slab)"""
    with np.errstate(all="ignore"):
        sumc = _quad(_lane(c)); live = sumc > 0
        mass = _quad(_lane(c * x))
        lo, hi = live & (mass < mn * sumc), live & (mass > mx * sumc)
        r = mass * (1.0 / sumc)
        mn, mx = np.where(lo, r, mn), np.where(hi, r, mx)
        xc = _clip(x, mn, mx)
        add = _quad(_lane((x - xc) * c))
        up = (add > 0)[:, None, None]
        v = np.where(up, mx[:, None, None] - xc, xc - mn[:, None, None])
        den = _quad(_lane(v * c))
        inc = np.where((den > 0) | (not guard), add / den, 0.0)
        xo = np.where(live[:, None, None], xc + inc[:, None, None] * v, x)
    if stats is not None:
        stats["den_guard"] = live & ~(den > 0)
    return xo, mn, mx, lo | hi, None


_dev = None


def device(option, x, c, mn, mx):
    """tse_test_limiter of the -DTSE_AB_HOOKS library (not in the product library): the limiters' own source on the GPU, slab s in wave
    s // 16"""
    global _dev
    if _dev is None:
        from transport_se_amd import _lib
        _dev = _lib.lib(_lib.HOOKS_SO)
        _dev.tse_test_limiter.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5
    n = x.shape[0]
    xo, co = np.array(x, dtype=np.float64, order="C"), np.ascontiguousarray(c, dtype=np.float64)
    mno, mxo, ch = np.array(mn, dtype=np.float64), np.array(mx, dtype=np.float64), np.zeros(n, np.int32)
    assert xo.shape == co.shape == (n, 4, 4) and mno.shape == mxo.shape == (n,)
    if _dev.tse_test_limiter(int(option), n, xo.ctypes.data, co.ctypes.data, mno.ctypes.data, mxo.ctypes.data, ch.ctypes.data):
        raise RuntimeError(_dev.tse_last_error().decode())
    return xo, mno, mxo, ch != 0, None


# ---- predicates ----------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """bit equality per slab"""
    e = _bits(a) == _bits(b)
    return e.reshape(e.shape[0], -1).all(axis=1)


def _div(a, b):
    return np.where(b > 0, a / np.where(b > 0, b, 1), 0)


class Report:
    """what the predicates found for one implementation on one batch: `bad` lists (predicate, slab indices); undecided: the slabs (b)
    skipped; ratio_c (limiter 9 overshoot / allowance), ratio_d, ratio_e: per slab, measured / bound"""

    def __init__(self):
        self.bad = []

    def fail(self, what, mask):
        if np.any(mask):
            self.bad.append((what, np.nonzero(mask)[0][:6].tolist(), int(np.count_nonzero(mask))))

    def failed(self, what):
        return any(b[0].startswith(what) for b in self.bad)


def evaluate(option, inp, out, ref=None, iters=None):
    """every predicate on `out` = (x, minp, maxp, changed, _) of one implementation for the inputs `inp`; ref: the reference's output for
    (e); iters: the reference's iteration count per slab (limiter 8: K8(T), and (c) demands T <= 14)"""
    x, c, mn, mx = inp
    xo, mno, mxo, ch = out[:4]
    n = x.shape[0]
    R = Report()
    xl, cl, mnl, mxl, xol = x.astype(LD), c.astype(LD), mn.astype(LD), mx.astype(LD), xo.astype(LD)
    assert np.all((c >= 0).reshape(n, -1).all(1) | (c <= 0).reshape(n, -1).all(1)), "weights of one sign per slab"
    sumc, mass, S = cl.sum((1, 2)), (cl * xl).sum((1, 2)), (cl * np.abs(xl)).sum((1, 2))
    live = sumc > 0
    R.fail("finite", ~(np.isfinite(xo).reshape(n, -1).all(1) & np.isfinite(mno) & np.isfinite(mxo)))
    # (b)
    g17, g18 = 17 * LD(U), 18 * LD(U)
    dec = {}
    for side, b, bo, sgn in (("minp", mnl, mno, 1), ("maxp", mxl, mxo, -1)):
        E = g17 * S + g18 * np.abs(b) * sumc
        d = (mass - b * sumc) * sgn     # relax when d < 0
        true, false = live & (d < -E), live & (d > E)
        dec[side] = (true, false)
        R.fail("(b) %s relaxed on a decided-false test" % side, false & ~_same(bo, b.astype(np.float64)))
        R.fail("(b) %s is not mass/sumc" % side, true & ~(np.abs(bo.astype(LD) - _div(mass, sumc)) <= RELAX_ULPS * LD(U) * _div(S, sumc)))
    decided = ~live | ((dec["minp"][0] | dec["minp"][1]) & (dec["maxp"][0] | dec["maxp"][1]))
    R.undecided = ~decided
    differs = ~(_same(mno, mn) & _same(mxo, mx))
    R.fail("changed is false for a bound that came back different", differs & ~ch)
    R.fail("changed is true for bounds that came back the same", decided & ch & ~differs)
    # (a)
    inside = ((x >= mn[:, None, None]) & (x <= mx[:, None, None])).reshape(n, -1).all(1)
    noop = ~live | (live & dec["minp"][1] & dec["maxp"][1] & inside)
    R.noop = noop
    R.fail("(a) a no-op slab changed", noop & ~(_same(xo, x) & ~differs & ~ch))
    # (c)
    lo3, hi3 = mno.astype(LD)[:, None, None], mxo.astype(LD)[:, None, None]
    R.ratio_c = np.zeros(n)
    if option == 8:
        T = np.zeros(n, int) if iters is None else np.asarray(iters)
        R.fail("(c) the reference needs more than 14 iterations", live & (T > 14))
        R.fail("(c) a point outside its bounds", live & ~((xol >= lo3) & (xol <= hi3)).reshape(n, -1).all(1))
        K, KE, tol = k8(T), k8e(T), LD(TOL_LIMITER)
    else:
        xc = np.minimum(np.maximum(xl, lo3), hi3)
        V = (cl * np.abs(xl - xc)).sum((1, 2))
        B = np.maximum(np.abs(lo3), np.abs(hi3))[:, 0, 0] * sumc
        ulp2 = 2 * LD(U) * np.maximum(np.abs(lo3), np.abs(hi3))
        over = np.zeros((n, 4, 4), LD); allow = np.ones((n, 4, 4), LD)
        for v, o in ((hi3 - xc, xol - hi3), (xc - lo3, lo3 - xol)):
            den = (cl * v).sum((1, 2))
            eta = LD(U) * (20 + _div(17 * V + 17 * S + 18 * B, den))
            a = ulp2 + v * eta[:, None, None]
            worse = (o > 0) & (o * allow > over * a)
            over, allow = np.where(worse, o, over), np.where(worse, a, allow)
        rc = np.where(live[:, None, None], over / allow, 0).astype(np.float64)
        R.ratio_c = rc.reshape(n, -1).max(1)
        R.fail("(c) a point beyond its bound by more than the allowance", R.ratio_c > 1)
        K, KE, tol = K9, K9E, LD(0)
    # (d)
    bound_d = tol * np.abs(mass) + K * LD(U) * S
    R.ratio_d = np.where(live, _div(np.abs((cl * xol).sum((1, 2)) - mass), bound_d), 0).astype(np.float64)
    R.fail("(d) mass not conserved", (R.ratio_d > 1) | (~live & ~_same(xo, x)))
    # (e)
    R.ratio_e = np.zeros(n)
    if ref is not None:
        bound_e = 2 * tol * np.abs(mass) + KE * LD(U) * S
        R.ratio_e = np.where(live, _div((cl * np.abs(xol - ref[0].astype(LD))).sum((1, 2)), bound_e), 0).astype(np.float64)
        R.fail("(e) differs from the reference", R.ratio_e > 1)
    return R


def scaling_bad(out, out_scaled, e):
    """(f): slabs whose output for inputs scaled by 2^e is not exactly 2^e times the unscaled output"""
    ok = _same(out_scaled[0], np.ldexp(out[0], e)) & _same(out_scaled[1], np.ldexp(out[1], e)) & _same(out_scaled[2], np.ldexp(out[2], e))
    return np.nonzero(~(ok & (np.asarray(out_scaled[3]) == np.asarray(out[3]))))[0]
