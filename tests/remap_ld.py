"""remap_Q_ppm (prim_advection_mod.F90:98-356) in numpy longdouble with a rigorous forward-error bound per output, for any level count
and vert_remap_q_alg in (0, 2): what tests/remap_model.py restates in fp64, here vectorised over columns and tracers and carried as the
T(v, A, m) triples of tests/step_ld.py (value, magnitude >= |v|, rounding count; |fl - v| <= gamma_m(2^-53) * A for ANY fp64 evaluation
of the same expression: any association of its sums and products, fused or not, a division x/y counted as x * (1/y)).  Plain numpy; no HIP.

The grid part is a definition.  pio(k+1) = pio(k) + dp1(k) and pin(k+1) = pin(k) + dp2(k) are the fp64 SERIAL prefix sums of the
reference (:134-158) with pin(nlev+1) = pio(nlev+1) and pio(nlev+2) = pio(nlev+1) + 1, and kid(k) is the reference's bracket search
(:160-172) on those fp64 numbers -- the kernel keeps that order on purpose (k_remap phase 1a: "their roundings are part of the result").
For the operator call (dt = 0, divdp_proj = 0) dpo = dp1 exactly.  pio, pin, dpo and kid are EXACT fp64 INPUTS of everything below, so
no kid decision is ever excluded.

Rounding counts.  Two forms of each quantity are counted and the longer one is used: the reference's (ten grid coefficients r0..r9 =
dx(1..10, j), divisions) and k_remap's (five folded coefficients e1 = r0*r1, e2 = r0*r2, f3 = r3 + r4*(r5*(r6 - r7)), f8 = r4*r8,
f9 = r4*r9, reciprocals 1/dpo, hand-written FMAs; an FMA counts as its product and its sum).  Folding distributes a factor over a sum;
the magnitudes are the same in both forms because A of a product is the product of the A and A of a sum the sum of the A.  DX = dpo
(m = 0); a k-term sum of exact numbers has m = k - 1; x/y has m_x + m_y + 2 (reciprocal, product).
  grid   r0 = DX/(3-term sum)                      0 + 2 + 2 = 4      r1, r2 = (2-term)/(2-term)      1 + 1 + 2 = 4
         r3 = DX/(2-term)                          0 + 1 + 2 = 3      r4 = 1/(4-term)                 3 + 1     = 4
         r5 = (2 DX DX')/(2-term)                  1 + 1 + 2 = 4      r6, r7 = (2-term)/(2-term)                  4
         r8, r9 = DX*(2-term)/(2-term)             2 + 1 + 2 = 5
         e1, e2 = r0*r1, r0*r2                     4 + 4 + 1 = 9      f8, f9 = r4*r8, r4*r9           4 + 5 + 1 = 10
         f3 = r3 + r4*(r5*(r6 - r7)):  r6 - r7 5;  r5*: 4 + 5 + 1 = 10;  r4*: 4 + 10 + 1 = 15;  + r3: 16
  x2 = z2(k) = (pin(k+1) - (pio(kk) + pio(kk+1))*0.5) / dpo(kk):  2-term sum 1, halving exact, 2-term sum 2, division + 2 = 4
  a = Q/dpo            kernel Q * (1/dpo): 0 + 1 + 1 = 2          (reference: one division, 1)
  d = a(j+1) - a(j)    3;  where one side is the mirrored copy of the other (a(0) = a(1), a(nlev+1) = a(nlev)) both sides subtract
                       identical bits: T(0, 0, .)
  dma                  da: kernel e1*d + e2*d': 9 + 3 + 1 = 13, + 1 = 14;  reference r0*(r1*d + r2*d'): 4+3+1 = 8, + 1 = 9, 4+9+1 = 14.
                       min(|da|, 2|d'|, 2|d|) and copysign(., da): no count of their own (step_ld.minimum, copysign_le)       14
  ai                   kernel a + f3*d - f8*dma' + f9*dma: products 16+3+1 = 20, 10+14+1 = 25; 4-term sum + 3 = 28
                       reference a + r3*d + r4*(r5*(r6-r7)*d - r8*dma' + r9*dma): 10+3+1 = 14, 5+14+1 = 20; 3-term sum 22; r4*: 27;
                       r3*d: 7; 3-term sum + 2                                                                                = 29
  parabola             al, ar start as ai (29) or, flattened, as a (2).  al' = 3a - 2ar: 3*a: 3, sum: 30.  ar' = 3a - 2al': 31.
                       c0 = 1.5 a - (al + ar)/4   3-term sum of (3, 30, 31) = 33      (kernel fma(1.5, a, -0.25*(al+ar)): 32 + 1 = 33)
                       c1 = ar - al               32
                       c2 = -6a + 3(al + ar)      al + ar: 32, 3*: 33, sum: 34        (kernel fma(3, al+ar, -6a): the same)
                       alg 2, cells 1, 2, nlev-1, nlev: c0 = a (2), c1 = c2 = 0 exactly (T(0, 0, .))
  z powers             z1 = x2 + 1/2: 5;  zz2 = (x2*x2 - 1/4)/2: 4+4+1 = 9, + 1 = 10;  z3 = x2*x2*x2 + 1/8: 9+4+1 = 14, + 1 = 15
                       (-1/2 squared and cubed, and the halving, are exact)
  integral             c0*z1: 33+5+1 = 39;  c1*zz2: 32+10+1 = 43;  (c2*z3)*(1/3): 34+15+1 = 50, the rounded 1/3 (1): 52 (reference
                       (c2*z3)/3: the same);  3-term sum                                                                      = 54
  masso(kk)            serial sum of the kk - 1 <= nlev exact masses above cell kk (any association, so the segment tasks' prefixes
                       count the same)                                                                                   nlev - 1
  massn2               masso(kk) + integral * dpo(kk):  54 + 0 + 1 = 55;  2-term sum                      max(nlev - 1, 55) + 1
  output               massn2(k) - massn2(k-1)                                                            max(nlev - 1, 55) + 2
The products that involve x2 (its powers, c*z, the integral times dpo) take their magnitude from the factors' absolute errors
(step_ld.mul_tight: same counts): |x2| <= 1/2 while A_x2 ~ 2 pio(kk)/dpo(kk), and A_x2 cubed would swamp every level below the top.
The largest m is the output's: 73 at 72 levels, 65 at 64.  (Of the decisions below the largest is 66.)
The output's magnitude A holds the old-mass prefix sum_{j < kid(k)} |Q_j| twice and |c0| * A_z1 * dpo with A_z1 ~ 2 pio(kk)/dpo(kk): the
conditioning of the reference's own algorithm (a new level is the difference of two running column masses, and z2 the difference of
two interface pressures) -- tight at the top of a column, loose at the bottom.

Decisions.  Four sign tests, each a discriminant triple D:
  D1(j)  (a(j+1)-a(j)) * (a(j)-a(j-1)) <= 0                         dma(j) = 0                          m = 3+3+1 = 7
  D2(j)  (ar-a) * (a-al) <= 0                                       al = ar = a (flat cell)             m = 30+30+1 = 61
  D3(j)  (ar-al)*(a-(al+ar)/2) - (ar-al)^2/6 > 0                    al' = 3a - 2ar                      m = 64
         (ar-al: 30; a-(al+ar)/2: 3-term 31; product 62; square 61, *(1/6): 63; difference 64)
  D4(j)  (ar-al')*(a-(al'+ar)/2) + (ar-al')^2/6 < 0                 ar' = 3a - 2al'                     m = 66  (31; 32; 64; 63, 65; 66)
A decision is SAFE when |v| > bound(m, A) or A == 0 (exact zeros and differences of identical bits: both sides compute exactly 0 and
take the same branch).  Where d(j), dma(j) and dma(j+1) are such exact zeros -- always at j = 0 and j = nlev, through the mirrored
ghost cells -- ai(j) = a(j) + 0 is a(j) bit for bit on both sides, and the factor of D2 that subtracts the two is T(0, 0, .): the end
cells are flat by an exact tie, not by a rounding.  In a flat cell al = ar = a are the same bits, so ar - al and a - (al+ar)/2 are exactly 0 on both sides: D3 and
D4 are T(0, 0, .) there.  Output level k is SAFE when every decision that feeds it is: it reads the parabolas of cells kid(k) (massn2)
and kid(k-1) (massn1 = the level before), and the parabola of a cell c reads D2..D4(c) and, through ai(c-1), ai(c), D1(c-1), D1(c),
D1(c+1) (which look at cells c-2 .. c+2); masso takes no decision, nor do the piecewise-constant cells of alg 2.  On safe outputs fp64
and longdouble take the same branches and the triple bound is rigorous; on the others nothing is claimed pointwise.

The longdouble evaluation's own error is in step_ld.bound (gamma_m(2^-64)); every nonzero magnitude is range-checked by T itself.
"""
import numpy as np

from step_ld import LD, T, _check_range, absval, add, bound, cancel, copysign_le, exact, minimum, mul, mul_tight, neg, pow2, ratio, recip, select  # noqa: F401

M_AI = 29   # the reference's association of ai (the kernel's folded form gives 28)


def _zeros(shape):
    z = np.zeros(shape, dtype=LD)
    return T(z, z.copy(), 0)


def _cat(ts):
    return T(np.concatenate([t.v for t in ts]), np.concatenate([t.A for t in ts]), max(t.m for t in ts))


def _take(t, idx):
    """t[idx[k, c]][:, c] along axis 0 of t[j][q][c]: -> [k][q][c]"""
    ix = idx[:, None, :]
    return T(np.take_along_axis(t.v, ix, 0), np.take_along_axis(t.A, ix, 0), t.m)


def _safe(D):
    return (np.abs(D.v).astype(np.float64) > bound(D.m, D.A)) | (D.A == 0)


# ---- the grid part: fp64, the reference's order (a definition) ----
def grid_fp64(d1, d2):
    """d1, d2[nlev][C] -> dpo[nlev+4][C] (index j+1, j = -1..nlev+2), pio[nlev+3][C] (index j, 1..nlev+2), pin[nlev+2][C], kid[nlev][C]
    (kid(k), k = 1..nlev, at [k-1]).  Asserts the precondition of the bracket search: dp1 > 0, dp2 > 0 and pin(k+1) < pio(nlev+1) + 1."""
    d1, d2 = np.asarray(d1, dtype=np.float64), np.asarray(d2, dtype=np.float64)
    nlev, C = d1.shape
    assert (d1 > 0).all() and (d2 > 0).all() and np.isfinite(d1).all() and np.isfinite(d2).all(), "dp1 > 0 and dp2 > 0"
    dpo = np.zeros((nlev + 4, C)); dpo[2:nlev + 2] = d1
    pio, pin = np.zeros((nlev + 3, C)), np.zeros((nlev + 2, C))
    for k in range(1, nlev + 1):
        pin[k + 1] = pin[k] + d2[k - 1]
        pio[k + 1] = pio[k] + dpo[k + 1]
    pio[nlev + 2] = pio[nlev + 1] + 1.
    assert (pio[nlev + 2] > pio[nlev + 1]).all(), "sum(dp1) + 1 > sum(dp1): the last level's search ends on it"
    assert (pin[2:nlev + 1] < pio[nlev + 2]).all(), "pin(k+1) < pio(nlev+1) + 1 for every k < nlev"
    pin[nlev + 1] = pio[nlev + 1]
    dpo[1], dpo[0], dpo[nlev + 2], dpo[nlev + 3] = dpo[2], dpo[3], dpo[nlev + 1], dpo[nlev]
    kid = np.zeros((nlev, C), dtype=np.int64)
    for k in range(1, nlev + 1):
        gt = pio[k:nlev + 3] > pin[k + 1]              # while (pio(kk) <= pin(k+1)) kk++ from kk = k
        assert gt.any(axis=0).all()
        kid[k - 1] = np.minimum(k + np.argmax(gt, axis=0) - 1, nlev)
    return dpo, pio, pin, kid


def check_inputs(dp1, dp2):
    """the precondition on [E][nlev][4][4] arrays (no array that fails it may reach a device)"""
    E, nlev = dp1.shape[:2]
    grid_fp64(np.moveaxis(np.asarray(dp1).reshape(E, nlev, 16), 1, 0).reshape(nlev, -1),
              np.moveaxis(np.asarray(dp2).reshape(E, nlev, 16), 1, 0).reshape(nlev, -1))


def _coefficients(dpo, nlev):
    """-> e1, e2 [nlev+2][1][C] (cells j = 0..nlev+1), f3, f8, f9 [nlev+1][1][C] (interfaces j = 0..nlev)"""
    X = exact(dpo[:, None, :])

    def sl(o, n):
        return X[o:o + n]
    n = nlev + 2
    m_, c_, p_ = sl(0, n), sl(1, n), sl(2, n)
    r0 = mul(c_, recip(add(m_, c_, p_)))
    r1 = mul(add(pow2(m_, 2.), c_), recip(add(p_, c_)))
    r2 = mul(add(c_, pow2(p_, 2.)), recip(add(m_, c_)))
    e1, e2 = mul(r0, r1), mul(r0, r2)
    n = nlev + 1
    m_, c_, p_, pp = sl(0, n), sl(1, n), sl(2, n), sl(3, n)
    r3 = mul(c_, recip(add(c_, p_)))
    r4 = recip(add(m_, c_, p_, pp))
    r5 = mul(pow2(mul(p_, c_), 2.), recip(add(c_, p_)))
    r6 = mul(add(m_, c_), recip(add(pow2(c_, 2.), p_)))
    r7 = mul(add(pp, p_), recip(add(pow2(p_, 2.), c_)))
    r8 = mul(mul(c_, add(m_, c_)), recip(add(pow2(c_, 2.), p_)))
    r9 = mul(mul(p_, add(p_, pp)), recip(add(c_, pow2(p_, 2.))))
    f3 = add(r3, mul(r4, mul(r5, add(r6, neg(r7)))))
    f8, f9 = mul(r4, r8), mul(r4, r9)
    assert (r0.m, r1.m, r3.m, r4.m, r5.m, r6.m, r8.m, e1.m, f3.m, f8.m) == (4, 4, 3, 4, 4, 4, 5, 9, 16, 10)
    return e1, e2, f3, f8, f9


def remap_columns(Q, d1, d2, alg=0):
    """Q[nlev][nq][C], d1, d2[nlev][C] -> (out: T [nlev][nq][C], safe: bool [nlev][nq][C], kid [nlev][C])"""
    assert alg in (0, 2)
    Q = np.asarray(Q, dtype=np.float64)
    nlev, nq, C = Q.shape
    dpo, pio, pin, kid = grid_fp64(d1, d2)
    e1, e2, f3, f8, f9 = _coefficients(dpo, nlev)
    # z2(k) and the powers of integrate_parabola
    kk = kid                                                            # [nlev][C], values 0..nlev (kid(k) >= k - 1; kid(1) >= 1)
    assert kk.min() >= 1
    g = lambda a: np.take_along_axis(a, kk, 0)                          # noqa: E731
    dpk = exact(g(dpo[1:])[:, None, :])                                 # dpo(kk) = dpo[kk + 1]
    x2 = mul(add(exact(pin[2:nlev + 2]), neg(pow2(add(exact(g(pio)), exact(g(pio[1:]))), 0.5))), recip(exact(g(dpo[1:]))))
    x2 = T(x2.v[:, None, :], x2.A[:, None, :], x2.m)
    half = exact(np.float64(0.5))
    z1 = add(x2, half)
    zz2 = pow2(add(mul_tight(x2, x2), neg(exact(np.float64(0.25)))), 0.5)
    z3 = add(mul_tight(mul_tight(x2, x2), x2), exact(np.float64(0.125)))
    assert (x2.m, z1.m, zz2.m, z3.m) == (4, 5, 10, 15)
    # cell means with the mirrored ghost cells: index j + 1, j = -1..nlev+2
    a = mul(exact(Q), recip(exact(dpo[2:nlev + 2, None, :])))
    af = _cat([a[1:2], a[0:1], a, a[nlev - 1:nlev], a[nlev - 2:nlev - 1]])
    d = add(af[1:], neg(af[:-1]))                                       # d(j) = a(j+1) - a(j) at [j + 1], j = -1..nlev+1
    mirror = np.zeros((nlev + 3, 1, 1), dtype=bool); mirror[1] = True; mirror[nlev + 1] = True
    d = cancel(d, mirror)
    assert (a.m, d.m) == (2, 3)
    # dma(j), j = 0..nlev+1
    dp_, dm_ = d[1:nlev + 3], d[0:nlev + 2]
    da = add(mul(e1, dp_), mul(e2, dm_))
    mag = minimum(absval(da), pow2(absval(dm_), 2.), pow2(absval(dp_), 2.))
    D1 = mul(dp_, dm_)
    s1 = _safe(D1)
    dma = select(D1.v <= 0, _zeros(D1.v.shape), copysign_le(mag, da))
    assert (da.m, dma.m, D1.m) == (14, 14, 7)
    del da, mag, D1
    # ai(j), j = 0..nlev
    n = nlev + 1
    t3, t8, t9 = mul(f3, d[1:n + 1]), neg(mul(f8, dma[1:n + 1])), mul(f9, dma[0:n])
    ai = add(af[1:n + 1], t3, t8, t9)
    same = (t3.A == 0) & (t8.A == 0) & (t9.A == 0)      # ai(j) is a(j) bit for bit: every other term is an exact zero on both sides
    assert ai.m == 28
    ai = T(ai.v, ai.A, M_AI)
    s_ai = s1[0:n] & s1[1:n + 1]
    del dma, d
    # the limited parabola of cells j = 1..nlev
    al, ar, aj = ai[0:nlev], ai[1:nlev + 1], af[2:nlev + 2]
    D2 = mul(cancel(add(ar, neg(aj)), same[1:nlev + 1]), cancel(add(aj, neg(al)), same[0:nlev]))
    flat = D2.v <= 0
    s2 = _safe(D2)
    al, ar = select(flat, aj, al), select(flat, aj, ar)
    sixth = recip(exact(np.float64(6.0)))
    w = cancel(add(ar, neg(al)), flat)
    mid = cancel(add(aj, neg(pow2(al, 0.5)), neg(pow2(ar, 0.5))), flat)
    D3 = add(mul(w, mid), neg(mul(mul(w, w), sixth)))
    lo = D3.v > 0
    s3 = _safe(D3)
    three = exact(np.float64(3.0))
    al = select(lo, add(mul(three, aj), neg(pow2(ar, 2.))), al)
    w = cancel(add(ar, neg(al)), flat)
    mid = cancel(add(aj, neg(pow2(al, 0.5)), neg(pow2(ar, 0.5))), flat)
    D4 = add(mul(w, mid), mul(mul(w, w), sixth))
    hi = D4.v < 0
    s4 = _safe(D4)
    ar = select(hi, add(mul(three, aj), neg(pow2(al, 2.))), ar)
    assert (D2.m, D3.m, D4.m, al.m, ar.m) == (61, 64, 66, 30, 31)
    del D2, D3, D4, w, mid
    c0 = add(mul(exact(np.float64(1.5)), aj), neg(pow2(al, 0.25)), neg(pow2(ar, 0.25)))
    c1 = cancel(add(ar, neg(al)), flat)
    c2 = add(mul(exact(np.float64(-6.0)), aj), mul(three, add(al, ar)))
    assert (c0.m, c1.m, c2.m) == (33, 32, 34)
    s_cell = s_ai[0:nlev] & s_ai[1:nlev + 1] & s2 & s3 & s4            # cell j at [j - 1]
    if alg == 2:
        pc = np.zeros((nlev, 1, 1), dtype=bool); pc[[0, 1, nlev - 2, nlev - 1]] = True
        c0 = select(pc, aj, c0); c1 = cancel(c1, pc); c2 = cancel(c2, pc)
        s_cell = s_cell | pc
    del al, ar, ai
    # new-grid running mass and its differences
    third = recip(exact(np.float64(3.0)))
    ci = kk - 1                                                         # cell kid(k) at [kid(k) - 1]
    integ = add(mul_tight(_take(c0, ci), z1), mul_tight(_take(c1, ci), zz2), mul(mul_tight(_take(c2, ci), z3), third))
    assert integ.m == 54
    ql = Q.astype(LD)
    zero = np.zeros((1, nq, C), dtype=LD)
    pre = T(np.concatenate([zero, np.cumsum(ql, axis=0)]), np.concatenate([zero, np.cumsum(np.abs(ql), axis=0)]), nlev - 1)
    massn2 = add(_take(pre, ci), mul_tight(integ, dpk))                       # masso(kk) = cells 1 .. kk-1
    prev = _cat([_zeros((1, nq, C)), massn2[0:nlev - 1]])
    out = add(massn2, neg(prev))
    assert out.m == max(nlev - 1, 55) + 2
    s_k = np.take_along_axis(s_cell, ci[:, None, :], 0)
    safe = s_k & np.concatenate([np.ones((1, nq, C), dtype=bool), s_k[0:nlev - 1]])
    return out, safe, kid


def _cols(x, E, nlev):
    """[E][..][nlev][4][4] -> [nlev][..][E*16]"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 4:
        return np.moveaxis(x.reshape(E, nlev, 16), 1, 0).reshape(nlev, E * 16)
    nq = x.shape[1]
    return np.transpose(x.reshape(E, nq, nlev, 16), (2, 1, 0, 3)).reshape(nlev, nq, E * 16)


def _back(y, E, nq, nlev):
    """[nlev][nq][E*16] -> [E][nq][nlev][4][4]"""
    return np.ascontiguousarray(np.transpose(y.reshape(nlev, nq, E, 16), (2, 1, 0, 3))).reshape(E, nq, nlev, 4, 4)


def remap_q_ppm(Qdp, dp1, dp2, alg=0):
    """Qdp[E][q][k][4][4], dp1, dp2[E][k][4][4] (the arrays of HipMod.remap_q_ppm) -> (T, safe, kid[E][k][4][4]) in that layout"""
    Qdp = np.asarray(Qdp, dtype=np.float64)
    E, nq, nlev = Qdp.shape[:3]
    out, safe, kid = remap_columns(_cols(Qdp, E, nlev), _cols(dp1, E, nlev), _cols(dp2, E, nlev), alg)
    kid = np.moveaxis(kid.reshape(nlev, E, 16), 0, 1).reshape(E, nlev, 4, 4)
    return T(_back(out.v, E, nq, nlev), _back(out.A, E, nq, nlev), out.m), _back(safe, E, nq, nlev), kid


# ---- the inputs of the CPU and the GPU tests: from seeds only, no geometry ----
GRIDS = ("gentle", "squeeze", "random", "identity", "thin")
TRACERS = ("sine", "bell", "noise", "spikes", "ramp", "signed")
NELEM = 24                      # ne 2
QSIZES = (1, 3, 16, 19, 20, 35)   # remap_left with 16 tracer slots: segment tasks only (1, 3: the 2^-200 and 2^+-200 slots), a whole
#                                   round (16), a round and 3 segment tracers (19: the last one at 2^200), a fourth leftover that takes
#                                   a partly idle round (20), two rounds and 3 segment tracers (35)


def hvcoord(nlev):
    """the reference's hybrid coefficients: acme-72 (the package's default) or 12k_top-64 (tests/golden/vcoord)"""
    import os
    from transport_se_amd.hybvcoord import HvCoord
    if nlev == 72:
        return HvCoord()
    assert nlev == 64
    vc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vcoord")
    return HvCoord(os.path.join(vc, "12k_top-64m.ascii"), os.path.join(vc, "12k_top-64i.ascii"))


def grid_family(e):
    return GRIDS[e * len(GRIDS) // NELEM]


def tracer_family(q):
    return TRACERS[q % len(TRACERS)]


def exponents(qsize):
    """slot scalings 2^-200 .. 2^200 (as _scaled of test_gpu_step_pointwise.py)"""
    return np.rint(np.linspace(-200, 200, qsize)).astype(int) if qsize > 1 else np.array([-200])


def grids(nlev, seed=0):
    """dp1, dp2[E][nlev][4][4]: per-column grids on the reference thicknesses, a family per block of elements.  The target grid dp2 is
    the reference's dp at a column's own surface pressure (except `gentle`, which displaces the interfaces of dp1 = that dp)."""
    hv = hvcoord(nlev)
    rng = np.random.default_rng(1000 * nlev + seed)
    ps = hv.ps0 * (1 + 0.02 * rng.standard_normal((NELEM, 1, 4, 4)).clip(-2, 2))
    ref = np.diff(hv.hyai)[None, :, None, None] * hv.ps0 + np.diff(hv.hybi)[None, :, None, None] * ps
    assert ref.shape[1] == nlev and (ref > 0).all()
    dp1, dp2 = ref.copy(), ref.copy()
    for e in range(NELEM):
        fam, r = grid_family(e), ref[e]
        if fam == "gentle":      # interface k+1 moves by less than 0.45 of the thinner layer next to it: kid(k) in {k, k+1} (lockstep loop)
            dlt = np.zeros((nlev + 1, 4, 4))
            dlt[1:nlev] = 0.45 * rng.uniform(-1, 1, (nlev - 1, 4, 4)) * np.minimum(r[:-1], r[1:])
            dp2[e] = r + np.diff(dlt, axis=0)
        elif fam == "squeeze":   # 0.3x above, 1.7x below (test_remap_column_loop_variants): displaced by many layers (generic loop)
            dp1[e] = r * np.where(np.arange(nlev) < nlev // 2, 0.3, 1.7)[:, None, None]
        elif fam == "random":
            dp1[e] = r * rng.uniform(0.4, 1.6, r.shape)
        elif fam == "thin":      # one layer at 1e-3 of its neighbours
            k0 = rng.integers(2, nlev - 2, (4, 4))
            jj, ii = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
            dp1[e][k0, jj, ii] = 1e-3 * np.minimum(r[k0 - 1, jj, ii], r[k0 + 1, jj, ii])
        if fam != "identity":
            dp1[e] *= dp2[e].sum(0, keepdims=True) / dp1[e].sum(0, keepdims=True)   # sum(dp1) == sum(dp2) to rounding
    check_inputs(dp1, dp2)
    return dp1, dp2


def mixing_ratio(family, nlev, rng):
    """a[E][nlev][4][4] of one tracer family"""
    shp = (NELEM, nlev, 4, 4)
    s = (np.arange(nlev)[None, :, None, None] + 0.5) / nlev
    col = lambda lo, hi: rng.uniform(lo, hi, (NELEM, 1, 4, 4))   # noqa: E731
    if family == "sine":       # interior extrema
        return 0.6 + 0.4 * np.sin(2 * np.pi * col(2.0, 4.0) * s + col(0, 2 * np.pi))
    if family == "bell":       # narrow bell: e^-25 half the column away from its centre
        return np.exp(-25.0 * ((s - col(0.3, 0.7)) / 0.5) ** 2)
    if family == "noise":
        return rng.uniform(0.0, 1.0, shp)
    if family == "spikes":     # 5 % spikes of 50 over exact zeros (no two in adjacent cells: their means would differ by rounding only)
        on = rng.uniform(size=shp) < 0.05
        on[:, 1:] &= ~on[:, :-1]
        return np.where(on, 50.0, 0.0)
    if family == "ramp":       # monotone
        return 0.1 + col(0.5, 1.5) * s
    if family == "signed":
        return rng.uniform(-1.0, 1.0, shp)
    raise ValueError(family)


def inputs(nlev, qsize, seed=0):
    """(Qdp[E][q][k][4][4], dp1, dp2): tracer slot q holds family TRACERS[q % 6] at 2^exponents(qsize)[q]; element e grid_family(e)"""
    dp1, dp2 = grids(nlev, seed)
    rng = np.random.default_rng(77 + 1000 * nlev + 10 * qsize + seed)
    ex = exponents(qsize)
    Q = np.stack([np.ldexp(mixing_ratio(tracer_family(q), nlev, rng) * dp1, int(ex[q])) for q in range(qsize)], axis=1)
    assert np.isfinite(Q).all()
    return Q, dp1, dp2


def uniform_inputs(nlev, seed=0):
    """the uniform mixing ratios Q = c*dp1, c = 0.75, 1, 2^-200 (outside the pointwise claim: every decision on them is rounding noise)"""
    dp1, dp2 = grids(nlev, seed)
    c = np.array([0.75, 1.0, 2.0 ** -200])
    return c[None, :, None, None, None] * dp1[:, None], dp1, dp2, c


def column_mass_ratio(got, Qdp, t):
    """sum_k out == sum_k Q for EVERY column, unsafe ones included: max of |sum_k got - sum_k Q| / bound and the ratio per column.
    Rigorous without any decision: sum_k got telescopes to the fp64 massn2(nlev) plus one rounding per difference (<= 2^-53 |got_k|
    each), and massn2(nlev) = masso(nlev) + (c0*z1 + c1*zz2 + c2*z3/3) * dpo(nlev) takes no decision at all -- ai(nlev) is a(nlev) bit
    for bit (module docstring), so D2(nlev) is an exact tie and cell nlev is flat (c0 = a, c1 = c2 = 0) on both sides whatever the
    cells above did.  Its count is the output's less one (the difference), and its magnitude at most A of output nlev.  Against
    sum_k Q itself one more unit of the same magnitude: in exact arithmetic massn2(nlev) - sum_k Q = Q(nlev) * (z2(nlev) - 1/2), and
    |z2(nlev) - 1/2| = |pio(nlev+1) - pio(nlev) - dpo(nlev)| / (2 dpo(nlev)) <= 2^-54 pio(nlev+1)/dpo(nlev), the rounding of the last
    prefix sum, while A holds |a(nlev)| * (pio(nlev)/dpo(nlev) + 1/2) * dpo(nlev)."""
    got, Qdp = np.asarray(got, dtype=np.float64), np.asarray(Qdp, dtype=np.float64)
    err = np.abs(got.astype(LD).sum(axis=2) - Qdp.astype(LD).sum(axis=2)).astype(np.float64)
    b = bound(t.m, t.A[:, :, -1]) + 2.0 ** -53 * (1 + 2.0 ** -40) * np.abs(got).sum(axis=2)
    r = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1e-300))
    return float(r.max()), r
