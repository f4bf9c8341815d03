"""The element partials of the DCMIP error norms (tse_norm_reference / tse_norm_partials), restated in numpy IN THE DEVICE'S ORDER, an exact
referee for them, and the error bounds the norm tests hold them to.

Terms.  For a point p of element e and level k, with Q0 the reference field, Qf the final one, dV = colw[e][p] * dh[k]:
    dq = Qf - Q0,  dev = |Q0 - avg|,   t0 = |dq| * dV,  t1 = dev * dV,  t2 = (dq * dq) * dV,  t3 = (dev * dev) * dV
each operation rounded once to fp64 (no contraction): the numbers diagnostics.dcmip_norms forms, and the numbers k_norm_partials forms.

The device's order (csrc/tse_kernels.h, "THE ORDER").  The levels are cut into LG = 4 groups of nlev/4 consecutive levels.
    1. per point and group: s = 0; for k ascending in the group: s = s + t(p, k)
    2. per point:           c(p) = ((s(p,0) + s(p,1)) + s(p,2)) + s(p,3)
    3. per element:         S = 0; for p = 0 .. 15 ascending, owned points only: S = S + c(p)
sum0 (the element's unweighted sum of Q0) takes the same route.

The referee adds the same terms with math.fsum: the exact sum, rounded once.

Bounds (u = 2^-53, gamma(m) = m u / (1 - m u); Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: a sum of n terms formed by
n - 1 fp64 additions IN ANY ORDER differs from the exact sum by at most gamma(n-1) * sum |terms|):
  * an element sum of n = (owned points) * nlev non-negative terms: |S - exact| <= gamma(n-1) * exact.  The referee is the exact sum rounded
    once, so against it the bound is (gamma(n-1) + 2u) * referee (element_bound).
  * a numpy sum over a [nlev][ncol] array: numpy adds pairwise in blocks of at most 128 terms, a block with 8 accumulators of 16 terms each and a
    3-level tree over them, one more addition per halving above 128 terms; where it does not fuse the two axes it adds the nlev rows one after
    the other.  Either way a term passes through at most M_NP = nlev + 20 + ceil(log2(max(N/128, 1))) additions, so the error is at most
    gamma(M_NP) * sum |terms| (numpy_depth).
  * forward_bounds() combines them into the bound on |L(norms_from_partials) - L(dcmip_norms)| / L(dcmip_norms); its docstring has the algebra.
"""
import math

import numpy as np

LG = 4           # level groups (NORM_LG of csrc/tse_kernels.h)
U = 2.0 ** -53


def gamma(m):
    return m * U / (1.0 - m * U)


def numpy_depth(nlev, n):
    """an upper limit of the additions a term passes through in a numpy sum over n = nlev * ncol fp64 numbers (module docstring)"""
    return nlev + 20 + int(math.ceil(math.log2(max(n / 128.0, 1.0))))


def terms(q0, qf, colw, dh, avg):
    """t[4][nelem][nlev][16]: the four summands at EVERY point (owned or not), each operation rounded once"""
    E, nlev = q0.shape[:2]
    q0 = q0.reshape(E, nlev, 16); qf = qf.reshape(E, nlev, 16)
    dV = colw.reshape(E, 1, 16) * np.asarray(dh).reshape(1, nlev, 1)
    dq = qf - q0
    dev = np.abs(q0 - avg)
    return np.stack([np.abs(dq) * dV, dev * dV, (dq * dq) * dV, (dev * dev) * dV])


def _point_sums(t):
    """steps 1 and 2 of the order: t[..., nlev, 16] -> c[..., 16]"""
    nlev = t.shape[-2]
    assert nlev % LG == 0
    per = nlev // LG
    s = []
    for g in range(LG):
        a = np.zeros(t.shape[:-2] + (16,))
        for k in range(g * per, (g + 1) * per):
            a = a + t[..., k, :]
        s.append(a)
    return ((s[0] + s[1]) + s[2]) + s[3]


def _element_sum(c, owner):
    """step 3: c[..., nelem, 16], owner[nelem][16] -> S[..., nelem]"""
    tot = np.zeros(c.shape[:-1])
    for p in range(16):
        tot = np.where(owner[:, p] != 0, tot + c[..., p], tot)
    return tot


def element_sum0(q0, owner):
    """sum0[nelem] of tse_norm_reference: the unweighted sum of Q0 over owned points and levels, in the device's order"""
    E, nlev = q0.shape[:2]
    return _element_sum(_point_sums(q0.reshape(E, nlev, 16)), owner.reshape(E, 16))


def model_avg(q0, owner):
    """avg as PrimRun.norm_reference forms it: the exact sum of the element sums over (nlev * ncol), rounded once each"""
    return math.fsum(element_sum0(q0, owner).tolist()) / (q0.shape[1] * int(owner.sum()))


def element_partials(q0, qf, owner, colw, dh, avg, plant=None, colw_all=None, avg_weighted=None):
    """out[nelem][8] of tse_norm_partials in the device's order.  q0, qf [nelem][nlev][4][4]; owner, colw [nelem][4][4]; dh[nlev].
    plant: one deliberate error, for the tests that show the bounds catching it --
      "owner": the owner mask ignored (every point counted; needs colw_all, the weight at every point),
      "dh":    dh applied in reversed level order,
      "mean":  dev taken against avg_weighted (the dV-weighted mean) instead of the unweighted one."""
    E, nlev = q0.shape[:2]
    own = owner.reshape(E, 16)
    if plant == "owner":
        own = np.ones_like(own); colw = colw_all
    elif plant == "dh":
        dh = np.asarray(dh)[::-1]
    elif plant == "mean":
        avg = avg_weighted
    else:
        assert plant is None, plant
    t = terms(q0, qf, colw, dh, avg)
    out = np.empty((E, 8))
    out[:, :4] = _element_sum(_point_sums(t), own).T
    mask = np.broadcast_to((own != 0)[:, None, :], (E, nlev, 16))
    out[:, 4] = np.where(mask, t[0], 0.0).max(axis=(1, 2))
    out[:, 5] = np.where(mask, t[1], 0.0).max(axis=(1, 2))
    qfr = qf.reshape(E, nlev, 16)
    out[:, 6] = np.where(mask, qfr, -np.inf).max(axis=(1, 2))
    out[:, 7] = np.where(mask, qfr, np.inf).min(axis=(1, 2))
    return out


def exact_element_sums(q0, qf, owner, colw, dh, avg):
    """the referee: (S[nelem][4], n[nelem]) -- math.fsum over the same terms at the owned points, and the number of terms of each element"""
    E, nlev = q0.shape[:2]
    t = terms(q0, qf, colw, dh, avg)
    own = owner.reshape(E, 16) != 0
    S = np.zeros((E, 4))
    for e in range(E):
        for j in range(4):
            S[e, j] = math.fsum(t[j, e][:, own[e]].ravel().tolist())
    return S, own.sum(1) * nlev


def exact_sum0(q0, owner):
    E, nlev = q0.shape[:2]
    own = owner.reshape(E, 16) != 0
    x = q0.reshape(E, nlev, 16)
    return np.array([math.fsum(x[e][:, own[e]].ravel().tolist()) for e in range(E)])


def element_bound(S_exact, n):
    """|device-order sum - referee| <= (gamma(n-1) + 2u) * referee for n non-negative terms (module docstring); 0 for an empty element"""
    n = np.asarray(n, dtype=np.float64)
    g = np.where(n > 0, (n - 1) * U / (1.0 - (n - 1) * U) + 2 * U, 0.0)
    return g.reshape(-1, *([1] * (np.ndim(S_exact) - 1))) * np.abs(S_exact)


def exact_globals(q0, qf, owner, colw, dh, avg):
    """the referee's global sums and maxima: dict(S[4], m4, m5, W = sum dV, wmax = max dV, absmean = mean |Q0|) over the owned points"""
    E, nlev = q0.shape[:2]
    t = terms(q0, qf, colw, dh, avg)
    own = np.broadcast_to((owner.reshape(E, 1, 16) != 0), (E, nlev, 16))
    dV = (colw.reshape(E, 1, 16) * np.asarray(dh).reshape(1, nlev, 1))[own]
    return dict(S=[math.fsum(t[j][own].tolist()) for j in range(4)], m4=float(t[0][own].max()), m5=float(t[1][own].max()),
                W=math.fsum(dV.tolist()), wmax=float(dV.max()), absmean=math.fsum(np.abs(q0.reshape(E, nlev, 16)[own]).tolist()) / dV.size)


def forward_bounds(q0, qf, owner, colw, dh, avg):
    """dict(L1, L2, Linf, davg): bounds on |x(norms_from_partials) - x(dcmip_norms)| / x(dcmip_norms), and on |avg(new) - qi.mean()|.

    Notation: N = nlev * ncol, n_max = the most terms of an element, e_d = gamma(n_max - 1) + u (an element sum, then the exact sum of the
    element sums rounded once), e_n = gamma(M_NP) (a numpy sum).  S_j are the exact sums of the fp64 terms.
      davg: the element sums of Q0 carry gamma(n_max - 1), fsum one rounding, the division one; qi.mean() carries e_n and one division:
            |avg_new - qi.mean()| <= (gamma(n_max-1) + e_n + 3u) * mean|Q0| =: d.
      t0, t2 do not contain avg: both routes add the SAME numbers, so s0, s2 differ by the summation errors alone.
      t1 = fl(fl|Q0 - avg| * dV): moving avg by d moves fl|Q0 - avg| by at most d + 2u dev, hence S_1 by at most r1 * S_1,
            r1 = (1 + 4u) d W / S_1 + 6u,   W = sum dV.
      t3 = fl(fl(dev * dev) * dV): dev_a^2 - dev_b^2 = (dev_a - dev_b)(dev_a + dev_b), so S_3 moves by at most r3 * S_3,
            r3 = (1 + 8u) (2 d S_1 + d^2 W) / S_3 + 10u.
      max t1 moves by at most r5 * m5, r5 = (1 + 4u) d max(dV) / m5 + 6u; max t0 is the same number on both routes.
      L1 = s0/s1: the two routes differ by at most (1+e_d)(1+e_n)(1+u) / ((1-e_d)(1-e_n)(1-r1)(1-u)) - 1 (numerator and denominator of
            each route once, one division each).
      L2 = sqrt(s2)/sqrt(s3): a square root halves a relative error and rounds once (two roots and a division per route):
            sqrt((1+e_d)(1+e_n) / ((1-e_d)(1-e_n)(1-r3))) * ((1+u)/(1-u))^3 - 1.
      Linf = m4/m5: (1+u) / ((1-u)(1-r5)) - 1."""
    E, nlev = q0.shape[:2]
    g = exact_globals(q0, qf, owner, colw, dh, avg)
    nmax = int(owner.reshape(E, 16).sum(1).max()) * nlev
    N = nlev * int(owner.sum())
    gm = gamma(nmax - 1)
    e_d = gm + U + gm * U
    e_n = gamma(numpy_depth(nlev, N))
    d = (gm + e_n + 3 * U) * g["absmean"]
    S = g["S"]
    r1 = (1 + 4 * U) * d * g["W"] / S[1] + 6 * U
    r3 = (1 + 8 * U) * (2 * d * S[1] + d * d * g["W"]) / S[3] + 10 * U
    r5 = (1 + 4 * U) * d * g["wmax"] / g["m5"] + 6 * U
    lp = math.log1p   # (the products of factors 1 +- 1e-14 are formed as sums of logarithms: 1 + x - 1 would lose x's last digits)
    both = lp(e_d) + lp(e_n) - lp(-e_d) - lp(-e_n)
    return dict(L1=math.expm1(both + lp(U) - lp(-r1) - lp(-U)),
                L2=math.expm1(0.5 * (both - lp(-r3)) + 3 * (lp(U) - lp(-U))),
                Linf=math.expm1(lp(U) - lp(-U) - lp(-r5)), davg=d)
