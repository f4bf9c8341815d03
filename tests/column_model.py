"""The model of tse_column_view: the three vertical scans of the primitive equations in numpy, operation for operation as the header
states them, in fp64 (the model the device is compared with in bits) or, the same code, in np.longdouble (the referee of the bounds).
Plain numpy; no HIP import.

Arrays carry the levels on their FIRST axis, level 0 at the model top, and any shape behind it (columns); a surface field has that shape
without the level axis.  The type of `dp` (or `p`) decides the arithmetic; scalars (ptop, rgas) are converted to it, exactly.

  pint(dp, ptop)                       pi[0] = ptop; pi[k+1] = pi[k] + dp[k]
  pmid(dp, ptop)                       p[0] = ptop + dp[0]*0.5; p[k] = (p[k-1] + dp[k-1]*0.5) + dp[k]*0.5
  phi(tv, dp, phis, rgas, p | ptop)    preq_hydrostatic (src/asp_tests.F90:1708-1757 of the reference): hkk = (dp*0.5)/p, hkl = 2*hkk,
                                       t = rgas*tv; phii[n-1] = t*hkl, phii[k] = phii[k+1] + t*hkl; phi[n-1] = phis + t*hkk,
                                       phi[k] = (phis + phii[k+1]) + t*hkk
  omega(vgrad_p, divdp, p | dp, ptop)  E3SM's preq_omega_ps: ckk = 0.5/p, ckl = 2*ckk; om[0] = vgrad_p/p - ckk*divdp, s = divdp[0];
                                       om[k] = (vgrad_p/p - ckl*s) - ckk*divdp, then s = s + divdp[k]
With p=None phi and omega use pmid(dp, ptop).  numpy evaluates every operator as one rounded operation of the arrays' type and contracts
nothing, so each line above is the sequence of roundings the header names.

THE BOUNDS (u = 2^-53; against the same lines evaluated in longdouble, whose own error of 2^-64 per operation is far below u).  First
order in u throughout; every count carries ONE MORE than the roundings it names, which pays for the referee's own roundings and for the
second-order terms (at most (2n)^2 u^2 relative, n <= 81).
  p     every summand is positive, p[k] is reached by 2k + 1 additions (*0.5 is exact), pi[k] by k:
           |err p[k]| <= (2k + 2) u p[k],   |err pi[k]| <= (k + 1) u pi[k].
        cp[k] = 2k + 1 below when the op forms p itself and 0 when p is given (an input is exact).
  phi   a[k] = t*hkl and b[k] = t*hkk carry the roundings of p, of the division, of t and of the product (2*hkk is exact):
           |err a[k]| <= (cp[k] + 3 + 1) u |a[k]|, the same for b[k].
        A[j] = |a[j]| + ... + |a[n-1]|, the running sum of absolute values.  The additions: phii[j] (j = n-2 .. k+1) each u A[j];
        phis + phii[k+1] (k < n-1) u (|phis| + A[k+1]); the last one u (|phis| + A[k+1] + |b[k]|).  So
           |err phi[k]| <= u [ sum_{j>k} (cp[j] + 4) |a[j]| + (cp[k] + 4) |b[k]| + sum_{j=k+1}^{n-2} A[j] + (k < n-1) (|phis| + A[k+1])
                               + |phis| + A[k+1] + |b[k]| ].
  omega q = vgrad_p/p carries cp + 1 roundings, ckl = 2*(0.5/p) cp + 1, c = ckk*divdp cp + 2.  D[j] = |divdp[0]| + ... + |divdp[j-1]|;
        s of level k is reached by k - 1 additions, the j-th of at most u D[j+1]:  |err s| <= u (D[2] + ... + D[k]).  The product ckl*s
        adds one rounding, the two subtractions u (|q| + ckl D[k]) and u (|q| + ckl D[k] + |c|):
           |err om[k]| <= u [ (cp + 2) |q| + (k > 0) ((cp + 3) ckl D[k] + ckl (D[2] + ... + D[k])) + (cp + 3) |c|
                              + (k > 0) (|q| + ckl D[k]) + |q| + (k > 0) ckl D[k] + |c| ].
tests/test_column_cpu.py measures the worst ratio of |model - referee| to these bounds and shows six planted errors far above them;
tests/test_gpu_column_view.py holds the device to the same bounds."""
import numpy as np

U = 2.0 ** -53
OPS = ("pint", "pmid", "phi", "omega")
PLANTS = ("hkk_for_hkl", "half_dropped", "pint_for_pmid", "phii_shifted", "s_early", "reversed")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def pint(dp, ptop):
    dp = np.asarray(dp)
    out = np.empty((dp.shape[0] + 1,) + dp.shape[1:], dtype=dp.dtype)
    out[0] = dp.dtype.type(ptop)
    for k in range(dp.shape[0]):
        out[k + 1] = out[k] + dp[k]
    return out


def pmid(dp, ptop, plant=None):
    dp = np.asarray(dp)
    half = dp.dtype.type(0.5)
    if plant == "pint_for_pmid":
        return pint(dp, ptop)[:-1]
    out = np.empty_like(dp)
    out[0] = dp.dtype.type(ptop) + dp[0] * half
    for k in range(1, dp.shape[0]):
        out[k] = (out[k - 1] + dp[k] * half) if plant == "half_dropped" else (out[k - 1] + dp[k - 1] * half) + dp[k] * half
    return out


def phi(tv, dp, phis, rgas, p=None, ptop=None, plant=None):
    dp, tv, phis = np.asarray(dp), np.asarray(tv), np.asarray(phis)
    ty = dp.dtype.type
    if p is None:
        p = pmid(dp, ptop, plant)
    n = dp.shape[0]
    hkk = (dp * ty(0.5)) / p
    hkl = hkk if plant == "hkk_for_hkl" else ty(2.0) * hkk
    t = ty(rgas) * tv
    a, b = t * hkl, t * hkk
    phii = np.empty_like(dp)
    out = np.empty_like(dp)
    phii[n - 1] = a[n - 1]
    out[n - 1] = phis + b[n - 1]
    for k in range(n - 2, -1, -1):
        if k > 0 or plant == "phii_shifted":
            phii[k] = phii[k + 1] + a[k]
        out[k] = (phis + phii[k if plant == "phii_shifted" else k + 1]) + b[k]
    return out


def omega(vgrad_p, divdp, p=None, dp=None, ptop=None, plant=None):
    vgrad_p, divdp = np.asarray(vgrad_p), np.asarray(divdp)
    if p is None:
        p = pmid(np.asarray(dp), ptop, plant)
    p = np.asarray(p)
    ty = p.dtype.type
    n = p.shape[0]
    ckk = ty(0.5) / p
    ckl = ty(2.0) * ckk
    q, c = vgrad_p / p, ckk * divdp
    out = np.empty_like(p)
    if plant == "s_early":
        s = divdp[0].copy()
        out[0] = (q[0] - ckl[0] * s) - c[0]
    else:
        out[0] = q[0] - c[0]
        s = divdp[0].copy()
    for k in range(1, n):
        if plant == "s_early":
            s = s + divdp[k]
        out[k] = (q[k] - ckl[k] * s) - c[k]
        if plant != "s_early" and k < n - 1:
            s = s + divdp[k]
    return out


def run(op, ty, ptop, rgas, dp=None, p=None, a=None, b=None, plant=None):
    """one op on the views of tse_column_view (dp, p, a, b), evaluated in the type ty; plant: one of PLANTS, a wrong version"""
    cv = lambda x: None if x is None else np.asarray(x).astype(ty)
    dp, p, a, b = cv(dp), cv(p), cv(a), cv(b)
    if plant == "reversed":
        rv = lambda x: None if x is None else x[::-1]
        got = run(op, ty, ptop, rgas, rv(dp), rv(p), rv(a), b if op == "phi" else rv(b))
        return got[::-1]
    if op == "pint":
        return pint(dp, ptop)
    if op == "pmid":
        return pmid(dp, ptop, plant)
    if op == "phi":
        return phi(a, dp, b, rgas, p, ptop, plant)
    if op == "omega":
        return omega(a, b, p, dp, ptop, plant)
    raise ValueError(op)


def model(op, ptop, rgas, **views):
    return run(op, np.float64, ptop, rgas, **views)


def referee(op, ptop, rgas, **views):
    return run(op, np.longdouble, ptop, rgas, **views)


def _level_counts(n, shape, ty):
    return np.arange(n, dtype=ty).reshape((n,) + (1,) * (len(shape) - 1))


def bound(op, ptop, rgas, dp=None, p=None, a=None, b=None):
    """the pointwise bounds of the docstring, from the referee's magnitudes; the shape of the op's result, longdouble"""
    ld = np.longdouble
    cv = lambda x: None if x is None else np.asarray(x).astype(ld)
    dp, p, a, b = cv(dp), cv(p), cv(a), cv(b)
    u = ld(U)
    if op == "pint":
        pi = pint(dp, ptop)
        return (_level_counts(pi.shape[0], pi.shape, ld) + 1) * u * pi
    formed = p is None
    if formed:
        p = pmid(dp, ptop)
    n = p.shape[0]
    k = _level_counts(n, p.shape, ld)
    cp = 2 * k + 1 if formed else 0 * k
    if op == "pmid":
        return (cp + 1) * u * p
    rsum = lambda x: np.cumsum(x[::-1], axis=0)[::-1]          # x[j] + ... + x[n-1]
    zero = np.zeros_like(p[:1])
    if op == "phi":
        hkk = (dp * ld(0.5)) / p
        t = ld(rgas) * a
        ta, tb = np.abs(t * (2 * hkk)), np.abs(t * hkk)
        aphis = np.abs(b) + 0 * p                               # |phis| on every level
        A = np.concatenate([rsum(ta), zero])                    # A[j], A[n] = 0
        terms = np.concatenate([rsum((cp + 4) * ta), zero])[1:] + (cp + 4) * tb       # sum_{j>k} (cp[j]+4)|a[j]| + (cp[k]+4)|b[k]|
        # sum_{j=k+1}^{n-2} A[j]: the additions that form phii[k+1]
        Ain = A[:n].copy(); Ain[n - 1] = 0                      # A[n-1] is phii[n-1] itself: no addition
        adds = np.concatenate([rsum(Ain), zero])[1:]
        nxt = A[1:]                                             # A[k+1]
        inner = np.where(k < n - 1, aphis + nxt, 0)
        return u * (terms + adds + inner + aphis + nxt + tb)
    if op == "omega":
        q, ckl, c = np.abs(a / p), 2 * (ld(0.5) / p), np.abs((ld(0.5) / p) * b)
        D = np.concatenate([zero, np.cumsum(np.abs(b), axis=0)])[:n]      # D[k] = |divdp[0]| + ... + |divdp[k-1]|, D[0] = 0
        D2 = D.copy(); D2[:2] = 0                                          # D[2] + ... + D[k]
        serr = np.cumsum(D2, axis=0)
        lower = k > 0
        return u * ((cp + 2) * q + np.where(lower, (cp + 3) * ckl * D + ckl * serr, 0) + (cp + 3) * c + np.where(lower, q + ckl * D, 0)
                    + q + np.where(lower, ckl * D, 0) + c)
    raise ValueError(op)


def family(n, ncol, seed=0, ptop=219.4, ps=1.0e5):
    """the input family of the bounds: dp within 10 % of a stretched grid from ptop to about ps, T_v in 180..320, signed phis, divdp and
    vgrad_p.  dict of fp64 arrays [n][ncol] (phis [ncol]) and ptop, rgas"""
    rng = np.random.default_rng(seed)
    eta = np.linspace(0.0, 1.0, n + 1) ** 2.5                    # thin layers at the top
    dp0 = np.diff(eta) * (ps - ptop)
    dp = dp0[:, None] * (0.9 + 0.2 * rng.random((n, ncol)))
    tv = 180.0 + 140.0 * rng.random((n, ncol))
    phis = 3.0e4 * (rng.random(ncol) - 0.3)
    divdp = dp * 1.0e-5 * (2.0 * rng.random((n, ncol)) - 1.0)
    vgrad = 1.0e-2 * (ptop + np.cumsum(dp, axis=0)) * 1.0e-3 * (2.0 * rng.random((n, ncol)) - 1.0)
    return dict(dp=dp, tv=tv, phis=phis, divdp=divdp, vgrad_p=vgrad, ptop=ptop, rgas=287.04)


def views_of(op, f, p=None):
    """the keyword views of run / model / bound for one op on a family (or on any dict with its keys); p: a given pressure or None"""
    if op in ("pint", "pmid"):
        return dict(dp=f["dp"])
    if op == "phi":
        return dict(dp=f["dp"], p=p, a=f["tv"], b=f["phis"])
    return dict(dp=None if p is not None else f["dp"], p=p, a=f["vgrad_p"], b=f["divdp"])


def to_cols(x):
    """[E][1][nk][4][4] -> [nk][E][4][4] (a surface field [E][1][1][4][4] -> [E][4][4])"""
    x = np.asarray(x)[:, 0]
    return x[:, 0] if x.shape[1] == 1 else np.moveaxis(x, 1, 0)


def from_cols(y):
    """[nk][E][4][4] -> [E][1][nk][4][4]"""
    return np.ascontiguousarray(np.moveaxis(np.asarray(y), 0, 1))[:, None]
