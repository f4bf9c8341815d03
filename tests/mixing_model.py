"""The element partials of the mixing and filament diagnostics (tse_mix_partials; Lauritzen and Thuburn 2012), restated in numpy IN THE
DEVICE'S ORDER, a longdouble referee for the distance d, and the point families the mixing tests use.

Definitions (include/transport_se_hip.h, csrc/tse_kernels.h).  psi(x) = c0 + c2*(x*x), c2 < 0, is the curve the two tracers start on, chi in
[xmin, xmax].  Derived once in fp64, each operation rounded once (constants()):
    yhi = psi(xmin), ylo = psi(xmax), Rx = xmax - xmin, Ry = yhi - ylo, sl = (ylo - yhi)/Rx, kk = (Ry*Ry)/(Rx*Rx), i2 = 1/(2*c2*c2)
Classes of a point (chi, xi): A  xmin <= chi <= xmax and yhi + (chi - xmin)*sl <= xi <= psi(chi);  B  not A, chi in [xmin, xmax] and
xi in [ylo, yhi];  C  the rest.  d = sqrt(min over x in [xmin, xmax] of g(x)), g(x) = ((chi - x)/Rx)^2 + ((xi - psi(x))/Ry)^2.

distance() is the device's algorithm operation for operation (+ - * / sqrt, comparisons, selects; numpy does not contract):
    P = (kk - (2*c2)*(xi - c0))*i2, Qc = (-(chi*kk))*i2, h(x) = (x*x + P)*x + Qc   (the stationary points of g are the roots of h)
    s = sqrt(max((-P)/3, 0)); break points b0 = xmin, b1 = clamp(-s), b2 = clamp(s), b3 = xmax
    best = min(g(b0), g(b3)); on each [b_i, b_i+1]: NB = 60 bisection steps (right when (h(mid) < 0) == (h(hi) >= h(lo))), and
    best = min(best, g(final mid)) where h changes sign over the interval;  d = sqrt(best)

An element's share out[32] adds its terms in THE ORDER of k_norm_partials (norm_model._point_sums, _element_sum): lane (point, level group)
ascending over its levels, column = ((s0 + s1) + s2) + s3, owned points ascending.  A term outside its class or below its threshold enters as
+ 0.0, which changes no bit of a sum of non-negative numbers.

The referee (referee_distance) minimises the same g -- with the same fp64 constants, which are the definition -- in longdouble: a dense scan of
[xmin, xmax], then a 120-step golden section around each of the scan's three best local minima.  Its own error: the scan cannot miss a
basin wider than its spacing, and g has at most two; inside a basin the golden section ends with a bracket of 0.618^120 of the spacing, so the
error of d is that of longdouble arithmetic, some 1e-19."""
import numpy as np

import norm_model as nm

NB = 60
NTAU = 24
NOUT = 32


def constants(xmin, xmax, c0, c2):
    xmin, xmax, c0, c2 = (np.float64(v) for v in (xmin, xmax, c0, c2))
    yhi = c0 + c2 * (xmin * xmin)
    ylo = c0 + c2 * (xmax * xmax)
    Rx = xmax - xmin
    Ry = yhi - ylo
    return dict(xmin=xmin, xmax=xmax, c0=c0, c2=c2, yhi=yhi, ylo=ylo, Rx=Rx, Ry=Ry, sl=(ylo - yhi) / Rx, kk=(Ry * Ry) / (Rx * Rx),
                i2=np.float64(1.0) / ((np.float64(2.0) * c2) * c2))


def _g(m, x, chi, xi):
    a = (chi - x) / m["Rx"]
    b = (xi - (m["c0"] + m["c2"] * (x * x))) / m["Ry"]
    return a * a + b * b


def cubic(m, chi, xi):
    """(P, Qc) of h(x) = (x*x + P)*x + Qc"""
    return (m["kk"] - (2.0 * m["c2"]) * (xi - m["c0"])) * m["i2"], (-(chi * m["kk"])) * m["i2"]


def _intervals(m, P):
    s = np.sqrt(np.maximum((-P) / 3.0, 0.0))
    lo, hi = m["xmin"], m["xmax"]
    return [np.full_like(P, lo), np.minimum(np.maximum(-s, lo), hi), np.minimum(np.maximum(s, lo), hi), np.full_like(P, hi)]


def sign_changes(m, chi, xi):
    """how many of the three intervals h changes sign over (0 to 3): which path of distance() a point takes"""
    chi = np.asarray(chi, np.float64); xi = np.asarray(xi, np.float64)
    P, Qc = cubic(m, chi, xi)
    b = _intervals(m, P)
    hb = [(x * x + P) * x + Qc for x in b]
    return sum((((hb[i] <= 0) & (hb[i + 1] >= 0)) | ((hb[i] >= 0) & (hb[i + 1] <= 0))).astype(int) for i in range(3))


def distance(m, chi, xi, plant=None):
    """d of every point, in the device's operations.  plant "ends": the end-point candidates left out (best starts at +inf)"""
    chi = np.asarray(chi, np.float64); xi = np.asarray(xi, np.float64)
    P, Qc = cubic(m, chi, xi)
    b = _intervals(m, P)
    best = np.minimum(_g(m, b[0], chi, xi), _g(m, b[3], chi, xi))
    if plant == "ends":
        best = np.full_like(chi, np.inf)
    for i in range(3):
        lo, hi = b[i], b[i + 1]
        hl = (lo * lo + P) * lo + Qc
        hh = (hi * hi + P) * hi + Qc
        has = ((hl <= 0) & (hh >= 0)) | ((hl >= 0) & (hh <= 0))
        up = hh >= hl
        for _ in range(NB):
            mid = 0.5 * (lo + hi)
            right = (((mid * mid + P) * mid + Qc) < 0) == up
            lo = np.where(right, mid, lo)
            hi = np.where(right, hi, mid)
        best = np.where(has, np.minimum(best, _g(m, 0.5 * (lo + hi), chi, xi)), best)
    return np.sqrt(best)


def classes(m, chi, xi, plant=None):
    """(A, B, C) as boolean arrays.  plants: "slope" = the chord's slope with the wrong sign, "swap" = B and C exchanged"""
    inx = (m["xmin"] <= chi) & (chi <= m["xmax"])
    sl = -m["sl"] if plant == "slope" else m["sl"]
    chord = m["yhi"] + (chi - m["xmin"]) * sl
    curve = m["c0"] + m["c2"] * (chi * chi)
    A = inx & (chord <= xi) & (xi <= curve)
    B = ~A & inx & (m["ylo"] <= xi) & (xi <= m["yhi"])
    C = ~A & ~B
    return (A, C, B) if plant == "swap" else (A, B, C)


def element_partials(chi, xi, owner, colw, dh, xmin, xmax, c0, c2, tau, plant=None):
    """out[nelem][32] of tse_mix_partials in the device's order.  chi, xi [nelem][nlev][4][4]; owner, colw [nelem][4][4]; dh[nlev]; tau: at
    most 24 thresholds.  plant: None, "slope", "ends" or "swap" -- one deliberate error, for the tests that show it caught."""
    assert plant in (None, "slope", "ends", "swap"), plant
    E, nlev = chi.shape[:2]
    tau = np.asarray(tau, np.float64).reshape(-1)
    assert tau.size <= NTAU
    m = constants(xmin, xmax, c0, c2)
    own = owner.reshape(E, 16)
    x = chi.reshape(E, nlev, 16); y = xi.reshape(E, nlev, 16)
    dV = colw.reshape(E, 1, 16) * np.asarray(dh).reshape(1, nlev, 1)
    d = distance(m, x, y, plant)
    A, B, C = classes(m, x, y, plant)
    with np.errstate(invalid="ignore"):      # (the "ends" plant leaves d = inf where nothing else is a candidate; colw = 0 at unowned points)
        ddV = d * dV
    t = [np.where(A, ddV, 0.0), np.where(B, ddV, 0.0), np.where(C, ddV, 0.0), dV + np.zeros_like(x),
         A.astype(np.float64), B.astype(np.float64), C.astype(np.float64)]
    t += [np.where(x >= tj, dV, 0.0) for tj in tau]
    out = np.zeros((E, NOUT))
    S = nm._element_sum(nm._point_sums(np.stack(t)), own)      # [len(t)][E]
    out[:, :7] = S[:7].T
    out[:, 8:8 + tau.size] = S[7:].T
    mask = np.broadcast_to((own != 0)[:, None, :], (E, nlev, 16))
    out[:, 7] = np.where(mask, d, 0.0).max(axis=(1, 2))
    return out


# ---- the longdouble referee ----
def referee_distance(m, chi, xi, nscan=4001, chunk=400):
    """d of every point in longdouble: dense scan + golden section (module docstring); chi, xi 1-d"""
    L = np.longdouble
    chi = np.asarray(chi, np.float64).ravel().astype(L); xi = np.asarray(xi, np.float64).ravel().astype(L)
    c0, c2, Rx, Ry = (L(m[k]) for k in ("c0", "c2", "Rx", "Ry"))
    xs = L(m["xmin"]) + (L(m["xmax"]) - L(m["xmin"])) * (np.arange(nscan).astype(L) / L(nscan - 1))
    xs[0], xs[-1] = L(m["xmin"]), L(m["xmax"])

    def g(x, X, Y):
        a = (X - x) / Rx; b = (Y - (c0 + c2 * (x * x))) / Ry
        return a * a + b * b
    gr = (np.sqrt(L(5)) - 1) / 2
    out = np.empty(chi.size, L)
    for s0 in range(0, chi.size, chunk):
        X = chi[s0:s0 + chunk, None]; Y = xi[s0:s0 + chunk, None]
        G = g(xs[None, :], X, Y)
        pad = np.pad(G, ((0, 0), (1, 1)), constant_values=np.inf)
        localmin = (G <= pad[:, :-2]) & (G <= pad[:, 2:])
        order = np.argsort(np.where(localmin, G, np.inf), axis=1)[:, :3]       # the three best local minima of the scan
        lo = xs[np.maximum(order - 1, 0)]; hi = xs[np.minimum(order + 1, nscan - 1)]
        for _ in range(120):
            c = hi - gr * (hi - lo); e = lo + gr * (hi - lo)
            left = g(c, X, Y) < g(e, X, Y)
            hi = np.where(left, e, hi); lo = np.where(left, lo, c)
        best = np.minimum(g(0.5 * (lo + hi), X, Y).min(axis=1), G.min(axis=1))
        out[s0:s0 + chunk] = np.sqrt(best)
    return out


# ---- the point families of the tests ----
def families(m, tau, rng, n=200):
    """{name: (chi, xi)}: the families the mixing tests must cover, n points each where a family is a continuum"""
    xmin, xmax, yhi, ylo, Rx, Ry = (float(m[k]) for k in ("xmin", "xmax", "yhi", "ylo", "Rx", "Ry"))
    c0, c2, sl = float(m["c0"]), float(m["c2"]), m["sl"]

    def psi(x):
        return m["c0"] + m["c2"] * (x * x)
    fam = {}
    x = rng.uniform(xmin, xmax, n)
    fam["on the curve"] = (x, psi(x))
    fam["near the curve"] = (x, psi(x) + rng.normal(0.0, 1e-9, n))
    w = rng.uniform(0.02, 0.98, n)
    chord = m["yhi"] + (x - m["xmin"]) * sl
    fam["inside the hull"] = (x, chord + w * (psi(x) - chord))
    fam["on the chord"] = (x, chord)
    y = rng.uniform(ylo, yhi, n)
    fam["on the rectangle's edges"] = (np.concatenate([np.full(n, xmin), np.full(n, xmax), x, x]),
                                       np.concatenate([y, y, np.full(n, ylo), np.full(n, yhi)]))
    fam["on the rectangle's corners"] = (np.array([xmin, xmin, xmax, xmax]), np.array([ylo, yhi, ylo, yhi]))
    far = rng.uniform(0.0, 0.3, n)
    fam["outside, left"] = (xmin - far * Rx - 1e-12, rng.uniform(ylo - 0.2 * Ry, yhi + 0.2 * Ry, n))
    fam["outside, right"] = (xmax + far * Rx + 1e-12, rng.uniform(ylo - 0.2 * Ry, yhi + 0.2 * Ry, n))
    fam["outside, below"] = (x, ylo - far * Ry - 1e-12)
    fam["outside, above"] = (x, np.maximum(psi(x), yhi) + far * Ry + 1e-12)
    # the paths of the distance: P >= 0 (h monotone), P < 0 with one and with three sign changes over the three intervals
    X = rng.uniform(xmin - 0.2 * Rx, xmax + 0.2 * Rx, 40 * n); Y = rng.uniform(ylo - 0.3 * Ry, max(yhi, c0) + 0.3 * Ry, 40 * n)
    P = cubic(m, X, Y)[0]
    sc = sign_changes(m, X, Y)
    fam["P >= 0"] = (X[P >= 0][:n], Y[P >= 0][:n])
    for k, name in ((1, "one"), (2, "two"), (3, "three")):
        pick = (P < 0) & (sc == k)
        if pick.any():
            fam["P < 0, %s sign change(s)" % name] = (X[pick][:n], Y[pick][:n])
    tau = np.asarray(tau, np.float64)
    fam["chi equal to a threshold"] = (np.repeat(tau, 3), np.tile(np.array([ylo - 0.1 * Ry, 0.5 * (ylo + yhi), yhi + 0.1 * Ry]), tau.size))
    return fam


def synthetic_fields(m, tau, nelem, nlev, rng):
    """(chi, xi) [nelem][nlev][4][4]: every family's points, shuffled and repeated until the fields are full, so that each family meets
    owned and unowned points, every level group and many layer depths"""
    fam = families(m, tau, rng)
    X = np.concatenate([np.asarray(v[0], np.float64).ravel() for v in fam.values()])
    Y = np.concatenate([np.asarray(v[1], np.float64).ravel() for v in fam.values()])
    n = nelem * nlev * 16
    idx = np.concatenate([rng.permutation(X.size) for _ in range(n // X.size + 1)])[:n]
    return X[idx].reshape(nelem, nlev, 4, 4), Y[idx].reshape(nelem, nlev, 4, 4)


# ---- the summation bound between the two routes ----
def summation_bounds(owner, nlev):
    """dict(l, l_f): bounds on |x(mixing_from_partials) - x(mixing_diagnostics)| / x(mixing_diagnostics).  Both routes add THE SAME
    non-negative fp64 terms; with norm_model's notation, e_d = gamma(n_max - 1) + u for the device's order followed by the exact sum of the
    element shares rounded once, e_n = gamma(M_NP) for a numpy sum.  A quotient of two such sums (l_r, l_u, l_o = S_j / S_3) carries one
    division per route: (1+e_d)(1+e_n)(1+u) / ((1-e_d)(1-e_n)(1-u)) - 1, norm_model.forward_bounds' L1 without the moving mean.
    l_f = 100 * S(t) / S(t0) carries one more rounding per route, the multiplication by 100."""
    import math
    E = owner.shape[0]
    nmax = int(owner.reshape(E, 16).sum(1).max()) * nlev
    N = nlev * int(owner.sum())
    gm = nm.gamma(nmax - 1)
    e_d = gm + nm.U + gm * nm.U
    e_n = nm.gamma(nm.numpy_depth(nlev, N))
    lp = math.log1p
    both = lp(e_d) + lp(e_n) - lp(-e_d) - lp(-e_n)
    return dict(l=math.expm1(both + lp(nm.U) - lp(-nm.U)), l_f=math.expm1(both + 2 * (lp(nm.U) - lp(-nm.U))))
