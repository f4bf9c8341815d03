"""The unlimited tracer step (limiter_option = 0) in numpy longdouble (64-bit mantissa on x86-64), with a rigorous forward-error bound
per point that holds for every fp64 evaluation of the same operation.  Plain numpy; no HIP import.

What is modelled: euler_step (prim_advection_mod.F90:667-970) without the limiter line, the divdp formation and the time average of
Prim_Advec_Tracers_remap_rk2 (:579-662) -- what tests/unlimited_model.py does in fp64, here vectorised over elements, tracers and levels.
The DSS is the oracle's (edgeVpack/edgeVunpack over Oracle.nbr_elem / nbr_dir / nbr_rev: the checker's element order; Dss.fp64 is its
serial sum, bit for bit Oracle.dss).  Cube corners are nodes of 3 elements, other element corners of 4.

Triples.  Every quantity is carried as T(v, A, m): the longdouble value v, a magnitude A >= |v| per point, and a rounding count m (one
integer per quantity).  Invariant: ANY fp64 evaluation of the same expression -- any association of its sums and products, with or without
FMA contraction -- gives fl with |fl - v_exact| <= gamma_m(2^-53) * A (Higham, Accuracy and Stability of Numerical Algorithms, 3.1-3.4):
  exact fp64 input             m = 0                    A = |x|
  product a*b                  m = m_a + m_b + 1        A = A_a * A_b          (times an exact power of two: m, A unchanged but scaled)
  n-term sum, any association  m = max m_i + (n - 1)    A = sum A_i            (an FMA counts as its unfused product and sum)
  reciprocal 1/y               m = m_y + 1              A = kappa_y / |y|,  kappa_y = A_y / |y|;  asserted gamma_{m_y} * kappa_y <= 2^-40
                               (a division x/y counts as x * (1/y): the device multiplies by reciprocals, the reference divides)
The divisors are dp of a stage (dp - rhs*dt*divdp_proj), and the constants spheremp and 3.  rhs*dt (rhs = 0, 1, 2) is exact.
The fp64 inputs of both sides are the same numbers: the geometry arrays, Dvv, vn0, dp, the tracers, RREARTH = 1/6.376e6 (correctly
rounded by the compiler and by Python alike) and dp0(k) = (hyai(k+1)-hyai(k))*ps0 + (hybi(k+1)-hybi(k))*ps0, which tse_init forms on
the host in this very expression and operand order (tse_api.hip, no contraction on the host) and uploads -- so dp0 is an exact input.

Counts that follow (m_in of the operand field; the 8-term sum of a divergence and of a weak divergence is counted as one sum):
  divergence_sphere(v)          m_v + 13    (Dinv*v, +, *metdet: 3; *Dvv, 8-term sum: 8; *(rmetdet*RREARTH): 2)
  laplace_sphere_wk(s)          m_s + 19    (Dvv*, 4-term sum, *RREARTH: 5; Dinv^T, Dinv: 4; *spheremp, *Dvv, 8-term sum, *RREARTH: 10)
  DSS(f)                        m_f + 3     (at most 4 contributions at a node)
  euler_step, inputs Qdp (m_q), divdp_proj (m_d), extra variable (m_x):
    dp_stage = dp - (rhs*dt)*divdp_proj          m_d + 2;   1/dp_stage: m_d + 3;   Vstar = vn0 * (1/dp_stage): m_d + 4
    advection  Qdp - dt*div(Vstar*Qdp)           m_q + m_d + 19
    biharmonic (rhs 2) Q = Qdp/dp_stage: m_q + m_d + 4; lap: +19; DSS: +3; *rspheremp: +1; lap: +19;
               * (-3*dt*nu_q*dp0) (3) * (1/spheremp) (1) and two products: +6        m_q + m_d + 52
    Qtens: the 2- or 3-term sum; Qdp(np1) = rspheremp * DSS(spheremp * Qtens): +1 +1 +3 +1
    extra variable rspheremp * DSS(spheremp * x)  m_x + 5
  From exact inputs (the per-stage route: each stage from the device's own fp64 output of the stage before):
    divdp = divdp_proj 13; stage 1 (rhs 0) 25; stage 2 (rhs 1) 25; stage 3 (rhs 2) 59; extra variable 5; qdp_time_avg(3) 3 (+1 +2)
  The whole step from its fp64 inputs (DSS on read or one DSS pass per stage: the same operation):
    divdp 13; divdp_proj 18; eta_dot_dpdn, omega_p 5; stage 1 38; stage 2 81; stage 3 158; Qdp(np1) after the time average 161.
  Element mass sum_k sum_p spheremp*Qdp (points, then levels): 1 + 15 + 71 = 87.

The longdouble evaluation carries its own error gamma_m(2^-64) * A, so the tests assert |got - v| <= (gamma_m(2^-53) + gamma_m(2^-64)) *
A * (1 + 2^-40): the (1 + 2^-40) absorbs the second-order terms of the reciprocals and the rounding of A itself.

Range.  Every nonzero magnitude A of every intermediate is asserted to lie within [2^-700, 2^700]: 322 binades clear of the subnormal
range (where the model above does not hold) and of overflow, for the test fields and their 2^+-200 scalings.
"""
import numpy as np

LD = np.longdouble
NLEV = 72
PS0 = 1.0e5
RREARTH = 1.0 / 6.376e6
A_LO, A_HI = 2.0 ** -700, 2.0 ** 700
KAPPA_SLACK = 2.0 ** -40


def has_extended_precision():
    return np.finfo(LD).nmant >= 63


def gamma(n, u=2.0 ** -53):
    return n * u / (1.0 - n * u)


def bound(m, A):
    """the asserted bound on |fp64 result - v| for a quantity of rounding count m and magnitude A"""
    return (gamma(m) + gamma(m, 2.0 ** -64)) * np.asarray(A, dtype=np.float64) * (1.0 + 2.0 ** -40)


def ratio(got, t):
    """max over points of |got - v| / bound (0/0 counts as 0) and the per-point ratio array"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - t.v).astype(np.float64)
    b = bound(t.m, t.A)
    r = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1e-300))
    return float(r.max()) if r.size else 0.0, r


def _check_range(A):
    a = np.asarray(A)
    nz = a[a != 0]
    if nz.size:
        lo, hi = nz.min(), nz.max()
        assert A_LO <= lo and hi <= A_HI, ("magnitude out of range", float(lo), float(hi))


class T:
    """(v, A, m): longdouble value, magnitude >= |v| per point, rounding count"""
    __slots__ = ("v", "A", "m")

    def __init__(self, v, A, m):
        self.v, self.A, self.m = v, A, int(m)
        _check_range(A)

    def __getitem__(self, ix):
        return T(self.v[ix], self.A[ix], self.m)


def exact(x):
    x = np.asarray(x, dtype=np.float64)
    return T(x.astype(LD), np.abs(x).astype(LD), 0)


def neg(a):
    return T(-a.v, a.A, a.m)


def pow2(a, s):
    """a * s, s an exact power of two (no rounding)"""
    assert np.frexp(s)[0] in (0.5, -0.5), s
    return T(a.v * LD(s), a.A * LD(abs(s)), a.m)


def mul(a, b):
    return T(a.v * b.v, a.A * b.A, a.m + b.m + 1)


def mul_tight(a, b):
    """a*b where |v| may lie far below A (a difference that cancelled, and its powers): the same count as mul, and the magnitude
    taken from the absolute errors E = gamma_m * A of the factors instead of A_a * A_b:
      |fl(a~ b~) - a b| <= |a| E_b + |b| E_a + E_a E_b + u (|a| + E_a)(|b| + E_b) =: err,   A = max(|v|, err / gamma_m), m = m_a + m_b + 1.
    err <= gamma_m * A_a * A_b, so this is never looser than mul; the longdouble evaluation's own error obeys the same formula with
    u = 2^-64, which bound() adds as gamma_m(2^-64) * A."""
    m = a.m + b.m + 1
    u = 2.0 ** -53
    av, bv = np.abs(a.v), np.abs(b.v)
    Ea, Eb = LD(gamma(a.m)) * a.A, LD(gamma(b.m)) * b.A
    err = av * Eb + bv * Ea + Ea * Eb + LD(u) * (av + Ea) * (bv + Eb)
    return T(a.v * b.v, np.maximum(av * bv, err / LD(gamma(m))), m)


def part(a):
    """a quantity as one term of a sum: (v, A, count of the term, number of terms)"""
    return a.v, a.A, a.m, 1


def sum_parts(*parts):
    """one sum over all terms of the parts, in any association"""
    n = sum(p[3] for p in parts)
    return T(sum(p[0] for p in parts), sum(p[1] for p in parts), max(p[2] for p in parts) + n - 1)


def add(*ts):
    return sum_parts(*[part(t) for t in ts])


# ---- continuous, piecewise operations (the PPM remap, tests/remap_ld.py): no decision is taken on any of them ----
def absval(a):
    """|a|: exact on the value, the error is that of a"""
    return T(np.abs(a.v), a.A, a.m)


def minimum(*ts):
    """min(a, b, ...).  min is 1-Lipschitz in the max norm, so |min(a,b)_fl - min(a,b)| <= max(err_a, err_b) whichever operand either
    side picks; (A, m) = (max A_i, max m_i) gives gamma_m * A >= gamma_{m_i} * A_i for every i, and A >= |v|."""
    v, A = ts[0].v, ts[0].A
    for t in ts[1:]:
        v, A = np.minimum(v, t.v), np.maximum(A, t.A)
    return T(v, A, max(t.m for t in ts))


def copysign_le(mag, da):
    """copysign(mag, da) for a mag that is min(|da|, ...) on BOTH sides, so 0 <= mag <= |da| in exact arithmetic and in every fp64
    evaluation.  Continuous through da = 0.  Same sign of da on both sides: the error is err_mag.  Opposite signs (or one side 0):
    |r_fl - r| = mag_fl + mag <= |da_fl| + |da| = |da_fl - da| = err_da, because da_fl and da then lie on opposite sides of 0.
    So |r_fl - r| <= max(err_mag, err_da): (A, m) = (max(A_mag, A_da), max(m_mag, m_da))."""
    return T(np.where(np.signbit(da.v), -mag.v, mag.v), np.maximum(mag.A, da.A), max(mag.m, da.m))


def select(cond, a, b):
    """where(cond, a, b) of a decision taken elsewhere (the caller answers for the decision): value and magnitude of the chosen operand,
    the larger count"""
    return T(np.where(cond, a.v, b.v), np.where(cond, a.A, b.A), max(a.m, b.m))


def cancel(t, where):
    """t with T(0, 0, .) at the points `where`: a difference of a quantity and a copy of its own bits (a ghost cell and the cell it
    mirrors, the two interface values of a flattened cell) is exactly 0 on both sides"""
    return T(np.where(where, LD(0), t.v), np.where(where, LD(0), t.A), t.m)


def contract(spec, C, t):
    """the products C * t of an exact coefficient matrix, summed over one index of length n (a part of a sum)"""
    C = np.asarray(C, dtype=np.float64)
    n = C.shape[-1]
    return np.einsum(spec, C.astype(LD), t.v), np.einsum(spec, np.abs(C).astype(LD), t.A), t.m + 1, n


def recip(y):
    ay = np.abs(y.v)
    kappa = y.A / ay
    worst = float((gamma(y.m) * kappa).max())
    assert worst <= KAPPA_SLACK, ("divisor too ill-conditioned for the bound", y.m, worst)
    return T(1 / y.v, kappa / ay, y.m + 1)


# ---- geometry (fields are [e][...][4 j][4 i]; element arrays broadcast over the middle axes) ----
class Geo:
    def __init__(self, o):
        Di = np.asarray(o.Dinv)
        self.D = [[np.ascontiguousarray(Di[..., b, a]) for b in range(2)] for a in range(2)]   # D[a][b] = Dinv(a,b)
        self.Dvv = np.asarray(o.Dvv).copy()                                                     # Dvv[l][i] = Dvv(i,l)
        self.metdet, self.rmetdet = np.asarray(o.metdet).copy(), np.asarray(o.rmetdet).copy()
        self.spheremp, self.rspheremp = np.asarray(o.spheremp).copy(), np.asarray(o.rspheremp).copy()
        self.nelem = o.nelem
        self.dss = Dss(o)

    def g(self, x, nd):
        """an element array [e][4][4] as an exact input broadcast to a field of nd axes"""
        return exact(np.asarray(x).reshape((x.shape[0],) + (1,) * (nd - 3) + (4, 4)))


def divergence_sphere(geo, v1, v2):
    """derivative_mod.F90:2364-2414 (oracle divergence_sphere_e) of the vector field (v1, v2)"""
    nd = v1.v.ndim
    D = [[geo.g(geo.D[a][b], nd) for b in range(2)] for a in range(2)]
    met = geo.g(geo.metdet, nd)
    gv1 = mul(met, add(mul(D[0][0], v1), mul(D[0][1], v2)))
    gv2 = mul(met, add(mul(D[1][0], v1), mul(D[1][1], v2)))
    s = sum_parts(contract("li,e...ji->e...jl", geo.Dvv, gv1), contract("li,e...ij->e...lj", geo.Dvv, gv2))
    return mul(s, mul(geo.g(geo.rmetdet, nd), exact(RREARTH)))


def laplace_sphere_wk(geo, s):
    """derivative_mod.F90:2418-2460 (oracle laplace_sphere_wk_e): divergence_sphere_wk(gradient_sphere(s))"""
    nd = s.v.ndim
    D = [[geo.g(geo.D[a][b], nd) for b in range(2)] for a in range(2)]
    rr = exact(RREARTH)
    v1 = mul(sum_parts(contract("li,e...ji->e...jl", geo.Dvv, s)), rr)
    v2 = mul(sum_parts(contract("li,e...ij->e...lj", geo.Dvv, s)), rr)
    ds1 = add(mul(D[0][0], v1), mul(D[1][0], v2))
    ds2 = add(mul(D[0][1], v1), mul(D[1][1], v2))
    vt1 = add(mul(D[0][0], ds1), mul(D[0][1], ds2))
    vt2 = add(mul(D[1][0], ds1), mul(D[1][1], ds2))
    sph = geo.g(geo.spheremp, nd)
    t = sum_parts(contract("jm,e...nj->e...nm", geo.Dvv, mul(sph, vt1)), contract("jn,e...jm->e...nm", geo.Dvv, mul(sph, vt2)))
    return neg(mul(t, rr))


# ---- DSS ----
_EDGE_ORDER, _CORNER_ORDER = (2, 1, 3, 0), (4, 5, 7, 6)      # unpack order S, E, N, W, then SW, SE, NE, NW (edge_mod.F90:685-734)
_CORNER_POINT = (0, 3, 12, 15)                              # SW SE NW NE


def _edge_point(d, k):
    return (k * 4, k * 4 + 3, k, 12 + k)[d]


class Dss:
    """edgeVpack / edgeVunpack over the oracle's connectivity: contribution c of point p of element e is point src_p of element src_e
    (self first, then the unpack order; absent ones point at an all-zero element nelem)"""
    NC = 4

    def __init__(self, o):
        n = o.nelem
        ne_, nd_, nr_ = np.asarray(o.nbr_elem), np.asarray(o.nbr_dir), np.asarray(o.nbr_rev)
        lists = [[[(e, p)] for p in range(16)] for e in range(n)]
        for e in range(n):
            for d in _EDGE_ORDER:
                nb, nd, rev = int(ne_[e, d]), int(nd_[e, d]), int(nr_[e, d])
                assert nb >= 0
                for k in range(4):
                    lists[e][_edge_point(d, k)].append((nb, _edge_point(nd, 3 - k if rev else k)))
            for d in _CORNER_ORDER:
                nb = int(ne_[e, d])
                if nb >= 0:
                    lists[e][_CORNER_POINT[d - 4]].append((nb, _CORNER_POINT[int(nd_[e, d]) - 4]))
        self.src_e = np.full((n, 16, self.NC), n, dtype=np.int64)
        self.src_p = np.zeros((n, 16, self.NC), dtype=np.int64)
        self.count = np.zeros((n, 16), dtype=np.int64)
        for e in range(n):
            for p in range(16):
                c = lists[e][p]
                assert 1 <= len(c) <= self.NC
                self.count[e, p] = len(c)
                for i, (se, sp) in enumerate(c):
                    self.src_e[e, p, i], self.src_p[e, p, i] = se, sp
        self.nelem = n

    def _gather(self, f):
        """f[e][...][4][4] -> g[e][16][NC][X] (the contributions of every point; absent ones 0)"""
        n = self.nelem
        x = np.asarray(f).reshape(n, -1, 16)
        x = np.concatenate([x, np.zeros((1,) + x.shape[1:], dtype=x.dtype)])
        return x[self.src_e, :, self.src_p]

    def _back(self, g, shape):
        return np.moveaxis(g, 1, -1).reshape(shape)

    def ld(self, t):
        """the DSS of a triple: m + 3"""
        shp = t.v.shape
        return T(self._back(self._gather(t.v).sum(axis=2), shp), self._back(self._gather(t.A).sum(axis=2), shp), t.m + self.NC - 1)

    def fp64(self, f, drop=None):
        """the oracle's serial fp64 DSS (Oracle.dss bit for bit); drop = (e, p, c): leave out contribution c of point p of element e"""
        f = np.asarray(f, dtype=np.float64)
        g = self._gather(f)
        y = g[:, :, 0].copy()
        for c in range(1, self.NC):
            use = (self.count > c)[:, :, None]
            if drop is not None:
                use = use.copy()
                use[drop[0], drop[1]] &= c != drop[2]
            y = np.where(use, y + g[:, :, c], y)
        return self._back(y, f.shape)


# ---- the step ----
def dp0_levels(hyai, hybi, ps0=PS0):
    """dp0(k) in the expression and operand order of the oracle and of tse_init (fp64, no contraction)"""
    hyai, hybi = np.asarray(hyai, dtype=np.float64), np.asarray(hybi, dtype=np.float64)
    return (hyai[1:] - hyai[:-1]) * ps0 + (hybi[1:] - hybi[:-1]) * ps0


def compute_divdp(geo, vn0):
    """divdp = divdp_proj = divergence_sphere(vn0) (prim_advection_mod.F90:614-623); vn0[e][k][2][4][4]"""
    vn0 = np.asarray(vn0)
    return divergence_sphere(geo, exact(vn0[:, :, 0]), exact(vn0[:, :, 1]))


def _lev(t):
    """a level field [e][k][4][4] broadcast against tracers [e][q][k][4][4]"""
    return T(t.v[:, None], t.A[:, None], t.m)


def euler_step(geo, Qn0, dp, vn0, divdp_proj, var, dt, rhs_multiplier, nu_q, dp0):
    """one RK stage without the limiter.  Qn0: T [e][q][k][4][4]; divdp_proj, var: T [e][k][4][4] (var: this stage's extra variable);
    dp, vn0, dp0: fp64 arrays.  -> (Qdp(np1), DSS'd extra variable)"""
    assert rhs_multiplier in (0, 1, 2)
    nd = Qn0.v.ndim
    dpk = add(exact(dp), neg(mul(exact(float(rhs_multiplier) * dt), divdp_proj)))     # rhs*dt: exact
    rdp = recip(dpk)
    vn0 = np.asarray(vn0)
    vs1, vs2 = _lev(mul(exact(vn0[:, :, 0]), rdp)), _lev(mul(exact(vn0[:, :, 1]), rdp))
    div = divergence_sphere(geo, mul(vs1, Qn0), mul(vs2, Qn0))
    terms = [Qn0, neg(mul(exact(dt), div))]
    if rhs_multiplier == 2:
        lap = laplace_sphere_wk(geo, mul(Qn0, _lev(rdp)))
        lap = mul(geo.g(geo.rspheremp, nd), geo.dss.ld(lap))
        lap = laplace_sphere_wk(geo, lap)
        coef = mul(mul(mul(exact(-3.0), exact(dt)), exact(nu_q)), exact(np.asarray(dp0)[None, None, :, None, None]))
        terms.append(mul(mul(coef, lap), recip(geo.g(geo.spheremp, nd))))
    qt = add(*terms)
    out = mul(geo.g(geo.rspheremp, nd), geo.dss.ld(mul(geo.g(geo.spheremp, nd), qt)))
    vd = mul(geo.g(geo.rspheremp, 4), geo.dss.ld(mul(geo.g(geo.spheremp, 4), var)))
    return out, vd


def qdp_time_avg(Qn0, Qnp1):
    """rkstage 3: (Qdp(n0) + 2*Qdp(np1)) / 3 (prim_advection_mod.F90:645-662)"""
    return mul(add(Qn0, pow2(Qnp1, 2.0)), recip(exact(3.0)))


def advec_tracers_remap_rk2(geo, Qn0, dp, vn0, eta_dot_dpdn, omega_p, dt, nu_q, dp0):
    """Prim_Advec_Tracers_remap_rk2 + qdp_time_avg without the limiter, from fp64 inputs (Qn0 [e][q][k][4][4], eta_dot_dpdn [e][k][4][4]
    of the first 72 levels).  -> dict of triples: Qdp (np1), divdp, divdp_proj, eta_dot_dpdn, omega_p, and the three stage outputs"""
    q0 = exact(Qn0)
    divdp = compute_divdp(geo, vn0)
    q1, dvp = euler_step(geo, q0, dp, vn0, divdp, divdp, dt / 2, 0, nu_q, dp0)
    q2, eta = euler_step(geo, q1, dp, vn0, dvp, exact(eta_dot_dpdn), dt / 2, 1, nu_q, dp0)
    q3, om = euler_step(geo, q2, dp, vn0, dvp, exact(omega_p), dt / 2, 2, nu_q, dp0)
    return dict(Qdp=qdp_time_avg(q0, q3), divdp=divdp, divdp_proj=dvp, eta_dot_dpdn=eta, omega_p=om, stages=(q1, q2, q3))


def element_mass(geo, Qdp):
    """sum_k sum_p spheremp*Qdp per element and tracer (tse_element_mass: points, then levels) from the fp64 Qdp [e][q][k][4][4]"""
    Qdp = np.asarray(Qdp, dtype=np.float64)
    sp = np.asarray(geo.spheremp).astype(LD)[:, None, None]
    q = Qdp.astype(LD)
    v = (sp * q).sum(axis=(2, 3, 4))
    A = (np.abs(sp) * np.abs(q)).sum(axis=(2, 3, 4))
    return T(v, A, 1 + 15 + (NLEV - 1))
