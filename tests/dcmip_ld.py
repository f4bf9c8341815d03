"""The prescribed DCMIP 1-1 / 1-2 fields in numpy longdouble, with a rigorous pointwise error bound that holds for every fp64 evaluation
of the same expressions: the referee of tests/test_dcmip_bound_cpu.py and tests/test_gpu_dcmip_pointwise.py.  Plain numpy; no HIP import;
any level count.

What is modelled.  dcmip_123_mod's test 1-1 and 1-2 point functions with zcoords = 1 (dcmip_123_mod.F90:85-260, 262-409) and the level
constants and products of the wrapper (dcmip_wrapper_mod.F90:49-243), as the program texts state them: orc_dcmip_point / orc_dcmip_init /
orc_dcmip_step_inputs of oracle/tse_oracle.c, and dcmip_point / k_dcmip_* / tse_dcmip_init of the library.  They were read, not imported.

Triples.  Every quantity is a triple T(v, A, m) of tests/step_ld.py, whose arithmetic rules (exact, mul, mul_tight, pow2, recip, the
n-term sum, bound, ratio) are used as they stand.  Every product here goes through mul_tight, because the time factors and s cancel.
A division x / y counts as x * (1 / y), one rounding more than the division has.
  Exact inputs: lat, lon, hyai, hybi, hyam, hybm, time = n * tstep (the fp64 product) and the literals as written; bs is the fp64 value
  of the single-precision literal 0.2f, pi the fp64 literal.  Constants the sources form from literals (H, tau, u0, k0, omega0, ptop,
  rho0, lambda0, 2 pi t / tau, ...) are counted as ordinary operations, so the bound holds however a compiler folds or contracts them.

The rule for a library function y = f(x), x a triple with absolute error E = bound(m_x, A_x):
    |fl - f(v)| <= D + c_f u (|f(v)| + D),   D = sup |f(t) - f(v)| over [v - E, v + E],   u = 2^-53,
  because the fp64 argument lies in that interval and the function is allowed c_f ulps of its own result there.
  exp, log, acos are monotone: D is the larger of the two longdouble differences at the interval's ends.  acos's ends are clipped to
  [-1, 1]: its argument is sin(lat) sin(0) + cos(lat) cos(0) cos(lon - lambda), the first product an exact zero, the second a product of
  cosines (each of magnitude <= 1 from any libm worth the name), which rounding cannot carry past 1 -- so no fp64 evaluation leaves the
  range.  sin and cos are 1-Lipschitz: D <= E.  The longdouble functions' own error (glibc documents 1 to 2 ulps of the 64-bit mantissa for
  expl, logl, sinl, cosl, acosl; 2 ulps <= 4 * 2^-64 relative, at the three values that enter) is added as 8 * 2^-64 (|f(v)| + D).
  The result is the triple (f(v), max(|f(v)|, err / gamma_m), m = m_x + c_f), as mul_tight forms its own.
  c_f is the function's allowance in ulps, not a measurement of any kernel: OpenCL's fp64 limits (OpenCL C 3.0 specification, section
  7.4, "Relative error as ULPs", double precision): exp 3, log 3, sin 4, cos 4, acos 4.  No ROCm device-library accuracy table is
  installed beside the compiler to cite in their place.  The same allowance serves the host's libm (glibc's documented errors of these five lie within it).
fmax / fmin against a constant (plim = fmax(p, ptop), hstar = fmin(z / ztop, 1), d = fmin(d, 1)) are 1-Lipschitz: value max / min, A and m
the larger of the two.  No decision is taken on them.

Counts (m of each quantity; asserted against the code by test_dcmip_bound_cpu.py::test_counts).  Level constants, host side:
  H = (Rd*T0)/g 3;  z = H*log(1/(hya+hyb)): sum 1, recip 2, log 5, *H 9;  p = P0*exp(-z/H): recip H 4, product 14, exp 17, *P0 18
  (pint, ps_v = pint[nlev]: 18);  dph = dhyai*ps0 + dhybi*pint[nlev]: differences 1, products 2 and 20, sum 21;
  dp = pint[k+1] - pint[k]: 19 with A = pint[k+1] + pint[k].
Shared:  tau = 12*86400 1;  2 pi t/tau and pi t/tau 4 (product 1, recip tau 2);  their cosines 8;  lonp = lon - 2 pi t/tau 5, its sine and
  cosine 9;  sin, cos of lat 4;  u0, k0, omega0 4;  ptop = P0*exp(-12000/H) 9;  plim 18;  1/(bs*ptop) 11;  rho = p/(Rd*T0) 21.
Test 1-1:  e1 = exp((ptop-P0)/(bs ptop)) 25;  e2, e3 34;  s = 1 + e1 - e2 - e3 37;
  ud = (omega0 a)/(bs ptop) cos(lonp) (cl cl) cos(2 pi t/tau) (-e2 + e3): 5, 17, 27, 37, 46, 82;
  u = k0 sin sin sin(2 lat) cos(pi t/tau) + u0 cos(lat) + ud: terms 38, 9, 82, 3-term sum 84;  v = k0 sin(2 lonp) cos(lat) cos(pi t/tau) 28;
  w = -((Rd T0)/(g plim)) omega0 sin(lonp) cos(lat) cos(2 pi t/tau) s: 22, 27, 37, 42, 51, 89;  eta_dot_dpdn = (-g rho) w: 22 + 89 + 1 = 112.
  lambda = 5 pi/6 3;  r = acos(sin_tmp + cos_tmp cos(lon - lambda)): 4, 8, 9 and 9, 18, 19, acos 23;  RR = 1/2 2 (exactly 0.5 however
  it is formed), r/RR 27, (r/RR)^2 55;  hz = (z - z0)/ZZ 12, hz^2 25;  d 56, pi d 57, its cosine 61, 1 + 62;
  q1 = 0.5 (1 + cos(pi d1)) + 0.5 (1 + cos(pi d2)) 63;  q2 = 0.9 - 0.8 (q1 q1): 127, 128, 129;  q4 = 1 - 0.3 (q1 + q2 + q3): 131, 132, 133.
Test 1-2:  rho = fmax(p, ptop)/(Rd T0) 21;  rho0 3;  rho0/rho 26;  hstar = fmin(z/ztop, 1) 11;  cos, sin of pi hstar 16;  K lat 1, its
  sine and cosine 5;  u = u0 cos(lat) 5;
  v = -(rho0/rho) (a w0 pi)/(K ztop) cos(lat) sin(K lat) cos(pi hstar) cos(pi t/tau): 29, 32, 37, 43, 60, 69;
  w = (rho0/rho)(w0/K)(-2 sin(K lat) sin(lat) + K cos(lat) cos(K lat)) sin(pi hstar) cos(pi t/tau): 29, (10 and 11, sum 12) 42, 59, 68;
  eta_dot_dpdn 22 + 68 + 1 = 91;  q2 = 0.5 (1 + cos(2 pi (z - z0)/(z2 - z1))): z - z0 10, *2 pi 11, /(z2 - z1) (1, recip 2) 14, cos 18, 19.
Products:  vn0 = u * dp and v * dp with dp the fp64 array of the side under test (an exact input, as in step_ld's per-stage tests; dp as a
  cancelling difference answers to its own triple) m + 1;  Qdp = Q * dph m_Q + 22 (a 0/1 tracer: its exact value times dph, 22).

Decisions.  Each returns a value and a mask of the points where it is decided: a comparison is decided where |lhs - rhs| exceeds the sum
of the two sides' absolute errors.  They are d1 <= RR, d2 <= RR (the normalised squared distance against RR, as the reference compares),
z > z0, |lat| < 0.125 (exact), z1 < z < z2.  The checkerboard sin(9 lon) sin(9 lat) < 0 takes the fp64 products 9.0 * lon and 9.0 * lat as
exact arguments (one IEEE multiplication, the same everywhere); a sine's sign is decided where |sin| exceeds its allowance, or where the
argument is an exact zero (the sine is then +-0, the term +-0, and -0.0 < 0 is false: 1.0); the term's sign follows from the two.  Slots
>= 4 of 1-1 and every slot but the second of 1-2 carry the checkerboard.  An undecided point may hold either of its two values.

Range.  step_ld's range check [2^-700, 2^700] on every nonzero magnitude is used as it stands: the exp arguments of the top levels need
no widening, since plim = fmax(p, ptop) keeps every one of them within [(ptop - P0)/(bs ptop), 0] = [-14.61, 0], and -z/H >= -9.22 on
the 72-level grid (its top interface lies at 10 Pa; the other two grids end at 12 km, -z/H = -1.37)."""
import math

import numpy as np

from step_ld import LD, T, add, bound, exact, gamma, minimum, mul_tight, neg, pow2, ratio, recip, select

U = 2.0 ** -53
C_F = dict(exp=3, log=3, sin=4, cos=4, acos=4)   # OpenCL C 3.0, 7.4, double precision
LD_FN = 8 * 2.0 ** -64                           # the longdouble functions' own error, relative
CAP = 1.0e-3                                     # at most this share of a field's points may be undecided

PI = 3.141592653589793238462643383279
REARTH, RGAS, GRAV, P0, T0 = 6.376e6, 287.04, 9.80616, 100000.0, 300.0
BS = float(np.float32(0.2))                      # dcmip_123_mod.F90:168: a default-real literal
_F = dict(exp=np.exp, log=np.log, sin=np.sin, cos=np.cos, acos=np.arccos)


def fn(name, x):
    """the library function `name` of a triple (the rule of the module docstring)"""
    f, cf = _F[name], C_F[name]
    E = np.asarray(bound(x.m, x.A)).astype(LD)
    if name in ("sin", "cos"):
        v, D = f(x.v), E
    else:
        lo, hi, at = x.v - E, x.v + E, x.v
        if name == "acos":
            lo, hi, at = np.clip(lo, -1, 1), np.clip(hi, -1, 1), np.clip(at, -1, 1)
        if name == "log":
            assert np.all(lo > 0)
        v = f(at)
        D = np.maximum(np.abs(f(lo) - v), np.abs(f(hi) - v))
    av = np.abs(v)
    err = D + LD(cf * U + LD_FN) * (av + D)
    m = x.m + cf
    return T(v, np.maximum(av, err / LD(gamma(m))), m)


def maximum(a, b):
    """max(a, b): 1-Lipschitz in the max norm, as step_ld.minimum"""
    return T(np.maximum(a.v, b.v), np.maximum(a.A, b.A), max(a.m, b.m))


def prod(*ts):
    """a left-to-right product (the count does not depend on the association)"""
    r = ts[0]
    for t in ts[1:]:
        r = mul_tight(r, t)
    return r


def div(a, b):
    return mul_tight(a, recip(b))


def sub(a, b):
    return add(a, neg(b))


def err_of(t):
    """the absolute error bound of a triple, per point"""
    return np.asarray(bound(t.m, t.A)).astype(LD)


def _lev(t):
    """a level quantity [n] against fields [e][n][4][4]"""
    return T(np.asarray(t.v).reshape(1, -1, 1, 1), np.asarray(t.A).reshape(1, -1, 1, 1), t.m)


def _c(x):
    return exact(np.float64(x))


# ---- the constants the sources form from literals ----
def scale_height():
    return div(mul_tight(_c(RGAS), _c(T0)), _c(GRAV))


def rd_t0():
    return mul_tight(_c(RGAS), _c(T0))


def pressure(z, H):
    return mul_tight(_c(P0), fn("exp", div(neg(z), H)))


def p_top(H):
    return mul_tight(_c(P0), fn("exp", div(_c(-12000.0), H)))


class Levels:
    """the wrapper's level constants (tse_dcmip_init's host part, ref_interface_p of the oracle) as triples [nlev] / [nlev + 1]"""

    def __init__(self, hyai, hybi, hyam, hybm, ps0=1.0e5):
        hyai, hybi, hyam, hybm = (np.asarray(x, dtype=np.float64) for x in (hyai, hybi, hyam, hybm))
        self.nlev = hyam.size
        assert hyai.size == self.nlev + 1
        self.H = H = scale_height()
        self.zi = mul_tight(H, fn("log", recip(add(exact(hyai), exact(hybi)))))
        self.zm = mul_tight(H, fn("log", recip(add(exact(hyam), exact(hybm)))))
        self.pint = pressure(self.zi, H)
        self.ps_v = self.pint[self.nlev]
        da, db = sub(exact(hyai[1:]), exact(hyai[:-1])), sub(exact(hybi[1:]), exact(hybi[:-1]))
        self.dph = add(mul_tight(da, _c(ps0)), mul_tight(db, self.ps_v))
        self.dp = sub(self.pint[1:], self.pint[:-1])


def times(nstep, tstep):
    """(t_wind, t_now) as both sides form them: an int times a double"""
    return float(nstep - 1 if nstep > 0 else 0) * float(tstep), float(nstep) * float(tstep)


class Referee:
    """lat, lon: [e][4][4] fp64.  Fields come back as triples shaped [e][levels][4][4] (or broadcastable to it)."""

    def __init__(self, test, lat, lon, hyai, hybi, hyam, hybm):
        assert test in (1, 2)
        self.test = test
        self.lat64 = np.asarray(lat, dtype=np.float64).reshape(-1, 1, 4, 4)
        self.lon64 = np.asarray(lon, dtype=np.float64).reshape(-1, 1, 4, 4)
        self.lat, self.lon = exact(self.lat64), exact(self.lon64)
        self.L = Levels(hyai, hybi, hyam, hybm)
        self.nlev = self.L.nlev
        self.pi = _c(PI)
        self.tau = mul_tight(_c(12.0), _c(86400.0)) if test == 1 else mul_tight(_c(1.0), _c(86400.0))

    # -- time factors --
    def _angle(self, time, two):
        pi = pow2(self.pi, 2.0) if two else self.pi
        return div(mul_tight(pi, _c(time)), self.tau)

    # -- test 1-1 --
    def _levels1(self, z):
        H = self.L.H
        p, ptop = pressure(z, H), p_top(H)
        plim = maximum(p, ptop)
        r = recip(mul_tight(_c(BS), ptop))
        e1 = fn("exp", mul_tight(sub(ptop, _c(P0)), r))
        e2 = fn("exp", mul_tight(sub(plim, _c(P0)), r))
        e3 = fn("exp", mul_tight(sub(ptop, plim), r))
        return dict(p=p, ptop=ptop, plim=plim, rbsp=r, e1=e1, e2=e2, e3=e3, s=add(_c(1.0), e1, neg(e2), neg(e3)))

    def _point1(self, time, z):
        """u, v, w, rho of dcmip_point(test 1) at heights z [1][n][1][1]"""
        a, lat = _c(REARTH), self.lat
        u0 = div(mul_tight(pow2(self.pi, 2.0), a), self.tau)
        k0 = div(mul_tight(_c(10.0), a), self.tau)
        omega0 = div(mul_tight(_c(23000.0), self.pi), self.tau)
        w2t, w1t = self._angle(time, True), self._angle(time, False)
        lonp = sub(self.lon, w2t)
        c2t, c1t = fn("cos", w2t), fn("cos", w1t)
        sl_, cl_ = fn("sin", lonp), fn("cos", lonp)
        cl = fn("cos", lat)
        lv = self._levels1(z)
        ud = prod(mul_tight(omega0, a), lv["rbsp"], cl_, mul_tight(cl, cl), c2t, add(neg(lv["e2"]), lv["e3"]))
        u = add(prod(k0, sl_, sl_, fn("sin", pow2(lat, 2.0)), c1t), mul_tight(u0, fn("cos", lat)), ud)
        v = prod(k0, fn("sin", pow2(lonp, 2.0)), fn("cos", lat), c1t)
        w = prod(neg(div(rd_t0(), mul_tight(_c(GRAV), lv["plim"]))), omega0, sl_, fn("cos", lat), c2t, lv["s"])
        rho = div(lv["p"], rd_t0())
        return dict(u=u, v=v, w=w, rho=rho, s=lv["s"])

    # -- test 1-2 --
    def _point2(self, time, z):
        H, lat = self.L.H, self.lat
        a, w0, K, ztop = _c(REARTH), _c(0.15), _c(5.0), _c(12000.0)
        p, ptop = pressure(z, H), mul_tight(_c(P0), fn("exp", div(neg(ztop), H)))
        rho = div(maximum(p, ptop), rd_t0())
        rr = div(div(_c(P0), rd_t0()), rho)
        hstar = minimum(div(z, ztop), _c(1.0))
        ph = mul_tight(self.pi, hstar)
        c1t = fn("cos", self._angle(time, False))
        klat = mul_tight(K, lat)
        u = mul_tight(_c(40.0), fn("cos", lat))
        v = prod(div(mul_tight(neg(rr), prod(a, w0, self.pi)), mul_tight(K, ztop)), fn("cos", lat), fn("sin", klat), fn("cos", ph), c1t)
        wcol = add(mul_tight(pow2(fn("sin", klat), -2.0), fn("sin", lat)), prod(K, fn("cos", lat), fn("cos", klat)))
        w = prod(mul_tight(rr, div(w0, K)), wcol, fn("sin", ph), c1t)
        return dict(u=u, v=v, w=w, rho=rho)

    def _point(self, time, z):
        return self._point1(time, z) if self.test == 1 else self._point2(time, z)

    # -- the per-step inputs --
    def step_inputs(self, nstep, tstep):
        """u, v [e][nlev][4][4] at t_wind; w, rho, eta_dot_dpdn [e][nlev + 1][4][4] at t_now; dp [1][nlev][1][1]"""
        t_wind, t_now = times(nstep, tstep)
        m = self._point(t_wind, _lev(self.L.zm))
        i = self._point(t_now, _lev(self.L.zi))
        eta = mul_tight(mul_tight(_c(-GRAV), i["rho"]), i["w"])
        return dict(u=m["u"], v=m["v"], w=i["w"], rho=i["rho"], eta=eta, dp=_lev(self.L.dp))

    def vn0(self, ins, dp64):
        """the two components of vn0 (vn0[:, :, 0] and vn0[:, :, 1]) = u * dp, v * dp, with dp64 [e][nlev][4][4] the fp64 array the side
        under test produced"""
        d = exact(np.asarray(dp64, dtype=np.float64))
        return mul_tight(ins["u"], d), mul_tight(ins["v"], d)

    # -- the initial state --
    def checker(self):
        """(value 0.0 / 1.0, decided) per column [e][1][4][4] of sin(9 lon) sin(9 lat) < 0 ? 0 : 1"""
        sg, ok, zero = [], [], []
        for x in (9.0 * self.lon64, 9.0 * self.lat64):        # the fp64 products: exact arguments
            s = fn("sin", exact(x))
            z = x == 0.0
            zero.append(z)
            ok.append(z | (np.abs(s.v) > err_of(s)))
            sg.append(np.signbit(s.v))
        anyzero = zero[0] | zero[1]
        decided = anyzero | (ok[0] & ok[1])
        val = np.where(anyzero, 1.0, np.where(sg[0] != sg[1], 0.0, 1.0))
        return val, decided

    def tracers1(self):
        """q1..q4 of 1-1 at the mid levels: dict q1, q2, q4 (triples), q3 (values 1.0 / 0.1), decided (q3's, also q4's mask)"""
        z, lat, lon = _lev(self.L.zm), self.lat, self.lon
        zero, one = _c(0.0), _c(1.0)
        sin_tmp, cos_tmp = mul_tight(fn("sin", lat), fn("sin", zero)), mul_tight(fn("cos", lat), fn("cos", zero))
        hz = div(sub(z, _c(5000.0)), _c(1000.0))
        hz2 = mul_tight(hz, hz)
        RR = div(_c(1.0), _c(2.0))
        assert float(RR.v) == 0.5
        d = []
        for five in (5.0, 7.0):
            lam = div(mul_tight(_c(five), self.pi), _c(6.0))
            r = fn("acos", add(sin_tmp, mul_tight(cos_tmp, fn("cos", sub(lon, lam)))))
            rr = div(r, RR)
            d.append(minimum(add(mul_tight(rr, rr), hz2), one))
        half = [pow2(add(one, fn("cos", mul_tight(self.pi, x))), 0.5) for x in d]
        q1 = add(*half)
        q2 = sub(_c(0.9), mul_tight(_c(0.8), mul_tight(q1, q1)))
        # decisions
        in_, dec = [], []
        for x in d:
            in_.append(x.v <= RR.v); dec.append(np.abs(x.v - RR.v) > err_of(x) + err_of(RR))
        above, dec_z = z.v > LD(5000.0), np.abs(z.v - LD(5000.0)) > err_of(z)
        band = np.abs(self.lat64) < 0.125                                # exact
        q3 = np.where(above & band, 0.1, np.where(in_[0] | in_[1], 1.0, 0.1))
        decided = dec[0] & dec[1] & (dec_z | ~band)
        q3, decided = np.broadcast_arrays(q3, decided)
        q4 = sub(one, mul_tight(_c(0.3), add(q1, q2, exact(q3))))
        return dict(q1=q1, q2=q2, q3=q3, q4=q4, decided=decided, d1=d[0], d2=d[1])

    def tracer2(self):
        """q2 of 1-2 at the mid levels: (triple, decided)"""
        z = _lev(self.L.zm)
        z1, z2 = 2000.0, 5000.0
        z0 = mul_tight(_c(0.5), add(_c(z1), _c(z2)))
        arg = div(mul_tight(pow2(self.pi, 2.0), sub(z, z0)), sub(_c(z2), _c(z1)))
        q = pow2(add(_c(1.0), fn("cos", arg)), 0.5)
        inside = (z.v < LD(z2)) & (z.v > LD(z1))
        E = err_of(z)
        decided = (np.abs(z.v - LD(z1)) > E) & (np.abs(z.v - LD(z2)) > E)
        zero = T(np.zeros_like(q.v), np.zeros_like(q.A), 0)
        return select(inside, q, zero), decided

    def initial(self, qsize):
        """the tracer slots of dcmip_init: a list of dict(kind="smooth", Q=triple, mask=) or dict(kind="binary", val=, hi=, lo=, decided=),
        every array broadcastable to [e][nlev][4][4]"""
        cval, cdec = self.checker()
        chk = dict(kind="binary", val=cval, hi=1.0, lo=0.0, decided=cdec)
        if self.test == 1:
            t = self.tracers1()
            yes = np.ones_like(t["decided"])
            four = [dict(kind="smooth", Q=t["q1"], mask=yes), dict(kind="smooth", Q=t["q2"], mask=yes),
                    dict(kind="binary", val=t["q3"], hi=1.0, lo=0.1, decided=t["decided"]), dict(kind="smooth", Q=t["q4"], mask=t["decided"])]
            return [four[q] if q < 4 else chk for q in range(qsize)]
        q2, dec = self.tracer2()
        return [dict(kind="smooth", Q=q2, mask=dec) if q == 1 else chk for q in range(qsize)]


def check_step(ref, nstep, tstep, vn0, eta, dp):
    """the per-step inputs of one side (vn0 [e][nlev][2][4][4], eta [e][nlev + 1][4][4], dp [e][nlev][4][4]) against the referee:
    {field: worst ratio} of vn0-u, vn0-v (with this side's own dp as an exact input), eta_dot_dpdn and dp"""
    ins = ref.step_inputs(nstep, tstep)
    tu, tv = ref.vn0(ins, dp)
    vn0 = np.asarray(vn0)
    return {"vn0-u": ratio(vn0[:, :, 0], tu)[0], "vn0-v": ratio(vn0[:, :, 1], tv)[0], "eta_dot_dpdn": ratio(eta, ins["eta"])[0],
            "dp": ratio(dp, ins["dp"])[0]}


def check_initial(ref, qsize, qdp, dph64):
    """Qdp [e][qsize][nlev][4][4] of one time level against the referee's slots; dph64 [nlev]: the fp64 dph of fp64_levels, used only to
    tell which of its two values a 0/1 slot holds.  -> per slot dict(ratio=, undecided=share of the points, wrong=decided points holding
    the other value)"""
    qdp = np.asarray(qdp, dtype=np.float64)
    dph, out = _lev(ref.L.dph), []
    d64 = np.asarray(dph64, dtype=np.float64).reshape(1, -1, 1, 1)
    for q, s in enumerate(ref.initial(qsize)):
        got = qdp[:, q]
        if s["kind"] == "smooth":
            r = ratio(got, mul_tight(s["Q"], dph))[1]
            mask = np.broadcast_to(s["mask"], got.shape)
            out.append(dict(ratio=float(np.where(mask, r, 0.0).max()), undecided=1.0 - mask.mean(), wrong=0))
            continue
        hi, lo = s["hi"], s["lo"]
        r_hi, r_lo = ratio(got, mul_tight(_c(hi), dph))[1], ratio(got, mul_tight(_c(lo), dph))[1]
        val, dec = np.broadcast_to(s["val"], got.shape), np.broadcast_to(s["decided"], got.shape)
        r = np.where(dec, np.where(val == hi, r_hi, r_lo), np.minimum(r_hi, r_lo))
        holds_hi = np.abs(got - hi * d64) < np.abs(got - lo * d64)
        out.append(dict(ratio=float(r.max()), undecided=1.0 - dec.mean(), wrong=int((dec & (holds_hi != (val == hi))).sum())))
    return out


# ---- fp64 restatements: the host part of tse_dcmip_init in Python, and the point functions vectorised (for the level files the oracle is
# not built for, and as the carrier of the planted errors of test_dcmip_bound_cpu.py) ----
def fp64_levels(hyai, hybi, hyam, hybm, ps0=1.0e5):
    """zm, zi, pint, dph in the expressions and operand order of tse_dcmip_init (math.log / math.exp: the host's libm)"""
    H = RGAS * 300.0 / GRAV
    n = len(hyam)
    zi = np.array([H * math.log(1.0 / (hyai[k] + hybi[k])) for k in range(n + 1)])
    pint = np.array([P0 * math.exp(-zi[k] / H) for k in range(n + 1)])
    zm = np.array([H * math.log(1.0 / (hyam[k] + hybm[k])) for k in range(n)])
    dph = np.array([(hyai[k + 1] - hyai[k]) * ps0 + (hybi[k + 1] - hybi[k]) * pint[n] for k in range(n)])
    return dict(zi=zi, zm=zm, pint=pint, dph=dph, dp=pint[1:] - pint[:-1])


def fp64_point(test, time, lon, lat, z, bs=BS):
    """orc_dcmip_point in numpy fp64, broadcasting lon, lat against z; -> dict u, v, w, rho, q (list of 4), term-by-term as the C text"""
    a, pi, Rd, g = REARTH, PI, RGAS, GRAV
    H = Rd * T0 / g
    p = P0 * np.exp(-z / H)
    if test == 1:
        tau = 12.0 * 86400.0
        u0, k0, omega0 = (2.0 * pi * a) / tau, (10.0 * a) / tau, (23000.0 * pi) / tau
        RR, ZZ, z0, lambda0, lambda1 = 1.0 / 2.0, 1000.0, 5000.0, 5.0 * pi / 6.0, 7.0 * pi / 6.0
        ptop = P0 * math.exp(-12000.0 / H)
        lonp = lon - 2.0 * pi * time / tau
        plim = np.maximum(p, ptop)
        s = 1.0 + math.exp((ptop - P0) / (bs * ptop)) - np.exp((plim - P0) / (bs * ptop)) - np.exp((ptop - plim) / (bs * ptop))
        cl = np.cos(lat)
        ud = (omega0 * a) / (bs * ptop) * np.cos(lonp) * (cl * cl) * math.cos(2.0 * pi * time / tau) * \
            (-np.exp((plim - P0) / (bs * ptop)) + np.exp((ptop - plim) / (bs * ptop)))
        u = k0 * np.sin(lonp) * np.sin(lonp) * np.sin(2.0 * lat) * math.cos(pi * time / tau) + u0 * np.cos(lat) + ud
        v = k0 * np.sin(2.0 * lonp) * np.cos(lat) * math.cos(pi * time / tau)
        w = -((Rd * T0) / (g * plim)) * omega0 * np.sin(lonp) * np.cos(lat) * math.cos(2.0 * pi * time / tau) * s
        rho = p / (Rd * T0)
        sin_tmp, cos_tmp = np.sin(lat) * math.sin(0.0), np.cos(lat) * math.cos(0.0)
        r1 = np.arccos(sin_tmp + cos_tmp * np.cos(lon - lambda0))
        r2 = np.arccos(sin_tmp + cos_tmp * np.cos(lon - lambda1))
        hz = (z - z0) / ZZ
        d1 = np.minimum((r1 / RR) * (r1 / RR) + hz * hz, 1.0)
        d2 = np.minimum((r2 / RR) * (r2 / RR) + hz * hz, 1.0)
        q1 = 0.5 * (1.0 + np.cos(pi * d1)) + 0.5 * (1.0 + np.cos(pi * d2))
        q2 = 0.9 - 0.8 * (q1 * q1)
        q3 = np.where((d1 <= RR) | (d2 <= RR), 1.0, 0.1)
        q3 = np.where((z > z0) & (np.abs(lat) < 0.125), 0.1, q3)
        q4 = 1.0 - 0.3 * (q1 + q2 + q3)
        return dict(u=u, v=v, w=w, rho=rho, q=[q1, q2, q3, q4])
    tau, u0, w0, K, z1, z2, ztop = 1.0 * 86400.0, 40.0, 0.15, 5.0, 2000.0, 5000.0, 12000.0
    z0 = 0.5 * (z1 + z2)
    ptop = P0 * math.exp(-ztop / H)
    rho = np.maximum(p, ptop) / (Rd * T0)
    rho0 = P0 / (Rd * T0)
    hstar = np.minimum(z / ztop, 1.0)
    ct = math.cos(pi * time / tau)
    u = u0 * np.cos(lat) + 0.0 * z
    v = -(rho0 / rho) * (a * w0 * pi) / (K * ztop) * np.cos(lat) * np.sin(K * lat) * np.cos(pi * hstar) * ct
    w = (rho0 / rho) * (w0 / K) * (-2.0 * np.sin(K * lat) * np.sin(lat) + K * np.cos(lat) * np.cos(K * lat)) * np.sin(pi * hstar) * ct
    q2 = np.where((z < z2) & (z > z1), 0.5 * (1.0 + np.cos(2.0 * pi * (z - z0) / (z2 - z1))), 0.0) + 0.0 * lat
    zero = np.zeros_like(q2)
    return dict(u=u, v=v, w=w, rho=rho + 0.0 * lat, q=[zero, q2, zero, zero])


def fp64_step_inputs(test, nstep, tstep, lat, lon, lev, bs=BS, v_at_now=False, w_table_shift=0):
    """orc_dcmip_step_inputs on fp64_levels' constants: dict vn0 [e][nlev][2][4][4], eta [e][nlev + 1][4][4], dp [e][nlev][4][4].
    The switches plant errors: bs; v evaluated at t_now; w of 1-2 at the top w_table_shift interfaces taken from the interface below."""
    lat, lon = np.asarray(lat).reshape(-1, 1, 4, 4), np.asarray(lon).reshape(-1, 1, 4, 4)
    t_wind, t_now = times(nstep, tstep)
    lv = lambda x: np.asarray(x).reshape(1, -1, 1, 1)   # noqa: E731
    m = fp64_point(test, t_wind, lon, lat, lv(lev["zm"]), bs)
    if v_at_now:
        m["v"] = fp64_point(test, t_now, lon, lat, lv(lev["zm"]), bs)["v"]
    i = fp64_point(test, t_now, lon, lat, lv(lev["zi"]), bs)
    w = i["w"].copy()
    if w_table_shift:
        w[:, :w_table_shift] = i["w"][:, 1:w_table_shift + 1]
    dp = np.broadcast_to(lv(lev["dp"]), m["u"].shape).copy()
    vn0 = np.stack([0.0 + 1.0 * m["u"] * dp, 0.0 + 1.0 * m["v"] * dp], axis=2)
    return dict(vn0=vn0, eta=-GRAV * i["rho"] * w, dp=dp)


def fp64_initial(test, qsize, lat, lon, lev, checker_le=False):
    """orc_dcmip_init on fp64_levels' constants: Qdp [e][qsize][nlev][4][4]; checker_le plants `<=` in the checkerboard"""
    lat, lon = np.asarray(lat).reshape(-1, 1, 4, 4), np.asarray(lon).reshape(-1, 1, 4, 4)
    term = np.sin(9.0 * lon) * np.sin(9.0 * lat)
    checker = np.where(term <= 0.0 if checker_le else term < 0.0, 0.0, 1.0)
    m = fp64_point(test, 0.0, lon, lat, np.asarray(lev["zm"]).reshape(1, -1, 1, 1))
    dph = np.asarray(lev["dph"]).reshape(1, -1, 1, 1)
    shp = np.broadcast_shapes(m["q"][1].shape, checker.shape)
    slots = []
    for q in range(qsize):
        Q = (m["q"][q] if q < 4 else checker) if test == 1 else (m["q"][1] if q == 1 else checker)
        slots.append(np.broadcast_to(Q, shp) * dph)
    return np.stack(slots, axis=1)
