"""numpy model of the tracer forcing (tse_apply_forcing; csrc/tse_view_kernels.h: forcing_rule, k_forcing): the rule operation for operation, the
budget in THE ORDER of k_norm_partials, an exact referee for the budget's sums, and the generator of the fields the tests use.

The rule, for every value of Qdp = Qdp(nt), each operation rounded once (numpy never contracts):
    mode 0 (tendency)  v = dt * FQ
    mode 1 (adjust)    dpk = level_dp(k, ps_v);  Q = Qdp / dpk;  v = dpk * (FQ - Q)
    asked = v;  if (Qdp + v < 0 and v < 0): v = 0.0 if Qdp < 0 else -Qdp;  Qdp = Qdp + v
The branches: 0 no clip, 1 clipped to -Qdp (the mass ends at +0.0), 2 clipped to 0.0 (a negative mass is left alone).

The budget of one (element, tracer): entry 0 = sum w[p] * v, entry 1 = sum w[p] * (asked - v) over the 16 points and all levels, w = spheremp,
every term one rounded product, added in THE ORDER (tests/norm_model.py): lane (p, g) adds the nlev/4 levels of group g ascending from 0.0,
column p = ((s0 + s1) + s2) + s3, then S = 0.0; S = S + c(p) for p = 0..15.

The closure bound (u = 2^-53, gamma(m) = m u / (1 - m u), Higham section 4.2), n = 16 * nlev terms per (element, tracer):
the call leaves Qa_i = fl(Qb_i + v_i), so |Qa_i - (Qb_i + v_i)| <= u |Qa_i| and the exact change of mass D = sum w_i Qa_i - sum w_i Qb_i
differs from sum w_i v_i by at most u * A, A = sum w_i |Qa_i|.  Entry 0 adds t_i = fl(w_i v_i), |t_i - w_i v_i| <= u |w_i v_i| <= u |t_i| / (1 - u),
in n - 1 additions: |entry 0 - sum t_i| <= gamma(n-1) * T, T = sum |t_i|.  Together
    |entry 0 - D| <= (gamma(n-1) + 2u) * T + u * A,
and T and A are themselves evaluated with rounded terms and one exact sum (relative error below 3u): closure_bound multiplies by 1 + 4u."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
NLG = 4            # level groups of THE ORDER (NORM_LG)
FAMILIES = 8
DT = 1800.0
NOCLIP, CLIP_TO_ZERO_MASS, LEFT_ALONE = 0, 1, 2


def gamma(m):
    return m * U / (1.0 - m * U)


def level_dp(hyai, hybi, ps0, ps_v):
    """dp[e][k][j][i] = (hyai(k+1)-hyai(k))*ps0 + (hybi(k+1)-hybi(k))*ps_v: the operand order of level_dp (csrc/tse_kernels.h)"""
    hyai = np.asarray(hyai, np.float64); hybi = np.asarray(hybi, np.float64)
    da = (hyai[1:] - hyai[:-1])[None, :, None, None]
    db = (hybi[1:] - hybi[:-1])[None, :, None, None]
    return da * ps0 + db * np.asarray(ps_v, np.float64)[:, None, :, :]


def apply(qdp, fq, dt, mode, dp=None, plant=None):
    """qdp, fq [e][q][k][j][i] (fq may broadcast), dp [e][k][j][i] (mode 1) -> dict(new=, applied=, withheld=, branch=).
    plant: one deliberate error, for the tests that show a bit comparison catching it --
      "ignore_negative": the clip ignores Qdp < 0;  "le": v <= 0 in place of v < 0."""
    qdp = np.asarray(qdp, np.float64)
    fq = np.broadcast_to(np.asarray(fq, np.float64), qdp.shape)
    with np.errstate(all="ignore"):
        if mode == 0:
            v = dt * fq
        else:
            dpk = np.asarray(dp, np.float64)[:, None]
            Q = qdp / dpk
            v = dpk * (fq - Q)
        asked = v
        down = (v <= 0.0) if plant == "le" else (v < 0.0)
        clip = (qdp + v < 0.0) & down
        to = -qdp if plant == "ignore_negative" else np.where(qdp < 0.0, 0.0, -qdp)
        v = np.where(clip, to, v)
        new = qdp + v
        withheld = asked - v
    branch = np.where(clip, np.where(qdp < 0.0, LEFT_ALONE, CLIP_TO_ZERO_MASS), NOCLIP)
    return dict(new=new, applied=v, withheld=withheld, branch=branch)


def _ordered_sum(t):
    """THE ORDER: t[e][q][k][16] -> [e][q]"""
    nlev = t.shape[2]
    assert nlev % NLG == 0
    lpg = nlev // NLG
    s = []
    for g in range(NLG):
        a = np.zeros(t.shape[:2] + (16,))
        for k in range(g * lpg, (g + 1) * lpg):
            a = a + t[:, :, k, :]
        s.append(a)
    c = ((s[0] + s[1]) + s[2]) + s[3]
    S = np.zeros(t.shape[:2])
    for p in range(16):
        S = S + c[:, :, p]
    return S


def budget(spheremp, res, plant=None):
    """[e][q][2] of a result of apply().  plant "no_withheld": the budget leaves out the withheld part."""
    w = np.asarray(spheremp, np.float64).reshape(-1, 1, 1, 16)
    sh = res["applied"].shape[:3] + (16,)
    out = np.zeros(sh[:2] + (2,))
    out[:, :, 0] = _ordered_sum(w * res["applied"].reshape(sh))
    if plant != "no_withheld":
        out[:, :, 1] = _ordered_sum(w * res["withheld"].reshape(sh))
    return out


def exact_budget(spheremp, res):
    """the referee: [e][q][2] of the exact sums of the ROUNDED terms w * v, each rounded once (math.fsum)"""
    w = np.asarray(spheremp, np.float64).reshape(-1, 1, 1, 16)
    sh = res["applied"].shape[:3] + (16,)
    out = np.zeros(sh[:2] + (2,))
    for j, key in enumerate(("applied", "withheld")):
        t = w * res[key].reshape(sh)
        for e in range(sh[0]):
            for q in range(sh[1]):
                out[e, q, j] = math.fsum(t[e, q].reshape(-1).tolist())
    return out


def exact_mass_change(spheremp, before, after):
    """[e][q] Fractions: sum w * after - sum w * before, exactly"""
    w = np.asarray(spheremp, np.float64).reshape(-1, 16)
    ne, nq = before.shape[:2]
    out = np.empty((ne, nq), dtype=object)
    for e in range(ne):
        wf = [Fraction(x) for x in w[e].tolist()]
        for q in range(nq):
            b = before[e, q].reshape(-1, 16).tolist(); a = after[e, q].reshape(-1, 16).tolist()
            tot = Fraction(0)
            for rb, ra in zip(b, a):
                for p in range(16):
                    tot += wf[p] * (Fraction(ra[p]) - Fraction(rb[p]))
            out[e, q] = tot
    return out


def closure_bound(spheremp, res):
    """[e][q]: the bound of the module docstring on |entry 0 - exact mass change|"""
    w = np.asarray(spheremp, np.float64).reshape(-1, 1, 1, 16)
    sh = res["applied"].shape[:3] + (16,)
    n = sh[2] * 16
    T = np.abs(w * res["applied"].reshape(sh)); A = w * np.abs(res["new"].reshape(sh))
    out = np.zeros(sh[:2])
    for e in range(sh[0]):
        for q in range(sh[1]):
            t = math.fsum(T[e, q].reshape(-1).tolist()); a = math.fsum(A[e, q].reshape(-1).tolist())
            out[e, q] = ((gamma(n - 1) + 2 * U) * t + U * a) * (1.0 + 4 * U)
    return out


def fma_contracted(dt, fq, qdp):
    """fl(dt * fq + qdp) with ONE rounding, what a contracted v_fma_f64 leaves where the rule does not clip: exact rational arithmetic,
    rounded to nearest even by Fraction.__float__ (math.fma where the interpreter has it)"""
    f = getattr(math, "fma", None)
    if f is not None:
        return np.array([f(dt, a, b) for a, b in zip(fq.tolist(), qdp.tolist())])
    fd = Fraction(dt)
    return np.array([float(fd * Fraction(a) + Fraction(b)) for a, b in zip(fq.tolist(), qdp.tolist())])


def family_of(shape):
    """the family of every entry: flat index % 8"""
    return (np.arange(int(np.prod(shape)), dtype=np.int64) % FAMILIES).reshape(shape)


def forcing_fields(nelemd, qsize, nlev, seed=20261020, mode=0, hv=None, families=tuple(range(FAMILIES))):
    """Qdp[e][q][k][j][i], FQ (same shape), ps_v[e][j][i], dt.  Entry number n (flat index) belongs to family families[n % 8 % len(families)]
    -- family n % 8 with the default, so every family occurs N // 8 times by construction:
      0  FQ > 0                                      1  FQ < 0 without a clip (|dt FQ| < Qdp / 2)
      2  Qdp > 0, dt FQ < -Qdp: clipped to +0.0      3  Qdp < 0 (an undershoot of about 1e-13 of the field), FQ < 0: left alone
      4  Qdp < 0, FQ > 0 large: becomes positive     5  Qdp + dt FQ lands on 0 (entry n // 8 % 3 == 0), one ulp above (1), one ulp below (2)
      6  Qdp = +0.0 / -0.0 (n // 8 even / odd), FQ < 0
      7  FQ = +0.0 / -0.0 (n // 8 even / odd); Qdp > 0 (n // 16 even) or a negative undershoot (odd)
    mode 1 (adjust; hv = (hyai, hybi, ps0) is needed): FQ is the new mixing ratio and the same families are expressed through FQ - Q, Q =
    Qdp / dp: 0 FQ > Q; 1 FQ = Q (1 - r), r < 1/2; 2 FQ = -Q r: more than the mass is taken; 3, 4, 6 FQ = -+ field / dp; 5 FQ = 0.0, so that
    v = -(dp * (Qdp / dp)) cancels Qdp to within an ulp, on either side as the roundings fall; 7 FQ = Q, v = +0.0."""
    rng = np.random.default_rng(seed)
    shape = (nelemd, qsize, nlev, 4, 4)
    N = int(np.prod(shape))
    n = np.arange(N, dtype=np.int64)
    fam = np.asarray(families, dtype=np.int64)[(n % FAMILIES) % len(families)]
    sub = n // FAMILIES
    base = 10.0 ** rng.uniform(-1.0, 3.0, N)
    r = rng.uniform(0.05, 0.45, N)
    big = rng.uniform(0.1, 3.0, N)
    under = -1e-13 * base * rng.uniform(0.1, 1.0, N)
    ps_v = 1.0e5 * (1.0 + 0.03 * rng.uniform(-1.0, 1.0, (nelemd, 4, 4)))
    dt = DT
    qdp = base.copy()
    qdp[(fam == 3) | (fam == 4)] = under[(fam == 3) | (fam == 4)]
    qdp[(fam == 6) & (sub % 2 == 0)] = 0.0
    qdp[(fam == 6) & (sub % 2 == 1)] = -0.0
    m7 = (fam == 7) & (sub // 2 % 2 == 1)
    qdp[m7] = under[m7]
    fq = np.zeros(N)
    if mode == 0:
        fq[fam == 0] = (base * big / dt)[fam == 0]
        for f in (1, 3, 6):
            fq[fam == f] = (-(r * base) / dt)[fam == f]
        fq[fam == 2] = (-(base * (1.0 + big)) / dt)[fam == 2]
        fq[fam == 4] = ((r * base) / dt)[fam == 4]
        m5 = fam == 5
        fq[m5] = (-(base / dt))[m5]
        q5 = -(dt * fq)                                   # Qdp + dt*FQ == 0 exactly
        q5 = np.where(sub % 3 == 1, np.nextafter(q5, np.inf), np.where(sub % 3 == 2, np.nextafter(q5, 0.0), q5))
        qdp[m5] = q5[m5]
        fq[(fam == 7) & (sub % 2 == 1)] = -0.0
    else:
        dp = np.broadcast_to(level_dp(hv[0], hv[1], hv[2], ps_v)[:, None], shape).reshape(-1)
        Q = qdp / dp
        fq[fam == 0] = (Q + (base * big) / dp)[fam == 0]
        fq[fam == 1] = (Q * (1.0 - r))[fam == 1]
        fq[fam == 2] = (-(Q * big))[fam == 2]
        for f in (3, 6):
            fq[fam == f] = (-(r * base) / dp)[fam == f]
        fq[fam == 4] = ((r * base) / dp)[fam == 4]
        fq[fam == 5] = 0.0
        fq[fam == 7] = Q[fam == 7]
    return qdp.reshape(shape), fq.reshape(shape), ps_v, dt


def layouts(nelemd, qsize, nlev):
    """the FQ views of the GPU test: (label, strides in doubles (e, q, k, j, i), doubles the buffer needs, offset of the view's first entry,
    expected path of tse_view_plan("qdp"), axes FQ is constant along)"""
    import view_model as vm
    e, q, k, j, i = range(5)
    ext = (nelemd, qsize, nlev, 4, 4)
    K = nlev
    out = []
    s, n = vm.nested_strides(ext, (i, j, k, q, e))
    out.append(("p0 dense", s, n, 0, 0, ()))
    s, n = vm.nested_strides(ext, (i, j, k, q, e), pads={q: (5 - qsize) * K * 16 + 48})
    out.append(("p0 qsize_d=5 and an element gap", s, n, 0, 0, ()))
    s, n = vm.nested_strides(ext, (i, j, k, q, e))
    out.append(("p0 base shifted by one double", s, n + 1, 1, 0, ()))
    s, n = vm.nested_strides(ext, (k, i, j, q, e))
    out.append(("p1 dense", s, n, 0, 1, ()))
    s, n = vm.nested_strides(ext, (k, i, j, q, e), pads={k: 3})
    out.append(("p1 rows of nlev + 3", s, n, 0, 1, ()))
    s, n = vm.nested_strides(ext, (j, i, k, q, e))
    out.append(("p2 j and i swapped", s, n, 0, 2, ()))
    s, n = vm.nested_strides(ext, (i, j, k, q, e))
    s = [-s[e], s[q], -s[k], s[j], s[i]]
    out.append(("p0 negative element and level strides", s, n, (nelemd - 1) * -s[e] + (K - 1) * -s[k], 0, ()))
    s, n = vm.nested_strides((1, qsize, nlev, 4, 4), (i, j, k, q))
    out.append(("p0 zero element stride", [0] + s[1:], n, 0, 0, (e,)))
    s, n = vm.nested_strides((nelemd, 1, nlev, 4, 4), (k, i, j, e))
    out.append(("p1 zero q stride", [s[e], 0] + s[2:], n, 0, 1, (q,)))
    return [(lab, s, n + 5, base, path, const) for lab, s, n, base, path, const in out]   # (five spare doubles behind every view)


def broadcast_along(fq, const):
    """fq made constant along the axes `const` (the first index is kept): the logical field a zero stride describes"""
    for a in const:
        fq = np.broadcast_to(np.take(fq, [0], axis=a), fq.shape)
    return np.ascontiguousarray(fq)


def intended_branch(qdp, fq, dt, mode, dp=None, families=tuple(range(FAMILIES))):
    """the branch every entry is built to take, from its family and sub-case alone; -1 where the family leaves it to the roundings
    (family 5 under adjust: the landing within one ulp of zero is what is asserted there)"""
    shape = qdp.shape
    n = np.arange(qdp.size, dtype=np.int64)
    fam = np.asarray(families, dtype=np.int64)[(n % FAMILIES) % len(families)]
    sub = n // FAMILIES
    want = np.full(qdp.size, NOCLIP, dtype=np.int64)
    want[(fam == 2) | (fam == 6)] = CLIP_TO_ZERO_MASS
    want[fam == 3] = LEFT_ALONE
    if mode == 0:
        want[(fam == 5) & (sub % 3 == 2)] = CLIP_TO_ZERO_MASS
    else:
        want[fam == 5] = -1
    return want.reshape(shape)
