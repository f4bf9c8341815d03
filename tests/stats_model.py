"""The model of tse_stats_view: the 16 entries of every share in the device's own order of addition, an exact referee and the forward bound
that follows from the order.  Plain numpy; no HIP import.

Shapes: h, ht [E][nf][nk][4][4] (or [...][16]); w [E][nk][4][4]; spheremp [E][4][4].  Points in memory order p = 4j + i.

THE ORDER (include/transport_se_hip.h, csrc/tse_view_kernels.h: k_stats_view):
  level share   the 16 terms of a slab as the pairwise tree (((t0+t1)+(t2+t3))+((t4+t5)+(t6+t7))) + (the same of t8..t15): four pairwise
                reshapes (tree16);
  element share S = L(0); S = S + L(1); ... ascending in k.
Extrema take the same route; a NaN enters an extremum as its identity (+inf for the minimum, -inf for the maximum, 0 for the maxima of
absolute values) and enters the sums as it is.

The referee adds the EXACT terms (fractions.Fraction: products and differences of doubles without rounding) and rounds once.  The bound
on |model - referee| is the textbook first-order one for a fixed summation tree: every term passes 4 additions of the tree over points and
at most nk - 1 additions over levels (level shares: none), after the n_mul products of its own (N_MUL: 1 to 3, the product spheremp * w
with a weight among them), so
    |model - referee| <= (4 + (nk - 1) + n_mul) * u * sum |term|,   u = 2^-53.
The rounding of the difference d = h - ht in entries 8 and 10 is not counted, as the bound is stated for the entry: a count of every
rounding would add 1 to entry 8 and 2 to entry 10.  The model lies under the tighter constant (worst ratio 0.63 on the ne2 fixtures).
Nothing in it is measured."""
import fractions
import math

import numpy as np

U = 2.0 ** -53
STATS = 16
SUMS = (2, 3, 4, 5, 8, 9, 10, 11, 14)          # entry 7 is a sum of 0 / 1: exact
MINS, MAXS = (0,), (1, 6, 12, 13)
# products in a term (without a weight; a weight adds one to every entry that has m)
N_MUL = {2: 0, 3: 1, 4: 1, 5: 2, 8: 1, 9: 1, 10: 2, 11: 2, 14: 0}
HAS_M = (3, 4, 5, 8, 9, 10, 11, 14)
SCALE_1 = (0, 1, 2, 3, 4, 6, 8, 9, 12, 13)     # entries that scale with the field; 5, 10, 11 scale with its square
SCALE_2 = (5, 10, 11)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_or_both_nan(a, b):
    """equal bits, except that two NaNs are equal whatever their payloads (the sums of a slab that holds a NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def tree16(t, op=np.add):
    """t[..., 16] -> [...]: the pairwise tree over the points"""
    for _ in range(4):
        t = op(t[..., 0::2], t[..., 1::2])
    return t[..., 0]


def _flat(x, nd):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(x.shape[:nd] + (16,))


def terms(h, spheremp, ht=None, w=None, plant=None):
    """(t[16][E][nf][nk][16], kinds): the 16 terms of every point; a NaN already replaced by the identity in the extrema.
    plant: one deliberate error -- "weight_in_sum" entry 2 formed as w * h; "fused_square" entry 5 as (m * h) * h; "transpose" spheremp
    read as [i][j]"""
    h = _flat(h, 3)
    E, nf, nk = h.shape[:3]
    sm = np.asarray(spheremp, dtype=np.float64).reshape(E, 4, 4)
    if plant == "transpose":
        sm = sm.transpose(0, 2, 1)
    m = np.broadcast_to(sm.reshape(E, 1, 1, 16), h.shape)
    if w is not None:
        m = m * _flat(w, 2)[:, None]
    t = np.zeros((STATS,) + h.shape)
    nan = np.isnan(h)
    ah = np.abs(h)
    t[0] = np.where(nan, np.inf, h); t[1] = np.where(nan, -np.inf, h); t[2] = h
    t[3] = m * h; t[4] = m * ah; t[5] = m * (h * h)
    t[6] = np.where(nan, 0.0, ah); t[7] = (~np.isfinite(h)).astype(np.float64); t[14] = m
    if plant == "weight_in_sum":
        t[2] = _flat(w, 2)[:, None] * h
    elif plant == "fused_square":
        t[5] = (m * h) * h
    if ht is not None:
        ht = _flat(ht, 3)
        with np.errstate(invalid="ignore"):
            d = h - ht
        ad, at = np.abs(d), np.abs(ht)
        t[8] = m * ad; t[9] = m * at; t[10] = m * (d * d); t[11] = m * (ht * ht)
        t[12] = np.where(np.isnan(d), 0.0, ad); t[13] = np.where(np.isnan(ht), 0.0, at)
    return t


def _op(j):
    return np.minimum if j in MINS else np.maximum if j in MAXS else np.add


def level_shares(h, spheremp, ht=None, w=None, plant=None):
    """out[E][nf][nk][16] of per_level = 1.  plant (besides those of terms): "drop_point" the last point of every slab left out"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = terms(h, spheremp, ht, w, plant)
        out = np.empty(t.shape[1:4] + (STATS,))
        for j in range(STATS):
            x = t[j]
            if plant == "drop_point":
                x = x.copy(); x[..., 15] = np.inf if j in MINS else -np.inf if j in (1,) else 0.0
            out[..., j] = tree16(x, _op(j))
    return out


def element_shares(levels, descending=False):
    """levels[E][nf][nk][16] -> out[E][nf][16] of per_level = 0: S = L(0); S = S + L(1); ...  descending: the planted other order"""
    L = levels[:, :, ::-1] if descending else levels
    out = L[:, :, 0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, L.shape[2]):
            for j in range(STATS):
                out[..., j] = _op(j)(out[..., j], L[:, :, k, j])
    return out


def model(h, spheremp, ht=None, w=None, per_level=False, plant=None):
    lev = level_shares(h, spheremp, ht, w, None if plant == "descending" else plant)
    return lev if per_level else element_shares(lev, descending=plant == "descending")


# ---- the referee ---------------------------------------------------------------------------------------------------------------
def exact_sums(h, spheremp, ht=None, w=None, per_level=False):
    """(S, A): the exact sums of the unrounded terms of entries SUMS, rounded once, and the sums of their absolute values, as
    [E][nf]([nk])[16] (the other entries 0).  All inputs finite."""
    F = fractions.Fraction
    h = _flat(h, 3)
    E, nf, nk = h.shape[:3]
    sm = np.asarray(spheremp, dtype=np.float64).reshape(E, 16)
    ht = None if ht is None else _flat(ht, 3)
    w = None if w is None else _flat(w, 2)
    shape = (E, nf, nk) if per_level else (E, nf)
    S, A = np.zeros(shape + (STATS,)), np.zeros(shape + (STATS,))
    js = [j for j in SUMS if ht is not None or j < 8 or j == 14]
    for e in range(E):
        me = [[F(sm[e, p]) * (F(w[e, k, p]) if w is not None else 1) for p in range(16)] for k in range(nk)]
        for f in range(nf):
            lev = []
            for k in range(nk):
                acc = {j: [F(0), F(0)] for j in js}
                for p in range(16):
                    x, m = F(h[e, f, k, p]), me[k][p]
                    tt = {2: x, 3: m * x, 4: m * abs(x), 5: m * x * x, 14: m}
                    if ht is not None:
                        y = F(ht[e, f, k, p]); d = x - y
                        tt.update({8: m * abs(d), 9: m * abs(y), 10: m * d * d, 11: m * y * y})
                    for j in js:
                        acc[j][0] += tt[j]; acc[j][1] += abs(tt[j])
                lev.append(acc)
            if per_level:
                for k in range(nk):
                    for j in js:
                        S[e, f, k, j] = float(lev[k][j][0]); A[e, f, k, j] = float(lev[k][j][1])
            else:
                for j in js:
                    S[e, f, j] = float(sum(a[j][0] for a in lev)); A[e, f, j] = float(sum(a[j][1] for a in lev))
    return S, A


def bound(A, nk, weight=False, per_level=False):
    """the forward bound on |model - referee| for the sums of absolute values A[..., 16] (module docstring)"""
    B = np.zeros_like(A)
    for j in SUMS:
        n = 4 + (0 if per_level else nk - 1) + N_MUL[j] + (1 if weight and j in HAS_M else 0)
        B[..., j] = n * U * A[..., j] * (1.0 + 2.0 * U)       # (A itself was rounded once on its way to a double)
    return B


def worst_ratio(got, S, B):
    """the largest |got - S| / B over the sum entries (0 / 0 counts as 0)"""
    worst = 0.0
    for j in SUMS:
        err, b = np.abs(got[..., j] - S[..., j]), B[..., j]
        assert np.all(err[b == 0] == 0), j
        if np.any(b > 0):
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    return worst


# ---- the reference's three norms, transcribed (global_norms_mod.F90: l1_snorm, l2_snorm, linf_snorm over global_integral) ----------
def global_integral(h, spheremp):
    """h[E][4][4]: J(ie) = sum over j, i of da * h, da = spheremp, added in the loop's order; the sum of J over elements exact (repro_sum)"""
    E = h.shape[0]
    J = np.zeros(E)
    for j in range(4):
        for i in range(4):
            J = J + spheremp[:, j, i] * h[:, j, i]
    return math.fsum(J.tolist()) / (4.0 * math.pi)


def snorms(h, ht, spheremp):
    """(l1, l2, linf) of one level h, ht [E][4][4]"""
    l1 = global_integral(np.abs(h - ht), spheremp) / global_integral(np.abs(ht), spheremp)
    l2 = math.sqrt(global_integral((h - ht) ** 2, spheremp)) / math.sqrt(global_integral(ht ** 2, spheremp))
    linf = float(np.abs(h - ht).max()) / float(np.abs(ht).max())
    return l1, l2, linf
