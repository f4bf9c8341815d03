"""The model of tse_sphere_op_view.  Plain numpy; no HIP import.

The operators are the reference's gradient_sphere (derivative_mod.F90:1660-1700), divergence_sphere (:2364-2414) and vorticity_sphere
(:2250-2301), and with c0 the make_C0 / make_C0_vector of viscosity_mod.F90:445-535 behind them: rspheremp * DSS(spheremp * op(f)).
Fields are [n][nf][nk][4 j][4 i]: nf = 1 for a scalar, 2 for a wind or a gradient (lat/lon components), as the entry's views.

reference(g, op, x)      the three routines in their source order of operations (the serial sums of the loops from 0.0, the products left
                         to right) for any numpy float type: in fp64 it has the bits of the oracle's gradient_sphere and
                         divergence_sphere (test_sphere_ops_cpu.py), which have the reference's; vorticity_sphere has no oracle, and is held to the
                         reference's own output in test_reference_fieldops_cpu.py (as are the other two, and the C0 forms).
device_order(o, D, op, x)  the order of operations of csrc/tse_device.h: the x-derivative a product and three fused multiply-adds, the
                         y-derivative quad_matvec's two-stage sum, the metric maps a product and a fused multiply-add, vorticity through
                         the tables Dr = rrearth * D.  A fused multiply-add is restated as one longdouble multiply-add rounded to fp64,
                         which is not always the bit of a true one: this restatement is held to the bound, not to bits.
longdouble(o, D, op, f, c0)  (value, A): `reference` in np.longdouble from the fp64 inputs, and the same chain on the absolute values of
                         every factor and term, the difference dvdx - dudy of the vorticity a sum.  c0: w = spheremp * value, the
                         longdouble sum of w over the copies of a node (the node identity from the mesh's coordinates), times rspheremp;
                         A is carried through the same three steps.

Forward bound elem_ops_ld.bound(N, A), as elem_ops_ld.py derives it: N is the longest chain of roundings that multiplies one product term
on its way to the result, over the reference's association and the device's alike.
  gradient_sphere     reference: Dvv * s 1, the 4-term sum 3, * rrearth 1, Dinv * v 1, the sum of the two 1                      ->  7
                      device:    the product and three fmas of d/dx (or quad_matvec's four roundings) 4, rrearth * 1, Dinv * w 1,
                                 fma 1                                                                                           ->  7
  divergence_sphere   N_DIV of elem_ops_ld.py                                                                                    -> 13
  vorticity_sphere    reference: D * v 1, the sum of the two 1, * Dvv 1, the 8-term sum dvdx - dudy 7, the factor rmetdet * rrearth
                                 1, the product with it 1                                                                        -> 12
                      device:    the table rrearth * D 1, Dr * v 1, fma 1, d/dx or quad_matvec 4, the difference 1, rmetdet * 1  ->  9
  N_GRAD = 7, N_DIV = 13, N_VOR = 12.   c0 adds the product with spheremp, the three additions at a node and the product with
  rspheremp: + 5.
The counts are derived from the two codes, not fitted to what the device returns."""
import numpy as np

import biharmonic_model as bm
import dss_view_model as dm
import elem_ops_ld as ld

LD = np.longdouble
OPS = ("gradient", "divergence", "vorticity")
N_GRAD, N_DIV, N_VOR, N_C0 = 1 + 3 + 1 + 1 + 1, ld.N_DIV, 1 + 1 + 1 + 7 + 1 + 1, 1 + 3 + 1
assert (N_GRAD, N_DIV, N_VOR, N_C0) == (7, 13, 12, 5)
NF = {"gradient": (1, 2), "divergence": (2, 1), "vorticity": (2, 1)}      # op -> (fields of in, fields of out)
PLANTS = ("D_swapped", "no_rmetdet", "dudy_sign")                        # errors planted into the vorticity
TRANSPOSITIONS = ("D_transposed", "ij_transposed")                       # errors of index convention, planted into any of the three ops


def steps(op, c0=False):
    return {"gradient": N_GRAD, "divergence": N_DIV, "vorticity": N_VOR}[op] + (N_C0 if c0 else 0)


def geo(o, D, T=np.float64, plant=None):
    """the metric terms at [n][1][4 j][4 i] in type T: 2x2 entries M[a][b] = M(a+1,b+1), Dvv[l][i] = Dvv(i+1,l+1).
    plant "D_transposed": M[a][b] = M(b+1,a+1) for D and Dinv"""
    t = lambda x: np.asarray(x).astype(T)[:, None]
    if plant == "D_transposed":
        m22 = lambda x: [[t(np.asarray(x)[..., a, b]) for b in range(2)] for a in range(2)]
    else:
        m22 = lambda x: [[t(np.asarray(x)[..., b, a]) for b in range(2)] for a in range(2)]
    return dict(D=m22(D), Dinv=m22(o.Dinv), metdet=t(o.metdet), rmetdet=t(o.rmetdet), Dvv=np.asarray(o.Dvv).astype(T), rr=T(ld.RREARTH))


def _ddx(Dvv, x):
    """out[..., j, l] = sum_i Dvv(i,l) x[..., j, i], added in the order i = 1..np from 0.0"""
    out = np.zeros(x.shape, dtype=x.dtype)
    for i in range(4):
        out = out + Dvv[:, i] * x[..., :, i:i + 1]
    return out


def _ddy(Dvv, x):
    """out[..., l, j] = sum_i Dvv(i,l) x[..., i, j]"""
    out = np.zeros(x.shape, dtype=x.dtype)
    for i in range(4):
        out = out + Dvv[:, i][:, None] * x[..., i:i + 1, :]
    return out


def reference(g, op, x, ab=False, plant=None):
    """x[n][nf_in][nk][4][4] of g's type -> op(x)[n][nf_out][nk][4][4] in the source order of operations; ab: every factor and term by
    its absolute value, the difference a sum; plant: one of PLANTS (vorticity)"""
    f = np.abs if ab else (lambda y: y)
    D, Di = ([[f(y) for y in row] for row in g[k]] for k in ("D", "Dinv"))
    met, rmet, Dvv, rr = f(g["metdet"]), f(g["rmetdet"]), f(g["Dvv"]), g["rr"]
    x = f(x)
    if op == "gradient":
        v1, v2 = _ddx(Dvv, x[:, 0]) * rr, _ddy(Dvv, x[:, 0]) * rr
        return np.stack([Di[0][0] * v1 + Di[1][0] * v2, Di[0][1] * v1 + Di[1][1] * v2], axis=1)
    v1, v2 = x[:, 0], x[:, 1]
    if op == "divergence":
        gv1 = met * (Di[0][0] * v1 + Di[0][1] * v2)
        gv2 = met * (Di[1][0] * v1 + Di[1][1] * v2)
        return ((_ddx(Dvv, gv1) + _ddy(Dvv, gv2)) * (rmet * rr))[:, None]
    assert op == "vorticity", op
    if plant == "D_swapped":      # D(1,2) and D(2,1) exchanged: D for D^T
        vco1, vco2 = D[0][0] * v1 + D[0][1] * v2, D[1][0] * v1 + D[1][1] * v2
    else:
        vco1, vco2 = D[0][0] * v1 + D[1][0] * v2, D[0][1] * v1 + D[1][1] * v2
    dvdx, dudy = _ddx(Dvv, vco2), _ddy(Dvv, vco1)
    vor = dvdx + dudy if ab or plant == "dudy_sign" else dvdx - dudy
    return (vor * (rr if plant == "no_rmetdet" else rmet * rr))[:, None]


def reference_fp64(o, D, op, x):
    return reference(geo(o, D), op, np.asarray(x, dtype=np.float64))


def _fma(a, b, c):
    return (np.asarray(a).astype(LD) * np.asarray(b).astype(LD) + np.asarray(c).astype(LD)).astype(np.float64)


def _dx_dev(Dvv, x):
    """at point l of a row: fma(Dvv(4,l), x4, fma(Dvv(3,l), x3, fma(Dvv(2,l), x2, Dvv(1,l) * x1)))"""
    out = Dvv[:, 0] * x[..., :, 0:1]
    for i in (1, 2, 3):
        out = _fma(Dvv[:, i], x[..., :, i:i + 1], out)
    return out


def _dy_dev(Dvv, x):
    """quad_matvec with M(j, m) = Dvv(m, j): rows {j^1, 3 - (j^1)} first, then the lane's own pair"""
    rows = []
    for j in range(4):
        a = j ^ 1
        b = 3 - a
        send = _fma(Dvv[j, b], x[..., b, :], Dvv[j, a] * x[..., a, :])
        rows.append(_fma(Dvv[j, 3 - j], x[..., 3 - j, :], _fma(Dvv[j, j], x[..., j, :], send)))
    return np.stack(rows, axis=-2)


def device_order(o, D, op, x):
    """x[n][nf_in][nk][4][4] fp64 -> op(x) in the order of gradient_sphere_row, divergence_sphere_row and vorticity_row"""
    g = geo(o, D)
    Dm, Di, met, rmet, Dvv, rr = g["D"], g["Dinv"], g["metdet"], g["rmetdet"], g["Dvv"], g["rr"]
    x = np.asarray(x, dtype=np.float64)
    if op == "gradient":
        w1, w2 = rr * _dx_dev(Dvv, x[:, 0]), rr * _dy_dev(Dvv, x[:, 0])
        return np.stack([_fma(Di[1][0], w2, Di[0][0] * w1), _fma(Di[1][1], w2, Di[0][1] * w1)], axis=1)
    v1, v2 = x[:, 0], x[:, 1]
    if op == "divergence":
        gv1 = met * _fma(Di[0][0], v1, Di[0][1] * v2)
        gv2 = met * _fma(Di[1][0], v1, Di[1][1] * v2)
        return ((_dx_dev(Dvv, gv1) + _dy_dev(Dvv, gv2)) * (rmet * rr))[:, None]
    assert op == "vorticity", op
    Dr = [[rr * Dm[a][b] for b in range(2)] for a in range(2)]
    vc1, vc2 = _fma(Dr[1][0], v2, Dr[0][0] * v1), _fma(Dr[1][1], v2, Dr[0][1] * v1)
    return (rmet * (_dx_dev(Dvv, vc2) - _dy_dev(Dvv, vc1)))[:, None]


def make_c0(o, w):
    """w[n][nf][nk][4][4] fp64 -> rspheremp * DSS(spheremp * w) in the oracle's order of addition: dss_view_model.model("average")"""
    return dm.model(o, w, "average")


def _c0_ld(o, w):
    n = w.shape[0]
    sm, rs = np.asarray(o.spheremp).astype(LD)[:, None, None], np.asarray(o.rspheremp).astype(LD)[:, None, None]
    return rs * bm.node_sum(o, (sm * w).reshape(n, -1, 4, 4)).reshape(w.shape)


def longdouble(o, D, op, f, c0=False, plant=None):
    """f[n][nf_in][nk][4][4] fp64 -> (value, A) longdouble [n][nf_out][nk][4][4].  plant: one of PLANTS (vorticity) or of TRANSPOSITIONS:
    "D_transposed" the 2x2 matrices D and Dinv read as (b,a) for (a,b); "ij_transposed" the field read, and the result written, at
    (j,i) for (i,j)"""
    g = geo(o, D, LD)
    x = np.asarray(f, dtype=np.float64).astype(LD)
    A = reference(g, op, x, True)
    if plant == "ij_transposed":
        w = reference(g, op, x.swapaxes(-1, -2), False).swapaxes(-1, -2)
    else:
        w = reference(geo(o, D, LD, plant), op, x, False, plant)
    if c0:
        w, A = _c0_ld(o, w), _c0_ld(o, A)
    return w, A


def ratio(got, ref, A, op, c0=False):
    """|got - ref| / bound at every point (0 where the bound is 0 and the value exact)"""
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    b = ld.bound(steps(op, c0), A)
    return np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))


# ---- fields ----
def random_field(n, nf, nk, seed=0):
    """values of order 30 with noise over the whole mantissa and both signs: [n][nf][nk][4][4]"""
    rng = np.random.default_rng(57 + 1000 * seed + 10 * nk + nf)
    return 30.0 * (0.5 + rng.random((n, nf, nk, 4, 4))) * np.where(rng.random((n, nf, nk, 4, 4)) < 0.4, -1.0, 1.0)


def node_field(o, nf, nk, seed=0):
    """a random field that is continuous: every copy of a node holds the same value (a host's state is; random_field is not)"""
    ids = dm.node_ids(o)
    rng = np.random.default_rng(23 + seed)
    vals = 30.0 * (0.5 + rng.random((ids.max() + 1, nf, nk))) * np.where(rng.random((ids.max() + 1, nf, nk)) < 0.4, -1.0, 1.0)
    return np.ascontiguousarray(np.moveaxis(vals[ids], 1, -1).reshape(o.nelem, nf, nk, 4, 4))


def smooth_field(o, nf, nk):
    """elem_ops_ld's smooth wind or scalar with another phase on every level"""
    if nf == 2:
        return np.stack([ld.smooth_vector(o, k=0.37 * k) for k in range(nk)], axis=2)
    return np.stack([ld.smooth_scalar(o, k=0.37 * k) for k in range(nk)], axis=1)[:, None]


def solid_body(o, U=40.0):
    """(v[n][2][1][4][4], zeta, div): u = U cos(lat), v = 0, for which zeta = 2 U sin(lat) * rrearth and div = 0"""
    la = np.asarray(o.lat)
    v = np.stack([U * np.cos(la), np.zeros(la.shape)], axis=1)[:, :, None]
    return v, (2.0 * U * np.sin(la) * ld.RREARTH)[:, None, None], np.zeros(la.shape)[:, None, None]


def sine_of_latitude(o):
    """(s[n][1][1][4][4], grad[n][2][1][4][4]): s = sin(lat), for which grad = (0, cos(lat) * rrearth)"""
    la = np.asarray(o.lat)
    return np.sin(la)[:, None, None], np.stack([np.zeros(la.shape), np.cos(la) * ld.RREARTH], axis=1)[:, :, None]
