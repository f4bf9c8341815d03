"""The model of tse_vlaplace_view.  Plain numpy; no HIP import.

The operator is the reference's vlaplace_sphere_wk_contra (derivative_mod.F90:2545-2591), constant coefficient:
    div = divergence_sphere(v)                (:2364-2414)      vor = vorticity_sphere(v)               (:2250-2301)
    lap = gradient_sphere_wk_testcov(nu_ratio * div) (:1765-1828) - curl_sphere_wk_testcov(vor) (:1703-1762)
    lap(:,:,c) += 2 * spheremp * v(:,:,c) * rrearth**2
order 1: out = lap(f) on every level (weak, not summed).
order 2: w = lap(f);  m_c = rspheremp * (sum of w_c over the copies of the node);  out = lap(m) -- the wind's line of biharmonic_wk_dp3d
         (viscosity_mod.F90:177-286) before its final DSS, nu_ratio in both Laplacians.

_vlap restates the four routines in their source order of operations (the serial sums of the loops, the products left to right) for any
numpy float type: reference_fp64 runs it in fp64, longdouble in np.longdouble from the fp64 inputs together with the same chain on the
absolute values of every factor and term, A -- both sides of every difference (dvdx - dudy, grad - curl) and the 2*spheremp*v*rr^2 term
enter A with a plus sign, because the operator cancels heavily and a bound made from the result would be far too small.  The node sum of
order 2 is biharmonic_model.node_sum (the node identity comes from the mesh's coordinates).

Forward bound elem_ops_ld.bound(N, A), as elem_ops_ld.py derives it: n is the longest chain of roundings that multiplies one product term
on its way to the result, over the reference's association and the device's folded tables (csrc/tse_device.h: vlaplace_row) alike.
  the reference, along v -> div -> grad -> lap (the longest: vor has the same 8-term sum but one product less, curl two products less):
    divergence_sphere                                                      13   (N_DIV, elem_ops_ld.py)
    nu_ratio * div                                                          1
    mp * metinv * metdet * s * Dvv                                          4
    the sum of the x- and the y-term                                        1
    * rrearth                                                               1
    the accumulation over j = 1..np into dscontra                           4
    D * dscontra + D * dscontra (product, sum)                              2
    grad - curl                                                             1
    + 2 * spheremp * v * rrearth**2                                         1   -> 28
  the device, the same path:
    table gDi = (rrearth * metdet) * Dinv                                   2
    gDi * v1, fma with gDi * v2                                             2
    Dvv * gv: a chain of one product and three fmas (dx), or quad_matvec's
    four roundings (dy); dx + dy                                            4 + 1
    table mr = mp * rmetdet; mr * (dx + dy); nu_ratio *                     1 + 1 + 1
    Dvv * md: one product and three fmas (X), quad_matvec (Y)               4
    table G = -(Dr * mg + Dr * mg), Dr = rrearth * D, mg = metdet * metinv  4
    G * X, then four fmas (G * Y, Dr * Yv, -Dr * Xv, s2 * v)                5   -> 25
  (device, v -> vor -> curl -> lap: 1 + 2 + 5 + 2 + 4 + 1 + 4 = 19; the term s2 * v: s2 = (2 * spheremp) * (rrearth * rrearth) 2, fma 1)
  N_VLAP = 28.   order 2: N_VBIH = 28 + 3 (additions at a node) + 1 (* rspheremp) + 28 = 60.
The counts are derived from the two codes, not fitted to what the device returns."""
import numpy as np

import biharmonic_model as bm
import dss_view_model as dm
import elem_ops_ld as ld

LD = np.longdouble
N_VLAP = ld.N_DIV + 1 + 4 + 1 + 1 + 4 + 2 + 1 + 1
N_VBIH = N_VLAP + 3 + 1 + N_VLAP
assert (N_VLAP, N_VBIH) == (28, 60)
ORDERS = (1, 2)
PLANTS1 = ("no_rr", "curl_added", "D_for_DT", "nu_on_vor")     # in the operator
PLANTS2 = bm.PLANTS                                            # in the node sum of order 2: dropped, average, no_rspheremp, unsummed
TRANSPOSITIONS = ("D_transposed", "ij_transposed")             # errors of index convention, in every Laplacian of either order


def steps(order):
    return {1: N_VLAP, 2: N_VBIH}[order]


def host_fields(o):
    """(D, metinv, mp) of the oracle's mesh as a host would hand them to tse_vector_setup"""
    from transport_se_amd import cube_mesh as cm
    D = np.array(o.D)
    return D, cm.metinv(D), np.array(o.mp)


def _geo(o, D, metinv, mp, T, plant=None):
    """everything in Fortran's index order [n][i][j] and type T: 2x2 entries M[a][b] = M(a+1,b+1), Dvv[i][l] = Dvv(i+1,l+1).
    plant "D_transposed": M[a][b] = M(b+1,a+1) for D and Dinv (and metinv, which is symmetric)"""
    t = lambda x: np.asarray(x).astype(T).transpose(0, 2, 1)
    if plant == "D_transposed":
        m22 = lambda x: [[t(np.asarray(x)[..., a, b]) for b in range(2)] for a in range(2)]
    else:
        m22 = lambda x: [[t(np.asarray(x)[..., b, a]) for b in range(2)] for a in range(2)]
    return dict(D=m22(D), Dinv=m22(o.Dinv), metinv=m22(metinv), mp=t(mp), metdet=t(o.metdet), rmetdet=t(o.rmetdet), spheremp=t(o.spheremp),
                Dvv=np.asarray(o.Dvv).astype(T).T, rr=T(ld.RREARTH))


def _vlap(g, v, nu_ratio, ab=False, plant=None):
    """v[n][i][j][2] of g's type -> vlaplace_sphere_wk_contra in the source order of operations; ab: every factor and term by its
    absolute value, every difference a sum"""
    f = np.abs if ab else (lambda x: x)
    sub = (lambda a, b: a + b) if ab else (lambda a, b: a - b)
    T = g["rr"].__class__
    D, Di, mi = ([[f(x) for x in row] for row in g[k]] for k in ("D", "Dinv", "metinv"))
    mp, met, rmet, sph, Dvv, rr = f(g["mp"]), f(g["metdet"]), f(g["rmetdet"]), f(g["spheremp"]), f(g["Dvv"]), g["rr"]
    v1, v2 = f(v[..., 0]), f(v[..., 1])
    nu = T(abs(nu_ratio) if ab else nu_ratio)
    zero = np.zeros(v1.shape, dtype=v1.dtype)
    # divergence_sphere
    gv1 = met * (Di[0][0] * v1 + Di[0][1] * v2)
    gv2 = met * (Di[1][0] * v1 + Di[1][1] * v2)
    dudx, vvtemp = zero, zero
    for i in range(4):
        dudx = dudx + Dvv[i, :][None, :, None] * gv1[:, i, :][:, None, :]          # div(l,j)    += Dvv(i,l) * gv(i,j,1)
        vvtemp = vvtemp + Dvv[i, :][None, None, :] * gv2[:, :, i][:, :, None]      # vvtemp(j,l) += Dvv(i,l) * gv(j,i,2)
    div = (dudx + vvtemp) * (rmet * rr)
    # vorticity_sphere (covariant components: D^T v)
    if plant == "D_for_DT":
        vco1, vco2 = D[0][0] * v1 + D[0][1] * v2, D[1][0] * v1 + D[1][1] * v2
    else:
        vco1, vco2 = D[0][0] * v1 + D[1][0] * v2, D[0][1] * v1 + D[1][1] * v2
    dvdx, vtemp = zero, zero
    for i in range(4):
        dvdx = dvdx + Dvv[i, :][None, :, None] * vco2[:, i, :][:, None, :]         # vort(l,j)  += Dvv(i,l) * vco(i,j,2)
        vtemp = vtemp + Dvv[i, :][None, None, :] * vco1[:, :, i][:, :, None]       # vtemp(j,l) += Dvv(i,l) * vco(j,i,1)
    vor = sub(dvdx, vtemp) * (rmet * rr)
    if plant == "nu_on_vor":
        vor = nu * vor
    else:
        div = nu * div
    # gradient_sphere_wk_testcov(div), curl_sphere_wk_testcov(vor): dscontra(m,n,:), the sums over j
    gc1, gc2, cc1, cc2 = zero, zero, zero, zero
    for j in range(4):
        mx, my = mp[:, j, :][:, None, :], mp[:, :, j][:, :, None]                   # mp(j,n), mp(m,j)
        dx, dy = Dvv[:, j][None, :, None], Dvv[:, j][None, None, :]                 # Dvv(m,j), Dvv(n,j)
        sx, sy = div[:, j, :][:, None, :], div[:, :, j][:, :, None]                 # s(j,n), s(m,j)
        gc1 = sub(gc1, ((mx * mi[0][0] * met * sx * dx) + (my * mi[1][0] * met * sy * dy)) * rr)
        gc2 = sub(gc2, ((mx * mi[0][1] * met * sx * dx) + (my * mi[1][1] * met * sy * dy)) * rr)
        wx, wy = vor[:, j, :][:, None, :], vor[:, :, j][:, :, None]
        cc1 = sub(cc1, (my * wy * dy) * rr)
        cc2 = cc2 + (mx * wx * dx) * rr
    out = []
    for c, vc in ((0, v1), (1, v2)):
        grad = D[c][0] * gc1 + D[c][1] * gc2
        curl = D[c][0] * cc1 + D[c][1] * cc2
        lap = grad + curl if plant == "curl_added" else sub(grad, curl)
        if plant != "no_rr":
            lap = lap + 2 * sph * vc * (rr ** 2)
        out.append(lap)
    return np.stack(out, axis=-1)


def _levels(g, x, nu_ratio, ab=False, plant=None):
    """x[n][2][nk][4 j][4 i] -> the operator on every level, the same shape"""
    out = np.empty(x.shape, dtype=x.dtype)
    for k in range(x.shape[2]):
        r = _vlap(g, x[:, :, k].transpose(0, 3, 2, 1), nu_ratio, ab, plant)       # [n][c][j][i] -> [n][i][j][c]
        out[:, :, k] = r.transpose(0, 3, 2, 1)
    return out


def reference_fp64(o, D, metinv, mp, v, nu_ratio=1.0):
    """v[n][2][4][4] fp64 -> the four reference routines in their source order of operations, in fp64"""
    g = _geo(o, D, metinv, mp, np.float64)
    return _levels(g, np.asarray(v, dtype=np.float64)[:, :, None], nu_ratio)[:, :, 0]


def reference_chain_fp64(o, D, metinv, mp, f, order, nu_ratio=1.0):
    """f[n][2][nk][4][4] -> order 1 or 2 in fp64: reference_fp64, dss_view_model.model(mode "weak") = rspheremp * Oracle.dss, reference_fp64"""
    g = _geo(o, D, metinv, mp, np.float64)
    w = _levels(g, np.asarray(f, dtype=np.float64), nu_ratio)
    if order == 2:
        w = _levels(g, dm.model(o, w, "weak"), nu_ratio)
    assert order in ORDERS
    return w


def longdouble(o, D, metinv, mp, f, order, nu_ratio=1.0, plant=None):
    """f[n][2][nk][4][4] fp64 -> (value, A) longdouble of the same shape.  plant: one of PLANTS1 (an error in the operator, either order) or
    of PLANTS2 (biharmonic_model's errors in the node sum, order 2) or of TRANSPOSITIONS: "D_transposed" the 2x2 matrices read as (b,a) for
    (a,b); "ij_transposed" every Laplacian reads its field, and writes its result, at (j,i) for (i,j)."""
    assert order in ORDERS and (plant is None or plant in PLANTS1 + TRANSPOSITIONS or (plant in PLANTS2 and order == 2)), (order, plant)
    g = _geo(o, D, metinv, mp, LD)
    f = np.asarray(f, dtype=np.float64)
    n, nk = f.shape[0], f.shape[2]
    x = f.astype(LD)
    p1 = plant if plant in PLANTS1 else None
    gp = _geo(o, D, metinv, mp, LD, plant)
    if plant == "ij_transposed":
        planted = lambda y: _levels(g, y.swapaxes(-1, -2), nu_ratio).swapaxes(-1, -2)
    else:
        planted = lambda y: _levels(gp, y, nu_ratio, False, p1)
    w, A = planted(x), _levels(g, x, nu_ratio, True)
    if order == 2:
        rs = np.asarray(o.rspheremp).astype(LD)[:, None, None]
        sm = np.asarray(o.spheremp).astype(LD)[:, None, None]
        if plant == "average":
            w, A = sm * w, sm * A
        flat = lambda y: y.reshape(n, 2 * nk, 4, 4)
        s, sA = (w, A) if plant == "unsummed" else (bm.node_sum(o, flat(w)).reshape(w.shape), bm.node_sum(o, flat(A)).reshape(A.shape))
        if plant == "dropped":
            e0, p0, e1, p1_ = bm.dropped_copy(o)
            s = s.copy()
            s.reshape(n, -1, 16)[e0, :, p0] -= w.reshape(n, -1, 16)[e1, :, p1_]
        if plant != "no_rspheremp":
            s, sA = rs * s, rs * sA
        w, A = planted(s), _levels(g, sA, nu_ratio, True)
    return w, A


def ratio(got, ref, A, order):
    """|got - ref| / bound at every point (0 where the bound is 0 and the value exact)"""
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    b = ld.bound(steps(order), A)
    return np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))


def random_field(n, nk, seed=0):
    """random wind components of order 30 with noise over the whole mantissa: [n][2][nk][4][4]"""
    rng = np.random.default_rng(91 + 1000 * seed + nk)
    return 30.0 * (0.5 + rng.random((n, 2, nk, 4, 4))) * np.where(rng.random((n, 2, nk, 4, 4)) < 0.4, -1.0, 1.0)


def smooth_field(o, nk):
    """elem_ops_ld.smooth_vector with another phase on every level"""
    return np.stack([ld.smooth_vector(o, k=0.37 * k) for k in range(nk)], axis=2)


# ---- the operator against the sphere's own eigenfunctions ----
def harmonic_fields(o):
    """name -> (v[n][2][4][4], eigenvalue of rspheremp * DSS(lap) / rrearth^2 for nu_ratio 1, whether the field is divergent)"""
    la, lo = np.asarray(o.lat), np.asarray(o.lon)
    z = np.zeros(la.shape)
    c, s = np.cos(la), np.sin(la)
    return {
        "l1 rigid rotation": (np.stack([c, z], axis=1), 0.0, False),
        "l2 rotational": (np.stack([s * c, z], axis=1), -4.0, False),
        "l2 divergent": (np.stack([z, s * c], axis=1), -4.0, True),
        # k x grad(psi), psi = cos^2(lat) sin(lat) cos(2 lon):  (-dpsi/dlat, dpsi/dlon / cos(lat))
        "l3 rotational": (np.stack([-(c ** 3 - 2.0 * c * s * s) * np.cos(2.0 * lo), -2.0 * c * s * np.sin(2.0 * lo)], axis=1), -10.0, False),
    }


def strong_laplacian(o, D, metinv, mp, v, nu_ratio=1.0, plant=None):
    """rspheremp * DSS(vlaplace(v)) / rrearth^2 in fp64 (the node sum from the mesh's coordinates): v[n][2][4][4] -> the same shape"""
    g = _geo(o, D, metinv, mp, np.float64)
    w = _levels(g, np.asarray(v, dtype=np.float64)[:, :, None], nu_ratio, False, plant)[:, :, 0]
    return np.asarray(o.rspheremp)[:, None] * dm.node_sums(o, w) / ld.RREARTH ** 2
