"""The model of tse_biharmonic_view.  Plain numpy and the oracle; no HIP import.

order 1: out = laplace_sphere_wk(f) on every layer (weak, not summed).
order 2: w = laplace_sphere_wk(f);  m = rspheremp * (sum of w over the copies of the node);  out = laplace_sphere_wk(m)
         -- biharmonic_wk_scalar before its final DSS (viscosity_mod.F90:315-344).

longdouble(o, f, order) evaluates the chain in numpy longdouble from the fp64 inputs: elem_ops_ld.laplace_sphere_wk on a longdouble field,
a longdouble node sum over dss_view_model.node_ids (the node identity comes from the mesh's coordinates, not from the DSS tables), and the
same chain on the absolute values of every factor and term, A.

Forward bound elem_ops_ld.bound(N, A).  The whole chain is one sum of products of fp64 inputs, so Higham's gamma_n applies as in
elem_ops_ld.py, n the longest chain of roundings a product term meets on its way to the result:
  order 1   N_LAP = 19                                   (elem_ops_ld.py counts them)
  order 2   N_BIH = 19 + 3 + 1 + 19 = 42                 first Laplacian, up to three additions at a node, * rspheremp, second Laplacian

oracle_fp64(o, f, order) is the oracle's fp64 composition: Oracle.laplace_sphere_wk per slab, dss_view_model.model(mode "weak") =
rspheremp * Oracle.dss, Oracle.laplace_sphere_wk per slab.  `plant` puts one error into the longdouble chain (tests/test_biharmonic_view_cpu.py)."""
import numpy as np

import dss_view_model as dm
import elem_ops_ld as ld

LD = np.longdouble
N_LAP, N_BIH = ld.N_LAP, ld.N_LAP + 3 + 1 + ld.N_LAP
ORDERS = (1, 2)
PLANTS = ("dropped", "average", "no_rspheremp", "unsummed")
TRANSPOSITIONS = ("D_transposed", "ij_transposed")     # errors of index convention, in every Laplacian of either order
assert N_BIH == 42


def steps(order):
    return {1: N_LAP, 2: N_BIH}[order]


class _DinvTransposed:
    """the mesh with Dinv(a,b) read as Dinv(b,a)"""

    def __init__(self, o):
        self._o, self.Dinv = o, np.asarray(o.Dinv).swapaxes(-1, -2)

    def __getattr__(self, name):
        return getattr(self._o, name)


def _lap(o, x, plant=None):
    """x[n][L][4][4] longdouble -> (lap, A) of every layer; plant: one of TRANSPOSITIONS, in the value alone"""
    out = [ld.laplace_sphere_wk(o, x[:, l]) for l in range(x.shape[1])]
    A = np.stack([b for _, b in out], axis=1)
    if plant == "D_transposed":
        return np.stack([ld.laplace_sphere_wk(_DinvTransposed(o), x[:, l])[0] for l in range(x.shape[1])], axis=1), A
    if plant == "ij_transposed":
        return np.stack([ld.laplace_sphere_wk(o, x[:, l].swapaxes(-1, -2))[0].swapaxes(-1, -2) for l in range(x.shape[1])], axis=1), A
    return np.stack([a for a, _ in out], axis=1), A


def node_sum(o, w):
    """w[n][L][4][4] longdouble -> at every point the longdouble sum of w over the copies of its node"""
    ids = dm.node_ids(o).reshape(-1)
    n, L = w.shape[:2]
    x = np.moveaxis(w.reshape(n, L, 16), 1, 2).reshape(n * 16, L)
    tot = np.zeros((ids.max() + 1, L), dtype=LD)
    np.add.at(tot, ids, x)
    return np.moveaxis(tot[ids].reshape(n, 16, L), 2, 1).reshape(w.shape)


def dropped_copy(o):
    """(e0, p0, e1, p1): a point of a node of four elements and another copy of that node -- the contribution the plant "dropped" leaves out"""
    ids = dm.node_ids(o).reshape(-1)
    copies = np.bincount(ids)
    node = int(np.flatnonzero(copies == 4)[0])
    a, b = np.flatnonzero(ids == node)[:2]
    return int(a // 16), int(a % 16), int(b // 16), int(b % 16)


def longdouble(o, f, order, plant=None):
    """f[n][nf][nk][4][4] fp64 -> (value, A) longdouble of the same shape.  plant (order 2): "dropped" one neighbour's contribution missing at
    one point of one element (dropped_copy); "average" spheremp applied before the sum; "no_rspheremp" the sum not scaled; "unsummed" the
    second Laplacian applied to rspheremp * w of the element alone.  plant (either order), one of TRANSPOSITIONS: "D_transposed" Dinv read
    as (b,a) for (a,b); "ij_transposed" every Laplacian reads its field, and writes its result, at (j,i) for (i,j)."""
    f = np.asarray(f, dtype=np.float64)
    n = f.shape[0]
    x = f.reshape(n, -1, 4, 4).astype(LD)
    tp = plant if plant in TRANSPOSITIONS else None
    w, A = _lap(o, x, tp)
    assert plant is None or tp or (plant in PLANTS and order == 2)
    if order == 2:
        rs = np.asarray(o.rspheremp).astype(LD)[:, None]
        sm = np.asarray(o.spheremp).astype(LD)[:, None]
        if plant == "average":
            w, A = sm * w, sm * A
        s, sA = (w, A) if plant == "unsummed" else (node_sum(o, w), node_sum(o, A))
        if plant == "dropped":
            e0, p0, e1, p1 = dropped_copy(o)
            s = s.copy()
            s.reshape(n, -1, 16)[e0, :, p0] -= w.reshape(n, -1, 16)[e1, :, p1]
        if plant != "no_rspheremp":
            s, sA = rs * s, rs * sA
        w, _ = _lap(o, s, tp)
        _, A = _lap(o, sA)
    assert order in ORDERS
    return w.reshape(f.shape), A.reshape(f.shape)


def oracle_fp64(o, f, order):
    """the oracle's fp64 composition, f[n][nf][nk][4][4] -> the same shape"""
    f = np.asarray(f, dtype=np.float64)
    n = f.shape[0]

    def lap(x):
        out = np.empty_like(x)
        for e in range(n):
            for l in range(x.shape[1]):
                out[e, l] = o.laplace_sphere_wk(e, x[e, l])
        return out
    w = lap(np.ascontiguousarray(f.reshape(n, -1, 4, 4)))
    if order == 2:
        w = lap(np.ascontiguousarray(dm.model(o, w[:, None], "weak")[:, 0]))
    return w.reshape(f.shape)


def ratio(got, ref, A, order):
    """|got - ref| / bound at every point (0 where the bound is 0 and the value exact)"""
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    b = ld.bound(steps(order), A)
    return np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))


def random_field(n, nf, nk, seed=0):
    """random values of order 300 with noise over the whole mantissa"""
    rng = np.random.default_rng(77 + 1000 * seed + 100 * nf + nk)
    return 300.0 * (0.5 + rng.random((n, nf, nk, 4, 4))) * np.where(rng.random((n, nf, nk, 4, 4)) < 0.25, -1.0, 1.0)


def smooth_field(o, nf, nk):
    """elem_ops_ld.smooth_scalar with another phase in every layer"""
    return np.stack([np.stack([ld.smooth_scalar(o, k=0.37 * (f * nk + k)) for k in range(nk)], axis=1) for f in range(nf)], axis=1)
