"""The model of tse_dss_view and the layouts its tests lay a field out in.  Plain numpy and the oracle; no HIP import.

Model: out = rspheremp * Oracle.dss(w), w = spheremp * f (mode "average", one stored fp64 product) or w = f (mode "weak"), the layers
flattened to (n, nf * nk, 4, 4).  Oracle.dss adds the contributions of a node in the reference's order of unpacking (edges S, E, N, W,
then the corner) and skips an absent one, where the device adds +0.0: the same bits for every w but -0.0, which the test fields avoid.

Layouts: name -> (strides of e, q, k, j, i in doubles, base, size) for nf fields of nk levels on E elements.  Everything outside the view
is filled with quiet NaNs that carry their own index, so a stray write shows as a changed bit."""
import numpy as np

PAYLOAD = 0x7FF8D55500000000
MODES = ("average", "weak")
LAYOUTS = ("dense", "epad", "lev0", "lev_even", "lev_odd", "ij", "dense_odd8", "lev_odd8")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def model(o, f, mode, weights=None):
    """f[n][nf][nk][4][4] -> rspheremp * DSS(w) in the oracle's order of addition; weights: (spheremp, rspheremp)[n][4][4] in place of the
    mesh's own (node_weights)"""
    f = np.asarray(f, dtype=np.float64)
    n, nf, nk = f.shape[:3]
    sm, rs = weights if weights is not None else (o.spheremp, o.rspheremp)
    sm, rs = np.asarray(sm)[:, None, None], np.asarray(rs)[:, None, None]
    w = sm * f if mode == "average" else f.copy()
    assert mode in MODES
    d = o.dss(np.ascontiguousarray(w.reshape(n, nf * nk, 4, 4))).reshape(f.shape)
    return rs * d


def field(n, nf, nk, seed=0):
    """values of order one with noise over the whole mantissa, no zeros: a changed order of addition cannot tie everywhere"""
    rng = np.random.default_rng(1000 * seed + 100 * nf + nk)
    e = np.arange(n, dtype=np.float64).reshape(n, 1, 1, 1, 1)
    return (1.0 + 0.01 * e) * (0.5 + rng.random((n, nf, nk, 4, 4))) * np.where(rng.random((n, nf, nk, 4, 4)) < 0.25, -1.0, 1.0)


def layout(name, E, nf, nk):
    if name == "dense":              # [e][q][k][j][i]
        s, base, size = [nf * nk * 16, nk * 16, 16, 4, 1], 0, E * nf * nk * 16
    elif name == "epad":             # point-fastest, 6 doubles of padding behind every element
        es = nf * nk * 16 + 6
        s, base, size = [es, nk * 16, 16, 4, 1], 0, E * es
    elif name in ("lev0", "lev_even", "lev_odd", "lev_odd8"):   # [e][q][j][i][k + pad]
        S = {"lev0": nk, "lev_odd8": nk, "lev_even": nk + 2 - nk % 2, "lev_odd": nk + 1 + nk % 2}[name]
        base = 1 if name == "lev_odd8" else 0
        s, size = [nf * 16 * S, 16 * S, 1, 4 * S, S], E * nf * 16 * S + 2 * base
    elif name == "ij":               # [e][q][k][i][j] behind an odd offset: any strides
        es = nf * nk * 16 + 5
        s, base, size = [es, nk * 16, 16, 1, 4], 3, E * es + 3
    elif name == "dense_odd8":       # point-fastest, the base 8 but not 16 bytes aligned
        s, base, size = [nf * nk * 16, nk * 16, 16, 4, 1], 1, E * nf * nk * 16 + 2
    else:
        raise ValueError(name)
    return s, base, size


def expected_path(name, nk, nlev):
    """what tse_dss_view_plan must report: 0 point-fastest, 1 level-fastest (nk == nlev only), 2 generic"""
    if name in ("dense", "epad", "dense_odd8"):
        return 0
    if name == "ij":
        return 2
    if nk == 1 and name in ("lev0", "lev_odd8"):   # rows of one level at pitch 1: stride i = 1, j = 4 -- point-fastest
        return 0
    return 1 if nk == nlev else 2


def footprint(name, E, nf, nk):
    """[lo, hi) in doubles relative to the view's pointer (every stride of these layouts is positive: the last index tuple ends it)"""
    s, _, _ = layout(name, E, nf, nk)
    ext = (E, nf, nk, 4, 4)
    return 0, sum(st * (n - 1) for st, n in zip(s, ext)) + 1


def index(s, base, shape):
    ix = np.full(shape, base, dtype=np.int64)
    for ax, n in enumerate(shape):
        sh = [1] * len(shape); sh[ax] = n
        ix = ix + s[ax] * np.arange(n, dtype=np.int64).reshape(sh)
    return ix


class Strided:
    """a dense field f[E][nf][nk][4][4] laid into a NaN-filled host buffer as a layout names it"""

    def __init__(self, data, name):
        data = np.asarray(data, dtype=np.float64)
        E, nf, nk = data.shape[:3]
        self.s, self.base, size = layout(name, E, nf, nk)
        self.ix = index(self.s, self.base, data.shape)
        assert np.unique(self.ix).size == self.ix.size and self.ix.min() >= 0 and self.ix.max() < size, name
        self.host = (np.uint64(PAYLOAD) + np.arange(size, dtype=np.uint64)).view(np.float64)
        self.host[self.ix] = data
        self.shape, self.name = data.shape, name
        self.gap = np.ones(size, dtype=bool); self.gap[self.ix.ravel()] = False

    def read(self, buf):
        """(the field, whether every gap kept its bits) of a buffer that came back from the device"""
        buf = np.asarray(buf)
        return buf[self.ix], np.array_equal(bits(buf[self.gap]), bits(self.host[self.gap]))


def node_ids(o):
    """[n][16] the node every GLL point sits on, read from the mesh's coordinates (not from the DSS tables)"""
    lat, lon = np.asarray(o.lat).reshape(-1), np.asarray(o.lon).reshape(-1)
    xyz = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=1)
    key = np.round(xyz * 1e9).astype(np.int64)
    _, ids = np.unique(key, axis=0, return_inverse=True)
    return np.asarray(ids).reshape(o.nelem, 16)


def continuous(o, x, copies=(2, 3, 4)):
    """(every copy of a shared node holds the same bits in every layer of x[n][...][4][4], the number of (node, layer) pairs that do not,
    the number looked at), over the nodes with one of the given numbers of copies"""
    ids = node_ids(o).reshape(-1)
    b = bits(np.moveaxis(np.asarray(x).reshape(o.nelem, -1, 16), 1, 2).reshape(o.nelem * 16, -1))
    order = np.argsort(ids, kind="stable")
    ids, b = ids[order], b[order]
    first = np.r_[True, ids[1:] != ids[:-1]]
    lead = np.maximum.accumulate(np.where(first, np.arange(ids.size), 0))
    take = np.isin(np.bincount(ids)[ids], copies)
    differs = np.zeros((ids.max() + 1, b.shape[1]), dtype=bool)
    np.logical_or.at(differs, ids[take], (b != b[lead])[take])
    nbad = int(differs.sum())
    return nbad == 0, nbad, int(np.isin(np.bincount(ids), copies).sum()) * b.shape[1]


# ---- continuity in every bit ----
# The reference's DSS adds the contributions of a node in an order of each element's own, so where three or four elements meet the copies
# of a node agree only as far as fp64 addition is associative, and rspheremp = 1 / DSS(spheremp) differs between them in the same way
# (DESIGN.md section 3 has the figures).  Equal bits at EVERY node are a property of the connectivity -- every copy receives the same set
# of contributions -- and show on inputs whose arithmetic does not depend on the order: every element its own small integer (all partial
# sums exact), and weights that are one per node.
def own_values(n, nf=1, nk=2):
    """every element its own value, every layer another: integers below 2^20"""
    e = 1.0 + np.arange(n, dtype=np.float64).reshape(n, 1, 1, 1, 1)
    layer = np.arange(nf * nk, dtype=np.float64).reshape(1, nf, nk, 1, 1)
    return np.broadcast_to(e + 1000.0 * layer, (n, nf, nk, 4, 4)).copy()


def node_weights(o):
    """(spheremp, rspheremp)[n][4][4] of a mass matrix that is one per node: spheremp = 1, rspheremp = fl(1 / copies of the node)"""
    ids = node_ids(o)
    copies = np.bincount(ids.reshape(-1))[ids].astype(np.float64)
    return np.ones((o.nelem, 4, 4)), (1.0 / copies).reshape(o.nelem, 4, 4)


def node_sums(o, f):
    """f[n][...][4][4] -> at every point the sum of f over the copies of its node, from the mesh's coordinates alone (exact for own_values)"""
    ids = node_ids(o).reshape(-1)
    x = np.moveaxis(np.asarray(f).reshape(o.nelem, -1, 16), 1, 2).reshape(o.nelem * 16, -1)
    tot = np.zeros((ids.max() + 1, x.shape[1]))
    np.add.at(tot, ids, x)
    return np.moveaxis(tot[ids].reshape(o.nelem, 16, -1), 2, 1).reshape(np.asarray(f).shape)
