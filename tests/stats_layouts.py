"""The layouts of tests/dss_view_model.py and two more for tse_stats_view: point-fastest views that may not move 16 bytes per lane because
of ONE ODD STRIDE, the base being 16-byte aligned.  Plain numpy; no HIP import.
  dense_odd_e   [e][q][k][j][i] with 5 doubles of padding behind every element: an odd element stride
  dense_odd_k   [e][q][k][17]: every level's 16 points followed by one double of padding, an odd level stride (q and element strides even
                where nf * nk is: the level stride alone decides)"""
import numpy as np

import dss_view_model as dm

ODD = ("dense_odd_e", "dense_odd_k")


def layout(name, E, nf, nk):
    if name == "dense_odd_e":
        es = nf * nk * 16 + 5
        return [es, nk * 16, 16, 4, 1], 0, E * es
    if name == "dense_odd_k":
        qs = nk * 17 + nk % 2                      # (even, so that the level stride is the only odd one)
        es = nf * qs
        return [es, qs, 17, 4, 1], 0, E * es
    return dm.layout(name, E, nf, nk)


def expected_path(name, nk, nlev):
    return 0 if name in ODD else dm.expected_path(name, nk, nlev)


def footprint(name, E, nf, nk):
    s, _, _ = layout(name, E, nf, nk)
    return 0, sum(st * (n - 1) for st, n in zip(s, (E, nf, nk, 4, 4))) + 1


class Strided(dm.Strided):
    """dss_view_model.Strided over these layouts"""

    def __init__(self, data, name):
        data = np.asarray(data, dtype=np.float64)
        E, nf, nk = data.shape[:3]
        self.s, self.base, size = layout(name, E, nf, nk)
        self.ix = dm.index(self.s, self.base, data.shape)
        assert np.unique(self.ix).size == self.ix.size and self.ix.min() >= 0 and self.ix.max() < size, name
        self.host = (np.uint64(dm.PAYLOAD) + np.arange(size, dtype=np.uint64)).view(np.float64)
        self.host[self.ix] = data
        self.shape, self.name = data.shape, name
        self.gap = np.ones(size, dtype=bool); self.gap[self.ix.ravel()] = False
