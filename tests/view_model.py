"""numpy model of the strided device views (tse_view_put / tse_view_get; csrc/tse_views.cpp): which index tuple of a field sits at which
offset of a flat buffer.  Brute force on purpose -- every address is enumerated -- so that the library's closed forms (footprint,
overlap test, path) have something independent to be held to."""
import numpy as np

AXES = "eqkji"   # the order of tse_view.stride: element, q (tracer / wind component), level, j, i

# field: (has a q axis: None | "q" (qsize) | 2, level extent of a put view, of a get view) with "n" = nlev, "p" = nlev + 1, 0 = no level
# axis, None = not served in that direction
FIELDS = {
    "qdp": ("q", "n", "n"), "vn0": (2, "n", None), "dp": (None, "n", None), "eta_dot_dpdn": (None, "p", "n"), "omega_p": (None, "n", "n"),
    "divdp": (None, "n", "n"), "divdp_proj": (None, "n", "n"), "dp3d": (None, None, "n"), "ps_v": (None, None, 0), "q": ("q", None, "n"),
    "lnps": (None, None, 0),
}
PUT_FIELDS = tuple(f for f, d in FIELDS.items() if d[1] is not None)
GET_FIELDS = tuple(f for f, d in FIELDS.items() if d[2] is not None)


def extents(field, nelemd, qsize, nlev, for_get=False):
    """extents of (element, q, level, j, i); 1 for an axis the field does not have"""
    qk, lp, lg = FIELDS[field]
    lev = lg if for_get else lp
    assert lev is not None, (field, for_get)
    return (nelemd, qsize if qk == "q" else (qk or 1), {"n": nlev, "p": nlev + 1, 0: 1}[lev], 4, 4)


def has_axes(field, for_get=False):
    qk, lp, lg = FIELDS[field]
    return (True, qk is not None, (lg if for_get else lp) != 0, True, True)


def offsets(field, nelemd, qsize, nlev, strides, for_get=False):
    """int64 array of shape extents(...): the offset (doubles, relative to the view's pointer) of every index tuple"""
    ext = extents(field, nelemd, qsize, nlev, for_get)
    off = np.zeros(ext, dtype=np.int64)
    for a in range(5):
        shape = [1] * 5; shape[a] = ext[a]
        off = off + (np.arange(ext[a], dtype=np.int64) * int(strides[a])).reshape(shape)
    return off


def squeeze(field, x, for_get=False):
    """drop the axes the field does not have: [e][q][k][j][i] -> the field's own array"""
    has = has_axes(field, for_get)
    return x.reshape([n for n, h in zip(x.shape, has) if h])


def scatter(field, logical, nelemd, qsize, nlev, strides, buf, base=0, for_get=False):
    """lay `logical` ([e][q][k][j][i] with the field's axes only) into the flat float64 buffer `buf` as the view (base, strides) names it"""
    off = offsets(field, nelemd, qsize, nlev, strides, for_get) + base
    assert off.min() >= 0 and off.max() < buf.size
    buf[off.reshape(-1)] = np.asarray(logical, dtype=np.float64).reshape(-1)
    return buf


def gather(field, nelemd, qsize, nlev, strides, buf, base=0, for_get=False):
    """read the field out of the flat buffer: the field's own array"""
    off = offsets(field, nelemd, qsize, nlev, strides, for_get) + base
    assert off.min() >= 0 and off.max() < buf.size
    return squeeze(field, buf[off], for_get)


def nested_strides(ext, order, pads=None):
    """strides of a view built by nesting: `order` lists the axes from fastest to slowest, each axis steps over the whole extent of the
    ones before it plus pads[axis] spare doubles"""
    s, acc = [0] * 5, 1
    for a in order:
        s[a] = acc
        acc = acc * ext[a] + (pads or {}).get(a, 0)
    return s, acc


def expected_path(field, strides, nlev, for_get=False):
    """the path rule of include/transport_se_hip.h, restated"""
    ext = extents(field, 1, 1, nlev, for_get)
    se, sq, sk, sj, si = strides
    if si == 1 and sj == 4:
        return 0
    if has_axes(field, for_get)[2] and sk == 1 and si >= ext[2] and sj == 4 * si:
        return 1
    return 2
