"""Model of tse_hypervis_view: one hyperviscosity sub-step of nf scalar fields and the wind.  Plain numpy and the oracle; no HIP import.

It composes the models of the entries the call chains -- biharmonic_model (order 2), vlaplace_model (order 2), dss_view_model ("weak") --
with the two operations the call adds, one product with the field's factor and one addition:
    b = biharmonic(x);  t = coef * b;  d = rspheremp * DSS(t);  x <- x + d
fp64(...)        the fp64 composition: (s + ds, v + dv, ds, dv)
longdouble(...)  the same chain in longdouble with the bound's magnitude A carried along: ((value, A) of s + ds, (value, A) of v + dv)
continue_ld(...) the steps behind the biharmonic alone, from any (b, A_b): what carries the reference's own biharmonic to the end
N_AFTER          the roundings those steps add to the biharmonic's count: the product, three additions at a node, one rspheremp, the
                 final addition
plant: "coef_shifted" coef[f] applied to scalar field f + 1 (cyclically), "wind_coef" the wind's factor applied to the scalars,
"no_rspheremp" the final rspheremp dropped.
"""
import numpy as np

import biharmonic_model as bm
import dss_view_model as dm
import fieldops_ref as fr
import vlaplace_model as vm

LD = np.longdouble
N_AFTER = 1 + (fr.N_DSS - 1) + 1
PLANTS = ("coef_shifted", "wind_coef", "no_rspheremp")


def steps(wind):
    """the rounding count of the whole chain for a scalar field (wind False) or the wind"""
    return (vm.steps(2) if wind else bm.steps(2)) + N_AFTER


def _factors(coef, nf, wind, plant=None):
    """the factor of every q slot, [nf or 2] broadcastable over [n][q][k][4][4]"""
    c = np.asarray(coef, dtype=np.float64)
    assert c.size == nf + 1
    if wind:
        return np.full(2, c[nf]).reshape(1, 2, 1, 1, 1)
    cs = c[:nf]
    if plant == "coef_shifted":
        cs = np.roll(cs, 1)
    if plant == "wind_coef":
        cs = np.full(nf, c[nf])
    return cs.reshape(1, nf, 1, 1, 1)


def fp64(o, geo, s, v, coef, nu_ratio=1.0):
    """s[n][nf][nk][4][4] or None, v[n][2][nk][4][4] or None, geo = (D, metinv, mp) -> (s + ds, v + dv, ds, dv), None for an absent half"""
    nf = 0 if s is None else s.shape[1]
    out = {}
    for key, x in (("s", s), ("v", v)):
        if x is None:
            out[key] = (None, None)
            continue
        b = vm.reference_chain_fp64(o, geo[0], geo[1], geo[2], x, 2, nu_ratio) if key == "v" else bm.oracle_fp64(o, x, 2)
        t = _factors(coef, nf, key == "v") * b
        d = dm.model(o, t, "weak")
        out[key] = (x + d, d)
    return out["s"][0], out["v"][0], out["s"][1], out["v"][1]


def continue_ld(o, x, b, A, factors, plant=None):
    """(value, A) of x + rspheremp * node_sum(factors * b) in longdouble, from the biharmonic b and its magnitude A"""
    n = x.shape[0]
    f = factors.astype(LD)
    t, At = f * b.astype(LD), np.abs(f) * A.astype(LD)
    rs = np.ones(1, dtype=LD) if plant == "no_rspheremp" else np.asarray(o.rspheremp).astype(LD)[:, None, None]
    d = rs * bm.node_sum(o, t.reshape(n, -1, 4, 4)).reshape(x.shape)
    Ad = np.abs(rs) * bm.node_sum(o, At.reshape(n, -1, 4, 4)).reshape(x.shape)
    return x.astype(LD) + d, np.abs(x).astype(LD) + Ad


def longdouble(o, geo, s, v, coef, nu_ratio=1.0, plant=None):
    """((value, A) of the new s, (value, A) of the new v), None for an absent half"""
    nf = 0 if s is None else s.shape[1]
    out = []
    for key, x in (("s", s), ("v", v)):
        if x is None:
            out.append(None)
            continue
        b, A = vm.longdouble(o, geo[0], geo[1], geo[2], x, 2, nu_ratio) if key == "v" else bm.longdouble(o, x, 2)
        out.append(continue_ld(o, x, b, A, _factors(coef, nf, key == "v", plant), plant))
    return tuple(out)


def ratio(got, ref, A, wind):
    """|got - ref| / bound(steps, A) at every point"""
    return fr.ratio(got, ref, A, steps(wind))
