"""The reference's own field operators as a referee of the view models and the view entries.  Plain numpy and the oracle; no HIP import.

tests/golden/ref_ne2_fieldops.npz holds what the reference's Fortran (derivative_mod.F90, viscosity_mod.F90) returned on every element of
ne2 and three levels of oracle/ref/fieldops_fill.F90's inputs: oracle/ref/ref_harness.F90's dump_fieldops, stored by
oracle/ref/make_golden.py --fieldops.  The geometry is the reference's as well: ref_ne2_static.npz, and metinv from the fixture.

mesh(st, fx)   a pyoracle.Oracle of ne2 whose metric arrays are overwritten with the reference's (the models read them as attributes, and
               its C operators read the same memory), in the reference's element order -- which is the oracle's: its node sum is checked
               against the node identity the reference's lat/lon give before anything relies on it.
CASES          name -> Case: the fixture's output key, the rounding count N of the model's bound, the model's longdouble chain (value, A),
               the model's fp64 restatement, the view call that computes it on the device, and the plants the model carries for it.
"""
import collections
import functools

import numpy as np

import biharmonic_model as bm
import dss_view_model as dm
import elem_ops_ld as ld
import sphere_ops_model as sm
import vlaplace_model as vm

LD = np.longdouble
N_DSS = 1 + 3 + 1          # one weight, three additions at a node, one rspheremp
GEOMETRY = ("lat", "lon", "D", "Dinv", "metdet", "rmetdet", "mp", "spheremp", "rspheremp")

Case = collections.namedtuple("Case", "out N src ld fp64 plants call")


def mesh(st):
    """the oracle of ne2 carrying the reference's arrays (ref_ne2_static.npz)"""
    import pyoracle as po
    o = po.Oracle(2, 1)
    assert o.nelem == st["lat"].shape[0] and np.array_equal(st["gid"], np.arange(1, o.nelem + 1))
    assert np.abs(o.Dvv - st["Dvv"]).max() <= 1e-15 * np.abs(st["Dvv"]).max()      # (the same index order, before it is overwritten)
    for k in GEOMETRY:
        assert np.abs(getattr(o, k) - st[k]).max() <= 1e-14 * np.abs(st[k]).max(), k   # the same element order: ulps, not another mesh
        getattr(o, k)[...] = st[k]
    o.Dvv[...] = st["Dvv"]
    # the oracle's node sum adds the copies of a node that the reference's coordinates name (integers: exact in any order)
    own = dm.own_values(o.nelem, 1, 2)
    assert np.array_equal(o.dss(own.reshape(o.nelem, 2, 4, 4).copy()).reshape(own.shape), dm.node_sums(o, own))
    return o


def _dss_ld(o, f, mode):
    """(value, A) of rspheremp * (sum over the node of w), w = spheremp * f ("average") or f ("weak"), in longdouble"""
    n = f.shape[0]
    smp, rs = np.asarray(o.spheremp).astype(LD)[:, None, None], np.asarray(o.rspheremp).astype(LD)[:, None, None]
    out = []
    for x in (f.astype(LD), np.abs(f).astype(LD)):
        w = smp * x if mode == "average" else x
        out.append(rs * bm.node_sum(o, w.reshape(n, -1, 4, 4)).reshape(f.shape))
    return out[0], out[1]


def cases(fx):
    """name -> Case for the fixture fx (nu_ratio read from it).  ld(o, geo, f, plant), fp64(o, geo, f), call(hip, in, out, stream) with
    geo = (D, metinv, mp) of the reference"""
    C = collections.OrderedDict()
    for key, mode in (("dss_average", "average"), ("dss_weak", "weak")):
        C[key] = Case(key, N_DSS, "s", functools.partial(lambda o, g, f, plant, mode: _dss_ld(o, f, mode), mode=mode),
                      functools.partial(lambda o, g, f, mode: dm.model(o, f, mode), mode=mode), (),
                      ("dss_view", dict(mode=mode)))
    sph = (("grad", "gradient", "s", False), ("grad_cont", "gradient", "dss_average", False), ("div", "divergence", "v", False),
           ("vor", "vorticity", "v", False), ("div_c0", "divergence", "v", True), ("vor_c0", "vorticity", "v", True),
           ("grad_c0", "gradient", "s", True), ("grad_cont_c0", "gradient", "dss_average", True),
           ("zeta_c0", "vorticity", "v", True), ("divergence_c0", "divergence", "v", True))
    for key, op, src, c0 in sph:
        plants = (sm.PLANTS if op == "vorticity" else ()) + sm.TRANSPOSITIONS
        fp64 = functools.partial(lambda o, g, f, op, c0: sm.make_c0(o, sm.reference_fp64(o, g[0], op, f)) if c0 else sm.reference_fp64(o, g[0], op, f),
                                 op=op, c0=c0)
        C[key] = Case(key, sm.steps(op, c0), src,
                      functools.partial(lambda o, g, f, plant, op, c0: sm.longdouble(o, g[0], op, f, c0, plant), op=op, c0=c0),
                      fp64, plants, ("sphere_op_view", dict(op=op, c0=c0)))
    for key, order in (("lap", 1), ("bih", 2)):
        C[key] = Case(key, bm.steps(order), "s", functools.partial(lambda o, g, f, plant, order: bm.longdouble(o, f, order, plant), order=order),
                      functools.partial(lambda o, g, f, order: bm.oracle_fp64(o, f, order), order=order),
                      (bm.PLANTS if order == 2 else ()) + bm.TRANSPOSITIONS, ("biharmonic_view", dict(order=order)))
    for i, nu in enumerate(fx["nu_ratio"]):
        nu = float(nu)
        for stem, order in (("vlap", 1), ("vbih", 2)):
            plants = tuple(p for p in vm.PLANTS1 if not (p == "nu_on_vor" and nu == 1.0)) + (vm.PLANTS2 if order == 2 else ()) + vm.TRANSPOSITIONS
            C["%s_nu%d" % (stem, i)] = Case(
                "%s_nu%d" % (stem, i), vm.steps(order), "v",
                functools.partial(lambda o, g, f, plant, order, nu: vm.longdouble(o, g[0], g[1], g[2], f, order, nu, plant), order=order, nu=nu),
                functools.partial(lambda o, g, f, order, nu: vm.reference_chain_fp64(o, g[0], g[1], g[2], f, order, nu), order=order, nu=nu),
                plants, ("vlaplace_view", dict(order=order, nu_ratio=nu)))
    return C


def ratio(got, ref, A, N):
    """|got - ref| / elem_ops_ld.bound(N, A) at every point (0 where the bound is 0 and the value exact)"""
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    b = ld.bound(N, A)
    return np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
