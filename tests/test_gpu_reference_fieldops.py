"""-m gpu: the view entries against the reference's own Fortran -- tests/golden/ref_ne2_fieldops.npz (derivative_mod.F90 and
viscosity_mod.F90 on all 24 elements of ne2 and three levels, oracle/ref/ref_harness.F90's dump_fieldops), on a context built from the
reference's own metric terms (ref_ne2_static.npz, as test_gpu_ops_golden.ref_ctx) and vector tables from the reference's D, metinv, mp.

dss_view (both modes), biharmonic_view (orders 1, 2), vlaplace_view (orders 1, 2, nu_ratio 1 and 2.5) and sphere_op_view (three ops, LOCAL
and C0; C0 also against compute_zeta_C0 / compute_div_C0 and on a continuous field), each once through a point-fastest and once through a
level-fastest view.  Bound: |device - reference| <= 2 * elem_ops_ld.bound(N, A) at every point, N and A the model's
(tests/fieldops_ref.py): the device and the reference each lie under bound(N, A) against the longdouble chain
(test_gpu_*_view.py, test_reference_fieldops_cpu.py), and the factor 2 is the triangle inequality, not a measurement."""

import numpy as np
import pytest

import dss_view_model as dm
import elem_ops_ld as ld
import fieldops_ref as fr
from conftest import record_margin
from view_common import FakeArray as _Fake

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
LAYOUTS = ("dense", "lev_even")          # point-fastest; level-fastest (rows of levels, padded to an even pitch)
KEYS = tuple(fr.cases(dict(nu_ratio=(1.0, 2.5))))


@pytest.fixture(scope="module")
def ctx(gold):
    from transport_se_amd.hip_mod import HipMod
    st, fx = gold("ref_ne2_static.npz"), gold("ref_ne2_fieldops.npz")
    st = {k: st[k] for k in st.files}
    fx = {k: fx[k] for k in fx.files}
    elem = dict(Dinv=st["Dinv"], metdet=st["metdet"], rmetdet=st["rmetdet"], spheremp=st["spheremp"], rspheremp=st["rspheremp"],
                putmapP=st["putmap"].astype(np.int32), getmapP=st["getmap"].astype(np.int32), reverse=st["reverse"].astype(np.int32))
    hip = HipMod(elem, st["Dvv"], (st["hyai"], st["hybi"], float(st["ps0"])), 3, 1e19, device=0)
    assert hip.nlev == 72 and hip.nelemd == 24
    geo = (st["D"], fx["metinv"], st["mp"])
    hip.vector_setup(*geo)
    o = fr.mesh(st)
    yield hip, o, geo, fx, fr.cases(fx)
    hip.close(); o.close()


def _device(hip, call, f, nf_out, name):
    """the view call on the host field f[n][nf][nk][4][4] laid out as `name` -> the result [n][nf_out][nk][4][4]; the gaps of the output
    keep their bits"""
    import torch
    entry, kw = call
    S = dm.Strided(f, name)
    buf = torch.from_numpy(S.host.copy()).cuda()
    src = _Fake(S.shape, S.s, buf.data_ptr() + 8 * S.base)
    if entry == "dss_view":
        hip.dss_view(src, "eqkji", **kw)
        T, res = S, buf
    else:
        T = dm.Strided(np.full((f.shape[0], nf_out) + f.shape[2:], SENTINEL), name)
        res = torch.from_numpy(T.host.copy()).cuda()
        dst = _Fake(T.shape, T.s, res.data_ptr() + 8 * T.base)
        if entry == "sphere_op_view":
            hip.sphere_op_view(src, "eqkji", dst, **kw)
        else:
            getattr(hip, entry)(src, "eqkji", out=dst, **kw)
        assert np.array_equal(dm.bits(buf.cpu().numpy()), dm.bits(S.host)), "the input changed"
    got, gaps = T.read(res.cpu().numpy())
    assert gaps, "bytes outside the view changed"
    return got


def _hold(key, name, got, want, A, N):
    b = 2.0 * ld.bound(N, A)
    d = np.abs(got - want)
    r = np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d > 0, np.inf, 0.0))
    worst = float(r.max())
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    print("device %s (%s) vs reference: worst |diff| / (2 bound(%d, A)) = %.3f at (element, field, level, j, i) = %s" % (key, name, N, worst, at))
    record_margin("device %s (%s) vs the reference's Fortran / 2 bound(%d, A)" % (key, name, N), worst, 1.0)
    assert np.isfinite(got).all() and not (got == SENTINEL).any()
    assert worst <= 1.0, (key, name, worst, at)


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("key", KEYS)
def test_view_entry_against_the_reference(ctx, key, name):
    hip, o, geo, fx, cases = ctx
    c = cases[key]
    f, want = fx[c.src], fx[c.out]
    _, A = _chain(ctx, key)
    _hold(key, name, _device(hip, c.call, f, want.shape[1], name), want, A, c.N)


_CHAINS = {}


def _chain(ctx, key, nk=None):
    hip, o, geo, fx, cases = ctx
    if (key, nk) not in _CHAINS:
        c = cases[key]
        _CHAINS[(key, nk)] = c.ld(o, geo, fx[c.src][:, :, :nk], None)
    return _CHAINS[(key, nk)]


@pytest.mark.parametrize("name", LAYOUTS)
def test_one_level_alone(ctx, name):
    """nk = 1 (where a row of one level is point-fastest in either layout): the vorticity of the fixture's first level"""
    hip, o, geo, fx, cases = ctx
    c = cases["vor"]
    f, want = np.ascontiguousarray(fx["v"][:, :, :1]), fx["vor"][:, :, :1]
    _, A = _chain(ctx, "vor", 1)
    _hold("vor nk=1", name, _device(hip, c.call, f, 1, name), want, A, c.N)
