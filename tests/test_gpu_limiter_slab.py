"""-m gpu: limiter8_quad and limiter9_quad alone on the device (tse_test_limiter of the -DTSE_AB_HOOKS library), slab by slab.

Whole stages and steps hold the limiters to 1e-13 of a field maximum; here a limiter is a function of 34 numbers, and the predicates of
tests/limiter_slab.py (no-op, relaxation, bounds, mass, the reference, scaling -- each true whichever way a near-tie falls) are asserted of
every slab of every input family and its 2^+-200 scalings, against pyoracle.limiter8 / limiter9_model.limiter9.  The entry runs the limiters'
own source, one wave per 16 consecutive slabs, so the caller chooses a slab's wave-mates: a slab's bits must not depend on them (the
wave-wide __any around limiter 8's division, its wave-wide __all(done) exit).  tests/test_limiter_slab_cpu.py shows the predicates holding on
the references and catching planted errors; level-order invariance (tests/test_gpu_level_order.py) covers the copies inlined in the
production kernels."""
import numpy as np
import pytest

import limiter_slab as ls
from conftest import record_margin
from transport_se_amd import _lib

pytestmark = pytest.mark.gpu

SCALES = (0, 200, -200)


@pytest.fixture(scope="module")
def batch():
    """the families in order, unscaled, then times 2^200, then times 2^-200; the references' outputs (computed once)"""
    fam = ls.families(ls.ne2_spheremp())
    inp = ls.concat([ls.scaled(fam[f], e) if e else fam[f] for e in SCALES for f in ls.FAMILIES])
    return {"inp": inp, 8: ls.oracle8(*inp), 9: ls.model9(*inp), "nfam": len(ls.FAMILIES), "n": ls.N_PER_FAMILY}


@pytest.mark.parametrize("option", [8, 9])
def test_predicates_on_the_device(batch, option):
    """(a)-(f) of tests/limiter_slab.py on every slab; at most 1 % of a family's slabs leave a relaxation test undecided"""
    inp, ref = batch["inp"], batch[option]
    out = ls.device(option, *inp)
    R = ls.evaluate(option, inp, out, ref=ref, iters=batch[8][4])
    n, nf = batch["n"], batch["nfam"]
    for i in range(nf * len(SCALES)):
        sl = slice(i * n, (i + 1) * n)
        name = "limiter %d slab %s 2^%d" % (option, ls.FAMILIES[i % nf], SCALES[i // nf])
        print("%-36s (c) %.3g (d) %.3g (e) %.3g undecided %d" % (name, R.ratio_c[sl].max(), R.ratio_d[sl].max(), R.ratio_e[sl].max(),
                                                                   R.undecided[sl].sum()))
        record_margin(name + " (d) mass", R.ratio_d[sl].max(), 1.0)
        record_margin(name + " (e) reference", R.ratio_e[sl].max(), 1.0)
        if option == 9:
            record_margin(name + " (c) overshoot", R.ratio_c[sl].max(), 1.0)
        assert R.undecided[sl].mean() <= 0.01, name
    assert not R.bad, R.bad
    N = nf * n
    for k, e in enumerate(SCALES[1:], 1):
        bad = ls.scaling_bad([a[:N] for a in out[:4]], [a[k * N:(k + 1) * N] for a in out[:4]], e)
        assert bad.size == 0, (e, bad[:8].tolist(), bad.size)


@pytest.mark.parametrize("option", [8, 9])
def test_a_slab_does_not_depend_on_its_wave_mates(batch, option):
    """the same slabs in family order, interleaved so that every wave of 16 mixes no-op slabs, sumc <= 0 slabs and the slabs that
    iterate most, and each alone among 15 copies of itself: x, the bounds and `changed` are the same bits in all three"""
    n, nf = batch["n"], batch["nfam"]
    N = nf * n
    inp = ls.take(batch["inp"], np.arange(N))
    a = ls.device(option, *inp)
    perm = np.arange(N).reshape(nf, n).T.ravel()   # round-robin over the families: 16 consecutive slabs span all 9
    fam_of = perm // n
    for w in range(0, N - 15, 16):
        f = {ls.FAMILIES[i] for i in fam_of[w:w + 16]}
        assert f.issuperset(ls.IDLE) and f.issuperset(ls.SLOW)
    b = ls.device(option, *ls.take(inp, perm))
    alone = ls.device(option, *ls.take(inp, np.repeat(np.arange(N), 16)))
    for what, got in (("interleaved", [np.empty_like(v) for v in b[:4]]), ("alone", [v[::16] for v in alone[:4]])):
        if what == "interleaved":
            for g, v in zip(got, b[:4]):
                g[perm] = v
        for nm, u, v in zip(("x", "minp", "maxp"), a[:3], got[:3]):
            bad = np.nonzero(~ls._same(u, v))[0]
            assert bad.size == 0, (what, nm, [(ls.FAMILIES[s // n], int(s % n)) for s in bad[:8]], bad.size)
        assert np.array_equal(a[3], got[3]), what
    for v in alone[:3]:   # the 16 copies of a slab agree among themselves
        assert ls._same(v.reshape((N, 16) + v.shape[1:]), np.repeat(v[::16], 16, axis=0).reshape((N, 16) + v.shape[1:])).all()


def test_the_product_library_has_no_slab_entry():
    assert hasattr(_lib.lib(_lib.HOOKS_SO), "tse_test_limiter")
    for nlev in (None,) + tuple(_lib.NLEV_BUILDS):
        assert not hasattr(_lib.lib(nlev=nlev), "tse_test_limiter"), nlev
