"""limiter_option = 9 (clip-and-sum) without a GPU: the reference model of the limiter (limiter9_model.py) and the front ends.

* The model differs from limiter 8 and from the unlimited step where a limiter has work (the 0/1 noise field) and agrees with limiter 8
  on a uniform field -- otherwise the device comparison of test_gpu_limiter9.py would prove nothing.
* It is not vacuous: it clips in at least a quarter of the slabs of every stage and relaxes a bound in every stage.
* It conserves the tracer mass of every level, and leaves every point inside the relaxed bounds.
* prim_main.settings and tse_init take 9 and still refuse 4 and 84."""
import ctypes as C

import numpy as np
import pytest

import unlimited_model as um
from limiter9_model import Limiter9
from test_unlimited_cpu import CONTINUOUS, DT, NL, STAGES, _state
from tracer_fields import BASE_NAMES, q_err
from transport_se_amd import _lib
from transport_se_amd import prim_main as pm

NOISE, UNIFORM = BASE_NAMES.index("noise"), BASE_NAMES.index("uniform")
ROUNDING_ULPS = 64   # of maxp - minp + |minp| + |maxp|: the redistribution's rounding (x = xc + inc*v, then x*dp_star/dp_star)


@pytest.fixture(scope="module")
def stages9():
    """the three stages of the model with Limiter9 on the ne2 state, computed once: per stage the counts, the per-level mass error of
    the continuous bases, the worst excursion past the relaxed bounds in units of its allowance; and Qdp after stage 1"""
    o = _state()
    out = dict(stats=[], mass=[], excess=[])
    worst = [0.0]

    def watch(x, mn, mx):
        tol = ROUNDING_ULPS * np.spacing(mx - mn + abs(mn) + abs(mx))
        d = max(float((mn - x).max()), float((x - mx).max()))
        if d > 0:
            worst[0] = max(worst[0], d / tol if tol > 0 else np.inf)

    def mass(tl, f=lambda x: x):
        return np.einsum("eqkji,eji->qk", f(o.qdp[tl - 1][:, CONTINUOUS]), o.spheremp)

    lim = Limiter9(o, watch)
    try:
        m0 = mass(1)
        out["dp"] = o.dp.copy()
        for np1, n0, dssopt, rhs in STAGES:
            worst[0] = 0.0
            um.euler_step(o, np1, n0, DT / 2, dssopt, rhs, limiter=lim)
            out["stats"].append((lim.slabs, lim.clipped, lim.relaxed))
            out["mass"].append(float((np.abs(mass(np1) - m0) / np.maximum(mass(np1, np.abs), 1e-300)).max()))
            out["excess"].append(worst[0])
            if rhs == 0:
                out["qdp1"] = o.qdp[1].copy()
    finally:
        o.close()
    return out


def test_differs_from_limiter_8_and_from_no_limiter(stages9):
    o8, o0 = _state(), _state()
    try:
        o8.euler_step(2, 1, DT / 2, 3, 0)
        um.euler_step(o0, 2, 1, DT / 2, 3, 0)
        e8, _ = q_err(stages9["qdp1"], o8.qdp[1], stages9["dp"])
        e0, _ = q_err(stages9["qdp1"], o0.qdp[1], stages9["dp"])
    finally:
        o8.close(); o0.close()
    print("limiter 9 after stage 1: q_err vs limiter 8 %s, vs no limiter %s" % (e8.tolist(), e0.tolist()))
    assert e8[NOISE] > 1e-6 and e0[NOISE] > 1e-6, (e8[NOISE], e0[NOISE])
    assert e8[UNIFORM] <= 1e-13, e8[UNIFORM]


def test_limiter_has_work_in_every_stage(stages9):
    print("limiter 9 (slabs, clipped, relaxed) per stage: %s" % (stages9["stats"],))
    for slabs, clipped, relaxed in stages9["stats"]:
        assert slabs == 10368
        assert 4 * clipped >= slabs, (slabs, clipped)
        assert relaxed >= 1


def test_conserves_mass_per_level(stages9):
    print("limiter 9 per-level mass error per stage: %s" % (stages9["mass"],))
    assert max(stages9["mass"]) < 1e-13, stages9["mass"]


def test_points_stay_inside_the_relaxed_bounds(stages9):
    print("limiter 9 worst excursion past the relaxed bounds per stage, in units of %d ulp: %s" % (ROUNDING_ULPS, stages9["excess"]))
    assert max(stages9["excess"]) <= 1.0, stages9["excess"]


def test_settings_take_limiter_option_9():
    assert pm.settings(pm.parse_namelists(NL.replace("limiter_option = 0", "limiter_option = 9")))["limiter_option"] == 9
    for bad in (4, 84):
        with pytest.raises(SystemExit, match="limiter_option"):
            pm.settings(pm.parse_namelists(NL.replace("limiter_option = 0", "limiter_option = %d" % bad)))


def _init_error(limiter_option):
    L = _lib.lib()
    a = _lib.InitArgs()
    # device 4096 exists nowhere: tse_init fails before it touches a field, on a host with GPUs as on one without
    a.nelemd, a.qsize, a.device, a.limiter_option = 1, 1, 4096, limiter_option
    h = C.c_void_p()
    assert L.tse_init(C.byref(h), C.byref(a)) != 0
    assert not h.value
    return L.tse_last_error().decode()


def test_init_takes_limiter_option_9():
    err = _init_error(9)
    assert err and "limiter" not in err, err
    for bad in (4, 84):
        err = _init_error(bad)
        assert "limiter_option=8" in err and "9" in err.split("supported")[1] and "0" in err.split("supported")[1], err
