"""The predicates of tests/limiter_slab.py on the CPU: they hold, with the margins printed here and quoted in DESIGN.md section 5, on the
oracle's limiter 8, on the limiter-9 model and on a float64 restatement of the device's order, on every input family and its 2^+-200
scalings -- and they catch three small errors planted in the restatement's output (a point one ulp outside its bound, 1e-12 of a slab's
mass dropped, a bound relaxed on a decided-false test).  tests/test_gpu_limiter_slab.py asserts the same predicates of the device."""
import numpy as np
import pytest

import limiter_slab as ls

IMPLS = {"oracle8": (8, ls.oracle8, None), "restate8": (8, ls.restate8, "oracle8"),
         "model9": (9, ls.model9, None), "restate9": (9, ls.restate9, "model9")}


@pytest.fixture(scope="module")
def runs():
    """{family: {"inp": inputs, impl: output}} -- computed once, never modified"""
    fam = ls.families(ls.ne2_spheremp())
    return {name: dict({"inp": inp}, **{k: f(*inp) for k, (_, f, _) in IMPLS.items()}) for name, inp in fam.items()}


def _evaluate(runs, name, impl):
    opt, _, refname = IMPLS[impl]
    r = runs[name]
    return ls.evaluate(opt, r["inp"], r[impl], ref=r[refname] if refname else None, iters=r["oracle8"][4])


def test_families_reach_the_branches(runs):
    """both signs, the dp range, no-op and sumc <= 0 slabs, relaxed bounds, pinned slabs, 1 to 14 iterations; at most 1 % of the slabs of
    any family leave a relaxation test undecided (the only slabs a predicate may skip)"""
    its, guards = {}, {}
    for name, r in runs.items():
        x, c, mn, mx = r["inp"]
        assert x.shape == (ls.N_PER_FAMILY, 4, 4) and not np.any(np.signbit(x) & (x == 0))
        assert (x.reshape(len(x), -1).min(1) < 0).any() and (name == "negmass" or (x.reshape(len(x), -1).max(1) > 0).any()), name
        for impl in IMPLS:
            R = _evaluate(runs, name, impl)
            assert R.undecided.mean() <= 0.01, (name, impl, R.undecided.mean())
        R = _evaluate(runs, name, "oracle8")
        its[name] = r["oracle8"][4]
        if name in ls.IDLE:
            assert R.noop.all(), name
        elif name not in ("flat", "pinned"):
            assert R.noop.mean() < 0.05, name   # (a slab of 16 points may happen to lie inside)
        if name in ("relax", "pinned"):   # (a weighted mean of 16 uniform values lands on the feasible side in a few relax slabs)
            keep = slice(0, -ls.CANCEL_SLABS if name in ls.CANCEL else None)   # (the cancelling slabs are undecided)
            assert min(r["oracle8"][3][keep].mean(), r["model9"][3][keep].mean()) >= (1.0 if name == "pinned" else 0.95), name
        st8, st9 = {}, {}
        ls.restate8(*r["inp"], stats=st8); ls.restate9(*r["inp"], stats=st9)
        guards[name] = (int(st8["w_guard"].sum()), int(st9["den_guard"].sum()))
        if name in ls.CANCEL:   # the cancelling slabs: every point pinned with done false, so limiter 8's `w <= 0` guard decides inc
            assert st8["w_guard"][-ls.CANCEL_SLABS:].all() and R.undecided[-ls.CANCEL_SLABS:].all(), name
        if name == "pinned":   # every point at the relaxed bound: limiter 9's den <= 0 in about half of the slabs
            assert st9["den_guard"].sum() >= len(x) // 4, guards[name]
    allc = np.concatenate([runs[f]["inp"][1] for f in runs if f != "noweight"])
    assert allc.min() > 0 and allc.max() / allc.min() > 1e4
    assert (runs["noweight"]["inp"][1] <= 0).all()
    print("slabs in which (limiter 8's w <= 0, limiter 9's den <= 0) guard decides:", guards)
    print("limiter 8 iterations (oracle):", {k: (int(v.min()), int(v.max())) for k, v in its.items()})
    assert max(v.max() for v in its.values()) <= 14
    assert max(its[f].max() for f in ls.SLOW) >= 6 and its["inside"].max() == 1 and its["noweight"].max() == 0
    # the restatement and the oracle stop at most one iteration apart
    for name, r in runs.items():
        assert np.abs(r["restate8"][4] - np.minimum(r["oracle8"][4], 15)).max() <= 1, name


@pytest.mark.parametrize("impl", list(IMPLS))
def test_predicates_hold_on_the_references(runs, impl):
    """(a)-(e) on every family; the margins (measured / bound) are printed per family"""
    worst = {}
    for name in runs:
        R = _evaluate(runs, name, impl)
        worst[name] = (float(R.ratio_c.max()), float(R.ratio_d.max()), float(R.ratio_e.max()))
        assert not R.bad, (impl, name, R.bad)
    print("%s: family: (c) overshoot/allowance, (d), (e) as measured/bound" % impl)
    for name, w in worst.items():
        print("  %-9s %.3g %.3g %.3g" % ((name,) + w))
    # the rounding allowances K*u*S are used to a few per cent; a flat slab may discard most of the tol*|mass| limiter 8 grants it
    assert max(max(w) for f, w in worst.items() if f != "flat") <= 0.25, worst


@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("e", [200, -200])
def test_scaling(runs, impl, e):
    """(f) x and the bounds times 2^e: the output is exactly 2^e times the unscaled one, and (a)-(e) hold on the scaled slabs"""
    opt, f, refname = IMPLS[impl]
    for name, r in runs.items():
        inp = ls.scaled(r["inp"], e)
        out = f(*inp)
        bad = ls.scaling_bad(r[impl], out, e)
        assert bad.size == 0, (impl, name, e, bad[:6].tolist(), bad.size)
        ref = IMPLS[refname][1](*inp) if refname else None
        R = ls.evaluate(opt, inp, out, ref=ref, iters=r["oracle8"][4])
        assert not R.bad, (impl, name, e, R.bad)


def _planted(runs, name, impl):
    r = runs[name]
    return r["inp"], [np.array(a, copy=True) for a in r[impl][:4]] + [None]


def test_a_point_one_ulp_outside_is_caught(runs):
    inp, out = _planted(runs, "clip", "restate8")
    xo, mno, mxo = out[:3]
    flat = xo.reshape(len(xo), 16)
    at_hi = flat == mxo[:, None]
    s = np.nonzero(at_hi.any(1))[0]
    assert s.size > 50
    p = at_hi[s].argmax(1)
    flat[s, p] = np.nextafter(flat[s, p], np.inf)
    R = ls.evaluate(8, inp, out, ref=runs["clip"]["oracle8"], iters=runs["clip"]["oracle8"][4])
    assert [b for b in R.bad if b[0].startswith("(c)") and b[2] == s.size], R.bad


@pytest.mark.parametrize("impl", ["restate8", "restate9"])
def test_a_lost_1e12_of_the_mass_is_caught(runs, impl):
    """1e-12 of the slab's mass taken from the point farthest from both bounds (same-sign slabs: |mass| = sum c*|x|)"""
    inp, out = _planted(runs, "clip", impl)
    x, c = inp[:2]
    xo, mno, mxo = out[:3]
    mass = (c * x).sum((1, 2))
    room = np.minimum(xo - mno[:, None, None], mxo[:, None, None] - xo).reshape(len(xo), 16)
    p = room.argmax(1); s = np.nonzero(room.max(1) > 1e-3)[0]; p = p[s]
    assert s.size > 200
    xo.reshape(len(xo), 16)[s, p] -= 1e-12 * mass[s] / c.reshape(len(xo), 16)[s, p]
    ref = runs["clip"]["oracle8" if impl == "restate8" else "model9"]
    R = ls.evaluate(int(impl[-1]), inp, out, ref=ref, iters=runs["clip"]["oracle8"][4])
    assert (R.ratio_d[s] > 1).all() and R.failed("(d)"), (R.ratio_d[s].min(), R.bad)
    assert not R.failed("(c)")


@pytest.mark.parametrize("impl", ["restate8", "restate9"])
def test_a_bound_relaxed_on_a_decided_false_test_is_caught(runs, impl):
    inp, out = _planted(runs, "inside", impl)
    x, c = inp[:2]
    out[1] = (c * x).sum((1, 2)) / c.sum((1, 2))   # minp = mass/sumc although mass > minp*sumc
    out[3] = np.ones(len(x), bool)
    R = ls.evaluate(int(impl[-1]), inp, out, iters=runs["inside"]["oracle8"][4])
    hit = [b for b in R.bad if b[0].startswith("(b) minp relaxed")]
    assert hit and hit[0][2] == len(x), R.bad


def test_the_guards_of_the_all_pinned_slab_are_needed(runs):
    """without limiter 8's `w <= 0` guard (resp. limiter 9's `den > 0`) the restatement turns exactly the slabs the guard decides into
    NaN, and the `finite` predicate says so: the families would catch a kernel that lost either guard"""
    for name in ls.CANCEL:
        inp = runs[name]["inp"]
        for opt, f, key in ((8, ls.restate8, "w_guard"), (9, ls.restate9, "den_guard")):
            st = {}
            f(*inp, stats=st)
            out = f(*inp, guard=False)
            nan = ~np.isfinite(out[0]).reshape(len(out[0]), -1).all(1)
            assert (st[key].any() or (opt == 9 and name != "pinned")) and np.array_equal(nan, st[key]), (name, opt, int(nan.sum()), int(st[key].sum()))
            if not st[key].any():   # (limiter 9 meets den <= 0 in the pinned family only)
                continue
            R = ls.evaluate(opt, inp, out, iters=runs[name]["oracle8"][4])
            hit = [b for b in R.bad if b[0] == "finite"]
            assert hit and hit[0][2] == int(st[key].sum()), R.bad
