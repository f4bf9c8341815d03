"""The longdouble model of the PPM remap and its pointwise bound (tests/remap_ld.py) on the CPU: the inputs the GPU test
(test_gpu_remap_pointwise.py) hands to the device satisfy the kernel's precondition; the model is right (tests/remap_model.py in fp64,
the oracle at 72 levels and the reference's own single-call outputs under tests/golden/ lie within the bound on every safe output); at
most 1 % of the outputs of any (grid family, tracer family, level count, algorithm) are excluded as unsafe; and the bound has teeth: a
vectorised fp64 copy of the kernel's arithmetic (folded coefficients, reciprocals, other associations, and the tie rule `<` on the
identity grid) stays within it, six realistic mutations of that copy do not.

Three mutations that look just as realistic change NO safe output, and the list below was chosen with that in mind.  (a) The mean of
a ghost cell off by one (a(0) = a(2)) and alg 2 forgetting cell 1 or cell nlev: with mirrored ghost cells ai(0) = a(1) and ai(nlev) =
a(nlev) bit for bit, so the limiter flattens the two end cells whatever a(0) is -- alg 2 differs from alg 0 in cells 2 and nlev-1
only (and by one rounding of c0 in the end cells).  So mutation 2 mirrors the ghost THICKNESS off by one as well, and mutation 5 forgets cell 2.  (b) 1/6 in float32: the constant
appears in the two comparisons only, so it can move a decision only where the discriminant lies within 6e-9 (relative) of the switch,
where the remap is continuous; on the test fields no decision moves at all.  Mutation 3 takes the integral's 1/3 in float32 instead.
(c) The seventh mutation one might think of -- a segment task that starts from an old-mass prefix short by one cell -- cannot be seen by
any test of the outputs: the task's run-in level and all its levels carry the same prefix, so every new level, the difference of two
running masses, loses the missing cell from both ends (only roundings move).  It is left out for that reason.
test_mutations_that_change_no_safe_output demonstrates (a), (b) and (c) on the fp64 copy."""
import functools
import os

import numpy as np
import pytest

import pyoracle as po
import remap_ld as rl
import remap_model as rm
from step_ld import has_extended_precision, ratio

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAP = 0.01     # at most 1 % of the outputs of a combination may be unsafe


@functools.lru_cache(maxsize=2)
def _model(nlev, alg, qsize):
    assert has_extended_precision(), np.finfo(np.longdouble)
    Q, dp1, dp2 = rl.inputs(nlev, qsize)
    return (Q, dp1, dp2) + rl.remap_q_ppm(Q, dp1, dp2, alg)


def _elements(grid):
    return [e for e in range(rl.NELEM) if rl.grid_family(e) == grid]


def _worst_safe(got, t, safe):
    _, r = ratio(got, t)
    r = np.where(safe, r, 0.0)
    return float(r.max()), np.unravel_index(int(np.argmax(r)), r.shape)


# ---- the inputs ----
@pytest.mark.parametrize("nlev", [72, 64])
def test_inputs_satisfy_the_precondition_and_are_what_their_names_say(nlev):
    """dp1 > 0, dp2 > 0, pin(k+1) < pio(nlev+1) + 1 in fp64 serial order (grid_fp64 asserts it; inputs() runs it); sum(dp1) == sum(dp2)
    to rounding; gentle: kid(k) in {k, k+1} everywhere (lockstep loop); squeeze: displaced by more than 15 layers (generic loop);
    identity: every interface an exact pio == pin tie; thin: one layer at 1e-3 of its neighbours; tracer scalings 2^-200 .. 2^200"""
    for qsize in rl.QSIZES:
        Q, dp1, dp2 = rl.inputs(nlev, qsize)
        assert Q.shape == (rl.NELEM, qsize, nlev, 4, 4) and dp1.shape == dp2.shape == (rl.NELEM, nlev, 4, 4)
        rl.check_inputs(dp1, dp2)
        ex = rl.exponents(qsize)
        assert ex[0] == -200 and (qsize == 1 or ex[-1] == 200)
    assert np.abs(dp1.sum(1) / dp2.sum(1) - 1).max() < 1e-14
    E = rl.NELEM
    dpo, pio, pin, kid = rl.grid_fp64(np.moveaxis(dp1.reshape(E, nlev, 16), 1, 0).reshape(nlev, -1),
                                      np.moveaxis(dp2.reshape(E, nlev, 16), 1, 0).reshape(nlev, -1))
    off = (kid - np.arange(1, nlev + 1)[:, None]).reshape(nlev, E, 16)
    assert {rl.grid_family(e) for e in range(E)} == set(rl.GRIDS)
    for e in range(E):
        fam = rl.grid_family(e)
        if fam in ("gentle", "identity"):
            assert off[:, e].min() >= 0 and off[:, e].max() <= 1, (fam, e)
        if fam == "gentle":
            assert (off[:, e] == 0).any() and (off[:-1, e] == 1).any()
        if fam == "squeeze":
            assert off[:, e].max() > 15
        if fam == "identity":
            assert np.array_equal(dp1[e], dp2[e]) and (off[:-1, e] == 1).all()
            c = slice(e * 16, e * 16 + 16)
            assert np.array_equal(pio[1:nlev + 2, c], pin[1:nlev + 2, c])
        if fam == "thin":
            r = dp1[e][1:-1] / np.minimum(dp1[e][:-2], dp1[e][2:])
            assert (np.sort(r, axis=0)[0] < 1.1e-3).all() and (np.sort(r, axis=0)[1] > 1e-2).all()


def test_the_precondition_check_refuses_a_grid_the_search_cannot_end_on():
    """(host arrays only: nothing of this reaches a library)"""
    _, dp1, dp2 = rl.inputs(72, 1)
    bad = dp2.copy(); bad[3, 70, 1, 2] += dp2[3, 71, 1, 2] + 2.0    # the partial sum above the last level exceeds sum(dp1) + 1
    with pytest.raises(AssertionError):
        rl.check_inputs(dp1, bad)
    bad = dp2.copy(); bad[0, 0, 0, 0] = 0.0
    with pytest.raises(AssertionError):
        rl.check_inputs(dp1, bad)
    bad = dp1.copy(); bad[5, 71, 3, 3] = -1.0
    with pytest.raises(AssertionError):
        rl.check_inputs(bad, dp2)


# ---- the model is right, and excludes little ----
@pytest.mark.parametrize("alg", [0, 2])
@pytest.mark.parametrize("nlev", [72, 64])
def test_fp64_models_lie_within_the_bound_and_at_most_one_percent_is_excluded(nlev, alg):
    """every qsize the GPU test uses (the very arrays): per grid family and tracer family at most 1 % of the outputs unsafe (a condition,
    with the real criterion); remap_model.remap_q_ppm in fp64, and at 72 levels the oracle (alg 0 and 2), within the bound on every safe one"""
    worst = {}
    for qsize in rl.QSIZES:
        Q, dp1, dp2, t, safe, kid = _model(nlev, alg, qsize)
        assert t.m == max(nlev - 1, 55) + 2
        ref = np.stack([rm.remap_q_ppm(Q[e], dp1[e], dp2[e], alg) for e in range(rl.NELEM)])
        w, ix = _worst_safe(ref, t, safe)
        assert w <= 1.0, ("remap_model", nlev, alg, qsize, w, ix)
        worst["model q%d" % qsize] = w
        wm, rmass = rl.column_mass_ratio(ref, Q, t)              # every column, unsafe ones included
        assert wm <= 1.0, ("column mass", nlev, alg, qsize, wm)
        if nlev == 72:
            po.set_vert_remap_q_alg(alg)
            try:
                orc = np.stack([po.remap_q_ppm(Q[e], dp1[e], dp2[e]) for e in range(rl.NELEM)])
            finally:
                po.set_vert_remap_q_alg(0)
            w, ix = _worst_safe(orc, t, safe)
            assert w <= 1.0, ("oracle", qsize, w, ix)
            worst["oracle q%d" % qsize] = w
        for grid in rl.GRIDS:
            es = _elements(grid)
            for f, fam in enumerate(rl.TRACERS):
                qs = [q for q in range(qsize) if rl.tracer_family(q) == fam]
                if qs:
                    frac = 1.0 - safe[es][:, qs].mean()
                    assert frac <= CAP, (nlev, alg, qsize, grid, fam, frac)
        assert safe.mean() > 0.99
    print("nlev %d alg %d: worst |fp64 - v| / bound on safe outputs %s" % (nlev, alg, worst))


@pytest.mark.parametrize("name,alg", [("ref_ops.npz", 0), ("ref_ne2_alg2.npz", 2)])
def test_the_references_own_outputs_lie_within_the_bound(name, alg):
    """remap_Qin, dp1, dp2 -> Qout as the reference's remap_Q_ppm computed it (vert_remap_q_alg 0 and 2)"""
    g = np.load(os.path.join(GOLD, name))
    q, dp1, dp2, out = g["remap_Qin"], g["remap_dp1"], g["remap_dp2"], g["remap_Qout"]
    assert has_extended_precision(), np.finfo(np.longdouble)
    rl.check_inputs(dp1, dp2)
    t, safe, kid = rl.remap_q_ppm(q, dp1, dp2, alg)
    per = [float(safe[:, q].mean()) for q in range(q.shape[1])]   # (the cap is a property of the generator's families, not of this field)
    assert max(per) > 0.99, per
    w, ix = _worst_safe(out, t, safe)
    print("%s: worst ratio %.3g at %s; safe fraction per tracer %s" % (name, w, ix, per))
    assert w <= 1.0, (name, w, ix)


# ---- the bound has teeth ----
def kernel_copy(Q, d1, d2, alg, mut=0, tie_lt=False, level6=10):
    """k_remap's arithmetic in vectorised fp64 numpy on [nlev][nq][C] columns: the five folded coefficients, reciprocals for every
    division, products and sums associated differently from remap_model.py.  tie_lt: the bracket search with `<` for `<=`.
    mut: 1 f8 and f9 swapped; 2 ghost mirror off by one (cell 0 = cell 2, mean and thickness: the mean alone changes no output, because
    a(0) only enters cell 1, which the limiter flattens either way); 3 the integral's 1/3 taken in float32; 4 the z^3 term's 1/8 off by 2^-40;
    5 alg 2 overrides cells 1, nlev-1, nlev only; 6 the kid(k) == k+1 bit ignored at level `level6` (masso(k) where masso(k+1) is due).
    Mutations that change no safe output: 12 the ghost MEAN alone off by one (a(0) = a(2)); 13 1/6 taken in float32; 15 alg 2 overrides
    cells 2 and nlev-1 only; 17 every segment task (8 levels, from level 9 on, with its run-in level) starts from an old-mass prefix
    short by one cell"""
    nlev, nq, C = Q.shape
    dpo, pio, pin, kid = rl.grid_fp64(d1, d2)
    if tie_lt:
        for k in range(1, nlev + 1):
            kid[k - 1] = np.minimum(k + np.argmax(pio[k:nlev + 3] >= pin[k + 1], axis=0) - 1, nlev)
    if mut == 2:
        dpo[1] = dpo[3]
    X = dpo[:, None, :]
    n = nlev + 2
    m_, c_, p_ = X[0:n], X[1:n + 1], X[2:n + 2]
    r0 = c_ * (1. / (m_ + (c_ + p_)))
    e1, e2 = r0 * ((m_ + m_ + c_) * (1. / (p_ + c_))), r0 * ((c_ + (p_ + p_)) * (1. / (m_ + c_)))
    n = nlev + 1
    m_, c_, p_, pp = X[0:n], X[1:n + 1], X[2:n + 2], X[3:n + 3]
    r4 = 1. / ((m_ + c_) + (p_ + pp))
    r678 = (2. * p_ * (c_ * (1. / (c_ + p_)))) * ((m_ + c_) * (1. / (2. * c_ + p_)) - (pp + p_) * (1. / (2. * p_ + c_)))
    f3 = c_ * (1. / (c_ + p_)) + r4 * r678
    f8 = r4 * (c_ * ((m_ + c_) * (1. / (2. * c_ + p_))))
    f9 = r4 * (p_ * ((p_ + pp) * (1. / (c_ + 2. * p_))))
    if mut == 1:
        f8, f9 = f9, f8
    a = Q * (1. / X[2:nlev + 2])
    af = np.concatenate([a[1:2], a[0:1], a, a[nlev - 1:nlev], a[nlev - 2:nlev - 1]])
    if mut in (2, 12):
        af[1] = a[1]
    d = af[1:] - af[:-1]
    dp_, dm_ = d[1:nlev + 3], d[0:nlev + 2]
    da = e2 * dm_ + e1 * dp_
    mg = np.minimum(2. * np.minimum(np.abs(dm_), np.abs(dp_)), np.abs(da))
    dma = np.where(dp_ * dm_ <= 0., 0., np.copysign(mg, da))
    ai = f9 * dma[0:n] + ((f3 * d[1:n + 1] + af[1:n + 1]) - f8 * dma[1:n + 1])
    al, ar, aj = ai[0:nlev], ai[1:nlev + 1], af[2:nlev + 2]
    flat = (ar - aj) * (aj - al) <= 0.
    al, ar = np.where(flat, aj, al), np.where(flat, aj, ar)
    sixth = float(np.float32(1.0 / 6.0)) if mut == 13 else 1.0 / 6.0
    w = ar - al
    al = np.where(w * (aj - 0.5 * (al + ar)) > w * w * sixth, 3. * aj - 2. * ar, al)
    w = ar - al
    ar = np.where(w * (aj - 0.5 * (al + ar)) < -(w * w) * sixth, 3. * aj - 2. * al, ar)
    c0, c1, c2 = 1.5 * aj - 0.25 * (al + ar), ar - al, 3. * (al + ar) - 6. * aj
    if alg == 2:
        pc = np.zeros((nlev, 1, 1), dtype=bool); pc[[1, nlev - 2] if mut == 15 else [0, nlev - 2, nlev - 1] + ([] if mut == 5 else [1])] = True
        c0, c1, c2 = np.where(pc, aj, c0), np.where(pc, 0., c1), np.where(pc, 0., c2)
    g = lambda x: np.take_along_axis(x, kid, 0)          # noqa: E731
    x2 = ((pin[2:nlev + 2] - (g(pio) + g(pio[1:])) * 0.5) * (1. / g(dpo[1:])))[:, None, :]
    z1, zz2, z3 = x2 + 0.5, (x2 * x2 - 0.25) * 0.5, x2 * (x2 * x2) + (0.125 + (2.0 ** -40 if mut == 4 else 0.0))
    ci = (kid - 1)[:, None, :]
    t = lambda x: np.take_along_axis(x, ci, 0)           # noqa: E731
    integ = (t(c2) * z3) * (float(np.float32(1.0 / 3.0)) if mut == 3 else 1.0 / 3.0) + (t(c1) * zz2 + t(c0) * z1)
    pre = np.zeros((nlev + 1, nq, C))                    # old-mass prefixes added in pairs
    pairs = np.cumsum(Q[0:nlev - 1:2] + Q[1:nlev:2], axis=0)
    pre[2::2] = pairs
    pre[1::2] = np.concatenate([np.zeros((1, nq, C)), pairs[:-1]]) + Q[0::2][:pre[1::2].shape[0]]
    ms = t(pre)
    if mut == 6:
        k = level6
        ms[k - 1] = np.where((kid[k - 1] == k + 1)[None, :], np.take_along_axis(pre, ci[k - 1:k] - 1, 0)[0], ms[k - 1])
    massn2 = ms + integ * g(dpo[1:])[:, None, :]
    out = massn2 - np.concatenate([np.zeros((1, nq, C)), massn2[:-1]])
    if mut == 17:
        for s in range(1, nlev // 8):        # levels 8s+1 .. 8s+8 after the run-in level 8s, all on a prefix without cell 8s-1
            short = (ms[8 * s - 1:8 * s + 8] - Q[8 * s - 2]) + (integ * g(dpo[1:])[:, None, :])[8 * s - 1:8 * s + 8]
            out[8 * s:8 * s + 8] = short[1:] - short[:-1]
    return out


def _columns(nlev, alg, qsize=12):
    Q, dp1, dp2, t, safe, kid = _model(nlev, alg, qsize)
    E = rl.NELEM
    return rl._cols(Q, E, nlev), rl._cols(dp1, E, nlev), rl._cols(dp2, E, nlev), t, safe


def _copy(nlev, alg, **kw):
    Qc, d1, d2, t, safe = _columns(nlev, alg)
    return rl._back(kernel_copy(Qc, d1, d2, alg, **kw), rl.NELEM, Qc.shape[1], nlev), t, safe


@pytest.mark.parametrize("alg", [0, 2])
@pytest.mark.parametrize("nlev", [72, 64])
def test_the_kernels_arithmetic_stays_within_the_bound(nlev, alg):
    """folded coefficients, reciprocals, other associations: within the bound on every safe output; and so is the tie rule `<` for
    `<=`, which moves kid(k) by one on every interface of the identity grid (the remap is continuous across kid)"""
    got, t, safe = _copy(nlev, alg)
    w, ix = _worst_safe(got, t, safe)
    assert w <= 1.0, (w, ix)
    tie, _, _ = _copy(nlev, alg, tie_lt=True)
    es = _elements("identity")
    assert not np.array_equal(tie[es], got[es])
    w2, ix = _worst_safe(tie, t, safe)
    assert w2 <= 1.0, ("tie rule", w2, ix)
    print("nlev %d alg %d: kernel copy %.3g, with the tie rule `<` %.3g" % (nlev, alg, w, w2))


MUTATIONS = [(1, 0, "f8 and f9 swapped"), (2, 0, "ghost mirror off by one"), (3, 0, "1/3 in float32"), (4, 0, "1/8 off by 2^-40"),
             (5, 2, "alg 2 leaves cell 2"), (6, 0, "kid bit ignored at one level")]


@pytest.mark.parametrize("nlev", [72, 64])
@pytest.mark.parametrize("mut,alg,what", MUTATIONS, ids=[m[2].replace(" ", "-") for m in MUTATIONS])
def test_a_mutated_kernel_breaks_the_bound_on_a_safe_output(nlev, mut, alg, what):
    got, t, safe = _copy(nlev, alg, mut=mut)
    w, ix = _worst_safe(got, t, safe)
    _, r = ratio(got, t)
    print("nlev %d %s: worst ratio %.3g at (element, tracer, level, j, i) = %s; %d safe outputs over" % (nlev, what, w, ix, int(((r > 1) & safe).sum())))
    assert w > 1.0, (what, w)


NULL_MUTATIONS = [(12, 0, "ghost mean off by one"), (13, 0, "1/6 in float32"), (15, 2, "alg 2 leaves cells 1 and nlev"),
                  (17, 0, "segment prefixes short by one cell")]


@pytest.mark.parametrize("nlev", [72, 64])
@pytest.mark.parametrize("mut,alg,what", NULL_MUTATIONS, ids=[m[2].replace(" ", "-") for m in NULL_MUTATIONS])
def test_mutations_that_change_no_safe_output(nlev, mut, alg, what):
    """the evidence for the module docstring's (a), (b), (c): the ghost mean and 1/6 in float32 leave EVERY output of the clean copy bit
    for bit (safe or not); alg 2 forgetting the end cells (the limiter's flat cell forms c0 = 1.5 a - 0.25 (a + a), one rounding away
    from a) and the short segment prefix move roundings only and stay within the bound"""
    clean, t, safe = _copy(nlev, alg)
    got, _, _ = _copy(nlev, alg, mut=mut)
    if mut in (15, 17):
        assert not np.array_equal(got, clean)
        w, ix = _worst_safe(got, t, safe)
        print("nlev %d %s: worst ratio %.3g" % (nlev, what, w))
        assert w <= 1.0, (what, w, ix)
    else:
        assert np.array_equal(got.view(np.uint64), clean.view(np.uint64)), (what, int((got != clean).sum()))
