"""diagnostics -- the numbers the reference's tests look at, as product code.

* `dcmip_norms`: L1/L2/Linf/q_max/q_min exactly as test/dcmip1-1/dcmip1-1_error_norm_ng.ncl:39-77 (and the dcmip1-2 twin)
  computes them from the history file: unique-column native grid, dV = R cos(lat) dlon * R dlat * dh(lev) with dh rebuilt
  from the level heights by the "2*(h-base)" recursion, relative to (q0 - avg(q0)).
* `column_weights` / `norms_from_partials`: the same norm line without the field on the host -- the device forms every element's share
  over the columns it owns (tse_norm_partials), rank 0 adds the shares exactly.
* `mixing_diagnostics` / `mixing_from_partials`: the numerical-mixing diagnostics l_r, l_u, l_o and the filament diagnostic l_f of
  Lauritzen and Thuburn (2012) for two tracers that start on a quadratic curve (DCMIP 1-1's q1, q2) -- from whole fields on the host, and
  from the element shares the device forms (tse_mix_partials), added exactly on rank 0.
* `tracer_mass`: the conserved integral behind the "Q,Q diss" line (prim_state_mod.F90:352-385 through
  global_integral, global_norms_mod.F90:39-86).
* `printstate_lines`: the `qv=  min max sum` lines of prim_printstate (prim_state_mod.F90:341-347).
* `stats_from_partials` / `printstate_field_lines` / `fortran_e`: min, max, sum, integral, mean and the l1 / l2 / linf norms of a resident
  host's own fields from the element shares the device forms (tse_stats_view), added exactly, and prim_printstate's `u = `, `v = `,
  `T = `, `ps= `, `M = ` lines in its format 100 from them.
* `global_sum` / `gather_by_gid`: the multi-rank forms.  The reference makes its global integrals independent of the task
  count with a fixed-point reproducible sum (repro_sum_mod.F90:216-632; "independent of thread count and task count",
  global_norms_mod.F90:66-68).  Here every ELEMENT's partial sum is formed in a fixed order (on the device:
  tse_element_mass), the partials travel to rank 0, and rank 0 adds them with math.fsum -- the correctly rounded exact sum,
  which does not depend on the order, hence not on how the elements were distributed.  The error norms go the same way
  (tse_norm_partials -> norms_from_partials).  `gather_by_gid` reassembles per-element rows on rank 0 in global element order.
"""
import math

import numpy as np

G = 9.80616      # physical_constants.F90:23
RGAS = 287.04    # :25
P0 = 100000.0    # :27


def unique_columns(lat, lon):
    """one owner per distinct GLL node: the first point in (element, j, i) order, i.e. the smallest
    (ig-1)*np^2+(j-1)*np+i among the sharers (dof_mod.F90:43-57,95-116)"""
    lat = np.asarray(lat).reshape(-1); lon = np.asarray(lon).reshape(-1)
    xyz = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1)
    key = np.round(xyz * 1e8).astype(np.int64)
    _, first = np.unique(key, axis=0, return_index=True)
    return np.sort(first)


def level_heights(hyam, hybm):
    """z_m = H ln(1/eta_m), H = Rd*T0/g with T0 = 300 K (dcmip_wrapper_mod.F90:24-25,68)"""
    return (RGAS * 300.0 / G) * np.log(1.0 / (np.asarray(hyam) + np.asarray(hybm)))


def hybrid_dp(hyai, hybi, ps_v):
    """dp(k) = dhyai*ps0 + dhybi*ps_v (prim_driver_mod.F90:810-812) -> [nelem][nlev][4][4]"""
    da = np.diff(hyai) * P0; db = np.diff(hybi)
    return da[None, :, None, None] + db[None, :, None, None] * np.asarray(ps_v)[:, None, :, :]


R_EARTH = 6.37122e6


def layer_depths(zm):
    """dh(lev) of the norm script: rebuilt from the mid-level heights by its "2*(h-base)" recursion, from the surface up"""
    nlev = len(zm)
    dh = np.zeros(nlev); base = 0.0
    for i in range(1, nlev + 1):
        dh[nlev - i] = 2.0 * (zm[nlev - i] - base)
        base = base + dh[nlev - i]
    return dh


def _norm_columns(ne, lat, lon):
    """(cols, colw): the unique columns (flat point indices, ascending) and the horizontal weight of each, the script's
    R cos(lat) dlon * R dlat with dlon = dlat = the mean node spacing; both norm routes take their weights from here"""
    cols = unique_columns(lat, lon)
    if cols.size != 6 * ne * ne * 9 + 2:
        raise ValueError("expected %d unique columns, found %d" % (6 * ne * ne * 9 + 2, cols.size))
    latc = np.asarray(lat).reshape(-1)[cols]
    R = R_EARTH
    dlat = 0.5 * np.pi / (ne * 3)
    return cols, (R * np.cos(latc) * dlat) * (R * dlat)


def column_weights(ne, lat, lon, zm):
    """(owner, colw, dh) of tse_norm_setup for the WHOLE mesh (lat, lon [nelem][4][4]; a rank passes on the rows of its elements):
    owner[nelem][4][4] = 1 where the element's point is the owner of its GLL column (unique_columns), colw[nelem][4][4] = that column's
    horizontal weight (0 where owner = 0: never read), dh[nlev] = layer_depths(zm) -- the very numbers dcmip_norms multiplies"""
    cols, w = _norm_columns(ne, lat, lon)
    shape = np.asarray(lat).shape
    owner = np.zeros(np.asarray(lat).size, dtype=np.int32); colw = np.zeros(owner.size)
    owner[cols] = 1; colw[cols] = w
    return owner.reshape(shape), colw.reshape(shape), layer_depths(zm)


def dcmip_norms(ne, lat, lon, q_i, q_f, zm):
    nlev = q_i.shape[1]
    cols, colw = _norm_columns(ne, lat, lon)
    qi = np.moveaxis(q_i, 1, 0).reshape(nlev, -1)[:, cols]
    qf = np.moveaxis(q_f, 1, 0).reshape(nlev, -1)[:, cols]
    dh = layer_depths(zm)
    dV = colw[None, :] * dh[:, None]
    dq = qf - qi
    dev = np.abs(qi - qi.mean())
    return dict(L1=float((np.abs(dq) * dV).sum() / (dev * dV).sum()),
                L2=float(np.sqrt((dq * dq * dV).sum()) / np.sqrt((dev * dev * dV).sum())),
                Linf=float((np.abs(dq) * dV).max() / (dev * dV).max()),
                q_max=float(qf.max()), q_min=float(qf.min()))


def norms_from_partials(partials, gid, nelem, dist_mod=None, rank=0, world=1):
    """partials[n_local][8] (tse_norm_partials: one row per local element) -> the norm line's dict on rank 0 (None elsewhere): entries 0
    to 3 added exactly over all elements (math.fsum: no order, hence no dependence on the partition), entries 4 to 7 reduced by max / min;
    L1 = s0/s1, L2 = sqrt(s2)/sqrt(s3), Linf = m4/m5."""
    full = gather_by_gid(np.asarray(partials, dtype=np.float64), gid, nelem, dist_mod, rank, world)
    if full is None:
        return None
    s = [math.fsum(full[:, j].tolist()) for j in range(4)]
    return dict(L1=float(s[0] / s[1]), L2=float(np.sqrt(s[2]) / np.sqrt(s[3])), Linf=float(full[:, 4].max() / full[:, 5].max()),
                q_max=float(full[:, 6].max()), q_min=float(full[:, 7].min()))


# ---- numerical mixing and filaments (Lauritzen and Thuburn 2012, QJRMS 138, "Evaluating advection/transport schemes using interrelated
# tracers, scatter plots and numerical mixing diagnostics") ----
MIX_NB = 60      # bisection steps per interval (csrc/tse_kernels.h: MIX_NB)
MIX_NTAU = 24    # the most filament thresholds of one call
MIX_TAU = tuple(k / 100.0 for k in range(10, 101, 5))   # 0.10, 0.15, ..., 1.00 (the paper's thresholds)


def mixing_constants(xmin, xmax, c0, c2):
    """what tse_mix_partials derives from its arguments, each operation rounded once: dict(xmin, xmax, c0, c2, yhi = psi(xmin),
    ylo = psi(xmax), Rx, Ry, sl = the chord's slope, kk = (Ry*Ry)/(Rx*Rx), i2 = 1/(2*c2*c2)) for the curve psi(x) = c0 + c2*(x*x)"""
    xmin, xmax, c0, c2 = (np.float64(v) for v in (xmin, xmax, c0, c2))
    if not (xmax > xmin and c2 < 0):
        raise ValueError("mixing_constants: needs xmin < xmax and c2 < 0 (xmin = %r, xmax = %r, c2 = %r)" % (xmin, xmax, c2))
    yhi = c0 + c2 * (xmin * xmin); ylo = c0 + c2 * (xmax * xmax)
    Rx = xmax - xmin; Ry = yhi - ylo
    return dict(xmin=xmin, xmax=xmax, c0=c0, c2=c2, yhi=yhi, ylo=ylo, Rx=Rx, Ry=Ry, sl=(ylo - yhi) / Rx, kk=(Ry * Ry) / (Rx * Rx),
                i2=np.float64(1.0) / ((np.float64(2.0) * c2) * c2))


def mixing_distance(m, chi, xi):
    """d = sqrt(min over x in [xmin, xmax] of ((chi-x)/Rx)^2 + ((xi-psi(x))/Ry)^2): the normalised distance of (chi, xi) to the curve, by
    the device's algorithm (csrc/tse_kernels.h: mix_distance) operation for operation -- the stationary points are the roots of the cubic
    h(x) = (x*x + P)*x + Qc, bracketed by the break points xmin, clamp(-s), clamp(s), xmax, s = sqrt(max(-P/3, 0)), and found by MIX_NB
    bisection steps on each of the three intervals; the end points are candidates of their own"""
    chi = np.asarray(chi, np.float64); xi = np.asarray(xi, np.float64)
    xmin, xmax, c0, c2, Rx, Ry, kk, i2 = (m[k] for k in ("xmin", "xmax", "c0", "c2", "Rx", "Ry", "kk", "i2"))

    def g(x):
        a = (chi - x) / Rx; b = (xi - (c0 + c2 * (x * x))) / Ry
        return a * a + b * b
    P = (kk - (2.0 * c2) * (xi - c0)) * i2
    Qc = (-(chi * kk)) * i2

    def h(x):
        return (x * x + P) * x + Qc
    s = np.sqrt(np.maximum((-P) / 3.0, 0.0))
    b = [np.full_like(chi, xmin), np.minimum(np.maximum(-s, xmin), xmax), np.minimum(np.maximum(s, xmin), xmax), np.full_like(chi, xmax)]
    best = np.minimum(g(b[0]), g(b[3]))
    for i in range(3):
        lo, hi = b[i], b[i + 1]
        hl, hh = h(lo), h(hi)
        has = ((hl <= 0) & (hh >= 0)) | ((hl >= 0) & (hh <= 0))
        up = hh >= hl
        for _ in range(MIX_NB):
            mid = 0.5 * (lo + hi)
            right = (h(mid) < 0) == up
            lo = np.where(right, mid, lo); hi = np.where(right, hi, mid)
        best = np.where(has, np.minimum(best, g(0.5 * (lo + hi))), best)
    return np.sqrt(best)


def mixing_classes(m, chi, xi):
    """(A, B, C): real mixing (between the chord and the curve), range-preserving unmixing (the rest of the rectangle
    [xmin, xmax] x [ylo, yhi]) and overshooting (everything else), as boolean arrays; every point is in exactly one"""
    chi = np.asarray(chi, np.float64); xi = np.asarray(xi, np.float64)
    inx = (m["xmin"] <= chi) & (chi <= m["xmax"])
    chord = m["yhi"] + (chi - m["xmin"]) * m["sl"]; curve = m["c0"] + m["c2"] * (chi * chi)
    A = inx & (chord <= xi) & (xi <= curve)
    B = ~A & inx & (m["ylo"] <= xi) & (xi <= m["yhi"])
    return A, B, ~A & ~B


def mixing_diagnostics(ne, lat, lon, chi, xi, zm, xmin, xmax, c0, c2, tau, chi0=None):
    """dict(l_r, l_u, l_o, l_f=[...], d_max, counts=(nA, nB, nC)) from whole fields chi, xi [nelem][nlev][4][4] on the unique-column grid:
    l_r, l_u, l_o = sum over class A, B, C of d dV / sum dV with dcmip_norms' dV, l_f(tau) = 100 * ((sum of dV where chi >= tau) / (the same
    of chi0, the field at t0; default: chi itself)) -- the quotient first, so that an unchanged area gives exactly 100 --, 0.0 where the
    denominator is 0.  The terms are the device's in every bit; the sums are numpy's."""
    nlev = chi.shape[1]
    m = mixing_constants(xmin, xmax, c0, c2)
    cols, colw = _norm_columns(ne, lat, lon)
    x = np.moveaxis(chi, 1, 0).reshape(nlev, -1)[:, cols]
    y = np.moveaxis(xi, 1, 0).reshape(nlev, -1)[:, cols]
    dV = colw[None, :] * layer_depths(zm)[:, None]
    d = mixing_distance(m, x, y)
    cls = mixing_classes(m, x, y)
    ddV = d * dV
    V = dV.sum()
    x0 = x if chi0 is None else np.moveaxis(chi0, 1, 0).reshape(nlev, -1)[:, cols]
    l_f = []
    for t in np.asarray(tau, np.float64).reshape(-1):
        a0 = np.where(x0 >= t, dV, 0.0).sum()
        l_f.append(float(100.0 * (np.where(x >= t, dV, 0.0).sum() / a0)) if a0 != 0 else 0.0)
    return dict(l_r=float(np.where(cls[0], ddV, 0.0).sum() / V), l_u=float(np.where(cls[1], ddV, 0.0).sum() / V),
                l_o=float(np.where(cls[2], ddV, 0.0).sum() / V), l_f=l_f, d_max=float(d.max()),
                counts=tuple(int(c.sum()) for c in cls))


def mixing_from_partials(partials, partials0, gid, nelem, dist_mod=None, rank=0, world=1, ntau=MIX_NTAU):
    """partials, partials0 [n_local][32] (tse_mix_partials now and at t0: one row per local element) -> the dict of mixing_diagnostics on
    rank 0 (None elsewhere): entries 0 to 3 and 8.. added exactly over all elements (math.fsum: no order, hence no dependence on the
    partition), l_r, l_u, l_o = S0, S1, S2 / S3, l_f(tau_j) = 100 * (S(8+j)(t) / S(8+j)(t0)) (0.0 where the denominator is 0) for j < ntau,
    the counts added (small integers held in doubles: exact), d_max = the largest entry 7"""
    both = np.concatenate([np.asarray(partials, dtype=np.float64), np.asarray(partials0, dtype=np.float64)], axis=1)
    full = gather_by_gid(both, gid, nelem, dist_mod, rank, world)
    if full is None:
        return None
    now, then = full[:, :32], full[:, 32:]
    S = [math.fsum(now[:, j].tolist()) for j in range(4)]
    l_f = []
    for j in range(8, 8 + int(ntau)):
        a0 = math.fsum(then[:, j].tolist())
        l_f.append(float(100.0 * (math.fsum(now[:, j].tolist()) / a0)) if a0 != 0 else 0.0)
    return dict(l_r=float(S[0] / S[3]), l_u=float(S[1] / S[3]), l_o=float(S[2] / S[3]), l_f=l_f, d_max=float(now[:, 7].max()),
                counts=tuple(int(now[:, j].sum()) for j in (4, 5, 6)))


def tracer_mass(spheremp, qdp):
    return np.einsum("eji,eqkji->q", spheremp, qdp)


def printstate_lines(qdp, dp):
    """(min, max, sum) of Q = Qdp/dp per tracer, as the `qv=` lines print them"""
    q = qdp / dp[:, None]
    return [(float(q[:, t].min()), float(q[:, t].max()), float(q[:, t].sum())) for t in range(q.shape[1])]


STATS = 16                                                       # TSE_STATS
STATS_SUMS = (2, 3, 4, 5, 7, 8, 9, 10, 11, 14)                   # the entries of a tse_stats_view share that are sums
STATS_MINS, STATS_MAXS = (0,), (1, 6, 12, 13)


def stats_from_partials(parts, ref=False):
    """parts: the shares HipMod.stats_view returned, [n][nf][16] or [n][nf][nk][16] -- one array, or a list with one per rank -> dict of
    arrays [nf] or [nf][nk]: min, max, sum (prim_printstate's MIN, MAX, SUM), integral (global_integral: entry 3 over 4 pi), absmax,
    nonfinite (an int), mean (entry 3 over entry 14), area (entry 14 over 4 pi) and, with ref=True, l1, l2, linf combined exactly as
    l1_snorm, l2_snorm, linf_snorm combine their integrals and maxima (global_norms_mod.F90).  Sums over elements and ranks are
    math.fsum's (exact, then rounded once; a column that holds a NaN or inf, or whose sum overflows, is added by numpy and gives NaN or
    inf), extrema min / max: the same digits however the elements are dealt to ranks."""
    if isinstance(parts, np.ndarray):
        parts = [parts]
    x = np.concatenate([np.asarray(p, dtype=np.float64) for p in parts], axis=0)
    if x.ndim not in (3, 4) or x.shape[-1] != STATS:
        raise ValueError("stats_from_partials: shares of shape %s (want [n][nf][16] or [n][nf][nk][16])" % (x.shape,))
    shape = x.shape[1:-1]
    flat = x.reshape(x.shape[0], -1, STATS)
    tot = np.zeros((flat.shape[1], STATS))
    for c in range(flat.shape[1]):
        for j in STATS_SUMS:
            col = flat[:, c, j]
            try:
                tot[c, j] = math.fsum(col.tolist()) if np.isfinite(col).all() else col.sum()
            except OverflowError:          # finite shares whose sum is not: fsum raises where an addition gives inf
                with np.errstate(over="ignore"):
                    tot[c, j] = col.sum()
        for j in STATS_MINS:
            tot[c, j] = flat[:, c, j].min()
        for j in STATS_MAXS:
            tot[c, j] = flat[:, c, j].max()
    tot = tot.reshape(shape + (STATS,))
    four_pi = 4.0 * math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(min=tot[..., 0], max=tot[..., 1], sum=tot[..., 2], integral=tot[..., 3] / four_pi, absmax=tot[..., 6],
                   nonfinite=tot[..., 7].astype(np.int64), mean=tot[..., 3] / tot[..., 14], area=tot[..., 14] / four_pi)
        if ref:
            out["l1"] = (tot[..., 8] / four_pi) / (tot[..., 9] / four_pi)
            out["l2"] = np.sqrt(tot[..., 10] / four_pi) / np.sqrt(tot[..., 11] / four_pi)
            out["linf"] = tot[..., 12] / tot[..., 13]
    return out


def fortran_e(x, w=23, d=15):
    """Fortran's Ew.d of x: 0.ddd...E+ee right-justified in w columns, the d digits correctly rounded (Python's own '%.*e' conversion;
    only the point is moved).  A three-digit exponent drops the E (0.ddd+100), as Fortran does; -0.0 keeps its sign."""
    x = float(x)
    if x != x:
        body = "NaN"
    elif x in (math.inf, -math.inf):
        body = "Infinity" if x > 0 else "-Infinity"
    else:
        mant, exp = ("%.*e" % (d - 1, x)).split("e")
        sign = "-" if mant.startswith("-") else ""
        digits = mant.lstrip("-").replace(".", "")
        e = int(exp) + 1 if x != 0 else 0
        body = sign + "0." + digits + ("E%+03d" % e if abs(e) < 100 else "%+04d" % e)
    return body.rjust(w) if len(body) <= w else "*" * w


PRINTSTATE_LABELS = dict(u="u     = ", v="v     = ", T="T     = ", ps="ps= ", dp3d="dp3d  = ", omega="omega = ")


def printstate_field_lines(fields, mass=None, scale=1.0 / G):
    """prim_printstate's lines (prim_state_mod.F90:340-347, format 100 = A10,3(E23.15)) from device statistics.  fields: (name, stats)
    pairs in the order to print, stats a dict of stats_from_partials for ONE field without levels (min, max, sum scalars or arrays of
    one value); name one of u, v, T, ps, dp3d, omega or any label of up to 10 characters.  mass: the integral of ps_v
    (stats_from_partials(...)["integral"]) for the line "      M = " Mass kg/m^2 Mass2 mb, Mass = Mass2 * scale (scale = 1/g)."""
    lines = []
    for name, st in fields:
        label = PRINTSTATE_LABELS.get(name, name)
        lines.append("%10s" % label[:10] + "".join(fortran_e(np.asarray(st[k]).reshape(-1)[0]) for k in ("min", "max", "sum")))
    if mass is not None:
        m2 = float(np.asarray(mass).reshape(-1)[0])
        lines.append("      M = " + fortran_e(m2 * scale) + " kg/m^2" + fortran_e(m2) + " mb     ")
    return lines


def gather_by_gid(local, gid, nelem, dist_mod, rank, world):
    """local[n_local, ...] on every rank -> full[nelem, ...] in global element order on rank 0 (None elsewhere)"""
    if world == 1:
        full = np.empty((nelem,) + local.shape[1:], dtype=local.dtype)
        full[gid] = local
        return full
    parts = [None] * world if rank == 0 else None
    dist_mod.gather_object((np.asarray(gid), np.ascontiguousarray(local)), parts, dst=0)
    if rank != 0:
        return None
    full = np.empty((nelem,) + local.shape[1:], dtype=local.dtype)
    for g, x in parts:
        full[g] = x
    return full


def global_sum(partials, gid, nelem, dist_mod=None, rank=0, world=1):
    """partials[n_local][m] (one row per local element, formed in a fixed order) -> [m] exact global sums on rank 0"""
    full = gather_by_gid(np.asarray(partials, dtype=np.float64), gid, nelem, dist_mod, rank, world)
    if full is None:
        return None
    return np.array([math.fsum(full[:, j].tolist()) for j in range(full.shape[1])])


def element_q_partials(qdp, dp):
    """per element and tracer: (min, max, sum) of Q = Qdp/dp, the sum over the element's points in a fixed (row) order"""
    q = (qdp / dp[:, None]).reshape(qdp.shape[0], qdp.shape[1], -1)
    return q.min(2), q.max(2), q.sum(2)
