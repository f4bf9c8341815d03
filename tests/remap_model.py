"""remap_Q_ppm (prim_advection_mod.F90:98-356) restated in numpy for ANY level count, vectorised over tracers and the 16 points of
a column.  The operations and their order are those of the reference (and of oracle/tse_oracle.c:orc_remap_q_ppm, which is
fixed at 72 levels): tests/test_nlev_cpu.py holds this model to pyoracle.remap_q_ppm at 72 levels, and the 64-level tests hold
the 64-level library to it.  vert_remap_q_alg 0|1: mirrored ghost cells; 2: piecewise-constant end cells (:336-341)."""
import numpy as np

GS = 2   # ghost cells on either end


def _grids(dpo, nlev):
    """compute_ppm_grids (:221-260): dpo[j + 1], j = -1..nlev+2, shape (nlev + 4, P) -> r[j][0..9], j = 0..nlev+1"""
    def DX(j):
        return dpo[j + 1]
    r = np.zeros((nlev + 2, 10) + dpo.shape[1:])
    for j in range(nlev + 2):
        r[j, 0] = DX(j) / (DX(j - 1) + DX(j) + DX(j + 1))
        r[j, 1] = (2. * DX(j - 1) + DX(j)) / (DX(j + 1) + DX(j))
        r[j, 2] = (DX(j) + 2. * DX(j + 1)) / (DX(j - 1) + DX(j))
    for j in range(nlev + 1):
        r[j, 3] = DX(j) / (DX(j) + DX(j + 1))
        r[j, 4] = 1. / (DX(j - 1) + DX(j) + DX(j + 1) + DX(j + 2))
        r[j, 5] = (2. * DX(j + 1) * DX(j)) / (DX(j) + DX(j + 1))
        r[j, 6] = (DX(j - 1) + DX(j)) / (2. * DX(j) + DX(j + 1))
        r[j, 7] = (DX(j + 2) + DX(j + 1)) / (2. * DX(j + 1) + DX(j))
        r[j, 8] = DX(j) * (DX(j - 1) + DX(j)) / (2. * DX(j) + DX(j + 1))
        r[j, 9] = DX(j + 1) * (DX(j + 1) + DX(j + 2)) / (DX(j) + 2. * DX(j + 1))
    return r


def _ppm(a, dx, nlev, alg):
    """compute_ppm (:264-341): a[j + 1], j = -1..nlev+2, shape (nlev + 4, Q, P) -> coefs[j][0..2], j = 1..nlev"""
    def A(j):
        return a[j + 1]
    dma = np.zeros((nlev + 2,) + a.shape[1:])
    for j in range(nlev + 2):
        da = dx[j, 0] * (dx[j, 1] * (A(j + 1) - A(j)) + dx[j, 2] * (A(j) - A(j - 1)))
        m = np.abs(da)
        m = np.minimum(m, 2. * np.abs(A(j) - A(j - 1)))
        m = np.minimum(m, 2. * np.abs(A(j + 1) - A(j)))
        d = np.where(np.signbit(da), -m, m)
        dma[j] = np.where((A(j + 1) - A(j)) * (A(j) - A(j - 1)) <= 0., 0., d)
    ai = np.zeros((nlev + 1,) + a.shape[1:])
    for j in range(nlev + 1):
        ai[j] = A(j) + dx[j, 3] * (A(j + 1) - A(j)) + \
            dx[j, 4] * (dx[j, 5] * (dx[j, 6] - dx[j, 7]) * (A(j + 1) - A(j)) - dx[j, 8] * dma[j + 1] + dx[j, 9] * dma[j])
    coefs = np.zeros((nlev + 1, 3) + a.shape[1:])
    for j in range(1, nlev + 1):
        al, ar, aj = ai[j - 1], ai[j], A(j)
        flat = (ar - aj) * (aj - al) <= 0.
        al = np.where(flat, aj, al); ar = np.where(flat, aj, ar)
        lo = (ar - al) * (aj - (al + ar) / 2.) > (ar - al) * (ar - al) / 6.
        al = np.where(lo, 3. * aj - 2. * ar, al)
        hi = (ar - al) * (aj - (al + ar) / 2.) < -((ar - al) * (ar - al)) / 6.
        ar = np.where(hi, 3. * aj - 2. * al, ar)
        coefs[j, 0] = 1.5 * aj - (al + ar) / 4.
        coefs[j, 1] = ar - al
        coefs[j, 2] = -6. * aj + 3. * (al + ar)
    if alg == 2:
        for j in (1, 2, nlev - 1, nlev):
            coefs[j, 0] = A(j); coefs[j, 1] = 0.; coefs[j, 2] = 0.
    return coefs


def _parabola(c, x1, x2):
    return c[0] * (x2 - x1) + c[1] * (x2 * x2 - x1 * x1) / 0.2e1 + c[2] * (x2 * x2 * x2 - x1 * x1 * x1) / 0.3e1


def remap_q_ppm(Qdp, dp1, dp2, alg=0):
    """Qdp[q][k][4][4], dp1/dp2[k][4][4] -> remapped copy (any nlev = Qdp.shape[1])"""
    Qdp = np.asarray(Qdp, dtype=np.float64)
    nq, nlev = Qdp.shape[0], Qdp.shape[1]
    Q = Qdp.reshape(nq, nlev, 16)
    d1 = np.asarray(dp1, dtype=np.float64).reshape(nlev, 16)
    d2 = np.asarray(dp2, dtype=np.float64).reshape(nlev, 16)
    P = 16
    # index j = 1-GS..nlev+GS at [j + 1] (as the oracle's ao_/dpo_): valid for j >= -1
    dpo = np.zeros((nlev + 2 * GS, P))
    pio = np.zeros((nlev + 3, P)); pin = np.zeros((nlev + 2, P))
    for k in range(1, nlev + 1):
        dpo[k + 1] = d1[k - 1]
        pin[k + 1] = pin[k] + d2[k - 1]
        pio[k + 1] = pio[k] + dpo[k + 1]
    pio[nlev + 2] = pio[nlev + 1] + 1.
    pin[nlev + 1] = pio[nlev + 1]
    for k in range(1, GS + 1):
        dpo[1 - k + 1] = dpo[k + 1]; dpo[nlev + k + 1] = dpo[nlev + 1 - k + 1]
    kid = np.zeros((nlev + 1, P), dtype=np.int64)
    z2 = np.zeros((nlev + 1, P))
    cols = np.arange(P)
    for k in range(1, nlev + 1):
        for p in range(P):
            kk = k
            while pio[kk, p] <= pin[k + 1, p]:
                kk += 1
            kk -= 1
            if kk == nlev + 1:
                kk = nlev
            kid[k, p] = kk
        kk = kid[k]
        z2[k] = (pin[k + 1] - (pio[kk, cols] + pio[kk + 1, cols]) * 0.5) / dpo[kk + 1, cols]
    dx = _grids(dpo, nlev)
    # tracers
    ao = np.zeros((nlev + 2 * GS, nq, P))
    masso = np.zeros((nlev + 2, nq, P))
    for k in range(1, nlev + 1):
        ao[k + 1] = Q[:, k - 1]
        masso[k + 1] = masso[k] + ao[k + 1]
        ao[k + 1] = ao[k + 1] / dpo[k + 1]
    for k in range(1, GS + 1):
        ao[1 - k + 1] = ao[k + 1]; ao[nlev + k + 1] = ao[nlev + 1 - k + 1]
    coefs = _ppm(ao, dx[:, :, None, :], nlev, alg)
    out = np.empty_like(Q)
    massn1 = np.zeros((nq, P))
    for k in range(1, nlev + 1):
        kk = kid[k]
        c = coefs[kk, :, :, cols].transpose(1, 2, 0)                    # [3][q][p] of cell kk(p)
        massn2 = masso[kk, :, cols].T + _parabola(c, -0.5, z2[k]) * dpo[kk + 1, cols]
        out[:, k - 1] = massn2 - massn1
        massn1 = massn2
    return out.reshape(Qdp.shape)
