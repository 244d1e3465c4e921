"""A NumPy statement of the reference's cumulus mixing of the tracers, cumtran2 (Main/chemlib/
mod_che_cumtran.F90:118-167), written from the Fortran text, with the pseudo-tendency it books into
cconvdiag when ichdiag > 0 (:124-130, 159-166).  Test infrastructure: tests/test_tracer_diag_gpu.py
compares the engine's k_tr_cumtran with it bit for bit, tests/test_tracer_diag_cpu.py checks it against
the plain quadruple loop of the text (cumtran2_loops) and checks the input generator both use.

Vectorised over (j, i), with an explicit loop over k: every column adds its own levels kctop .. kz in
ascending order, so deltas and the two means are summed in the text's order.  Every expression keeps the
text's operation order (left to right) in float64; the chain has no transcendental function.

Arrays are (k, i, j) with the Fortran point (j, i, k) at [k - 1, i - 1, j - 1]; the 2-D inputs (i, j).
"""
import numpy as np


def dsigma(rc):
    """dsigma(k) = sigma(k + 1) - sigma(k) (Main/mod_params.F90), [k - 1]."""
    sig = np.asarray(rc.sigma, dtype=np.float64)
    return sig[1:] - sig[:-1]


def interior(rc):
    """The (i, j) slices of jci x ici; a band keeps every j."""
    return slice(1, rc.iy - 2), (slice(None) if rc.i_band else slice(1, rc.jx - 2))


def cumtran2(rc, amxc, bmxc, dotran, kcumtop, convcldfra, dt=None, cfdout=None):
    """cumtran2 on one tracer's atm1 (amxc) and atm2 (bmxc): (new atm1, new atm2, conv).  conv is the
    term cconvdiag gains, (bmxc_after - bmxc_before) / dt * 2 * cfdout on jci x ici and zero elsewhere
    (None without dt and cfdout)."""
    kz = rc.kz
    ds = dsigma(rc)
    I, J = interior(rc)
    a, b = amxc[:, I, J].copy(), bmxc[:, I, J].copy()
    frc = convcldfra[:, I, J]
    ktop = kcumtop[I, J].astype(np.int64)
    act = (dotran[I, J] != 0.0) & (ktop > 0)
    kctop = np.maximum(ktop, 4)
    deltas = np.zeros(ktop.shape)
    chiabar = np.zeros(ktop.shape)
    chibbar = np.zeros(ktop.shape)
    for k in range(1, kz + 1):                      # the Fortran level
        m = act & (k >= kctop)
        deltas = np.where(m, deltas + ds[k - 1], deltas)
        chiabar = np.where(m, chiabar + a[k - 1] * ds[k - 1], chiabar)
        chibbar = np.where(m, chibbar + b[k - 1] * ds[k - 1], chibbar)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(1, kz + 1):
            m = act & (k >= kctop)
            cumfrc = frc[k - 1]
            a[k - 1] = np.where(m, a[k - 1] * (1.0 - cumfrc) + cumfrc * chiabar / deltas, a[k - 1])
            b[k - 1] = np.where(m, b[k - 1] * (1.0 - cumfrc) + cumfrc * chibbar / deltas, b[k - 1])
    an, bn = amxc.copy(), bmxc.copy()
    an[:, I, J] = a
    bn[:, I, J] = b
    conv = None
    if dt is not None:
        conv = np.zeros(bmxc.shape)
        conv[:, I, J] = (b - bmxc[:, I, J]) / dt * 2.0 * cfdout
    return an, bn, conv


def cumtran2_loops(rc, amxc, bmxc, dotran, kcumtop, convcldfra, dt, cfdout):
    """The same as the plain loops of the text (one tracer: the loop over n is the caller's)."""
    kz, iy, jx = rc.kz, rc.iy, rc.jx
    ds = [float(x) for x in dsigma(rc)]
    an, bn = amxc.copy(), bmxc.copy()
    conv = np.zeros(bmxc.shape)
    for i in range(2, iy - 1):                       # ici1 .. ici2, Fortran indices
        for j in range(2, jx - 1):                   # jci1 .. jci2
            if not dotran[i - 1, j - 1]:
                continue
            if kcumtop[i - 1, j - 1] > 0:
                deltas = 0.0
                chiabar = 0.0
                chibbar = 0.0
                kctop = max(int(kcumtop[i - 1, j - 1]), 4)
                for k in range(kctop, kz + 1):
                    deltas = deltas + ds[k - 1]
                    chiabar = chiabar + float(an[k - 1, i - 1, j - 1]) * ds[k - 1]
                    chibbar = chibbar + float(bn[k - 1, i - 1, j - 1]) * ds[k - 1]
                for k in range(kctop, kz + 1):
                    cumfrc = float(convcldfra[k - 1, i - 1, j - 1])
                    an[k - 1, i - 1, j - 1] = float(an[k - 1, i - 1, j - 1]) * (1.0 - cumfrc) + cumfrc * chiabar / deltas
                    bn[k - 1, i - 1, j - 1] = float(bn[k - 1, i - 1, j - 1]) * (1.0 - cumfrc) + cumfrc * chibbar / deltas
    for i in range(2, iy - 1):
        for j in range(2, jx - 1):
            for k in range(1, kz + 1):
                conv[k - 1, i - 1, j - 1] = (float(bn[k - 1, i - 1, j - 1]) - float(bmxc[k - 1, i - 1, j - 1])) / dt * 2.0 * cfdout
    return an, bn, conv


def inputs(rc, seed=11):
    """(dotran, kcumtop, convcldfra) as (iy, jx), (iy, jx), (kz, iy, jx) arrays that populate every
    branch of cumtran2 on the interior columns: no transport (dotran false), no convection
    (kcumtop = 0), a cloud top above level 4 (kcumtop in 1 .. 3: the clamp), a one-level cloud
    (kcumtop = kz), columns whose cloud fraction is exactly 0 and exactly 1, and the general case
    (kcumtop in 4 .. kz - 1, fractions inside (0, 1))."""
    rng = np.random.default_rng(seed)
    kz, shape = rc.kz, (rc.iy, rc.jx)
    dotran = (rng.uniform(size=shape) >= 0.15).astype(np.float64)
    u = rng.uniform(size=shape)
    ktop = rng.integers(4, kz, size=shape).astype(np.float64)          # 4 .. kz - 1
    ktop[u < 0.20] = 0.0
    sel = (u >= 0.20) & (u < 0.35)
    ktop[sel] = rng.integers(1, 4, size=shape).astype(np.float64)[sel]
    ktop[(u >= 0.35) & (u < 0.45)] = float(kz)
    frc = rng.uniform(0.02, 0.98, size=(kz,) + shape)
    v = rng.uniform(size=shape)
    frc[:, v < 0.10] = 0.0
    frc[:, (v >= 0.10) & (v < 0.20)] = 1.0
    return dotran, ktop, frc


def branch_shares(rc, dotran, ktop, frc):
    """The share of the interior columns on each branch of cumtran2, by name."""
    I, J = interior(rc)
    d, k, f = dotran[I, J], ktop[I, J], frc[:, I, J]
    n = float(d.size)
    return {"dotran false": (d == 0.0).sum() / n, "kcumtop = 0": (k == 0.0).sum() / n,
            "kcumtop in 1..3": ((k >= 1.0) & (k <= 3.0)).sum() / n, "kcumtop = kz": (k == float(rc.kz)).sum() / n,
            "cumfrc = 0": (f == 0.0).all(axis=0).sum() / n, "cumfrc = 1": (f == 1.0).all(axis=0).sum() / n}
