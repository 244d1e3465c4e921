"""The serial part of the negative-moisture fix (regcm_amd/csrc/qxcommon.hpp) against the oracle's
plain serial loop (qx_forecast_fix, oracle/rcm_oracle.c; Main/mod_tendency.F90:382-393) on every
path and launch site, at the shapes where each can go wrong.

The fix has three algorithms: the row sweep on LDS (negfix_sweep), the same sweep without LDS
(lane 0 reads memory) and the dense skewed wavefront (negfix_dense_dpp) with its LDS ring between
wavefronts; negfix_resolve takes the wavefront for a plane with more than NEGFIX_SPARSE = 16
marked rows when the block holds a thread per row (R <= 512).  The grids are small and odd-shaped
so that a plane is more than one wavefront of rows (R > 64), more than one 64-column chunk
(W > 64), taller than the largest block (R = 513) or wider than k_split_project's LDS (W = 741);
the moisture fields are synthetic sign patterns, one per level, that make every predecessor
combination, the longest chain, both sides of the threshold and forecasts small enough for the
`xs < 2^-960` branch beside div_by.

Every case asserts from the oracle's own pre-fix forecast (never from the engine) that its data
reach what the case is for: `Marks` restates the marking rule and `Marks.takes_wavefront` the
integer comparisons of negfix_resolve.  Every case runs with two forms of atm1 (patterned_state):
with atm1 = atm2 the RAW filter floors every fixed point of the single-level patterns at zero, so
the state shows only where the fix acted; with a positive atm1 it shows what the fix computed,
which `check_visible` asserts on the oracle.  A second pattern set (supplement_field) adds what
the first cannot reach: a sweep that must not trust its previous-row buffer.

Tolerances are the suite's: the moisture chain of qc / qi / qr / qs has no transcendental
function, so after one step their interior is bit-identical to the oracle; qv's tendency is not
bit-exact (QVTEN, tests/test_parity_gpu.py), so its patterned levels are held to 1e-12 of that
level's own maximum (the fixed values lie orders of magnitude below the field's maximum, which a
whole-field norm would hide); the other fields to 1e-12 (hydrostatic) and 1e-11 (NH) after one
step, the patterned levels to 1e-11 after three.
"""
import numpy as np
import pytest

from tests.support import case, oracle, pair, relerr, state_names

pytestmark = pytest.mark.gpu

NEGFIX_SPARSE = 16          # qxcommon.hpp
NEGFIX_MAX_BLOCK = 512      # negfix_threads (engine.hpp): the largest block, a thread per row
TINY = 2.0 ** -960          # below it negfix_dense_dpp divides plainly instead of div_by
DEEP = 2.0 ** -1010         # the sums of supplement_field's deep stack lie below it

# grid name -> (jx, iy): R = iy - 3 interior rows, W = jx - 3 interior columns
GRIDS = {"G1": (24, 67), "G2": (24, 68), "G3": (24, 132), "G4": (70, 68), "G5": (24, 515), "G6": (24, 516),
         "G7": (744, 24)}

# the oracle's total tendency of each species: a field, or a work array of the nqx = 5 chain
TENDENCY = {"QV": "QVTEN", "QC": "QCTEN", "QI": "qteni", "QR": "qtenr", "QS": "qtens"}


# ------------------------------------------------------------------------------- the inputs
def grid_case(core, grid, nqx, band=False):
    """(rc, data) of one grid, generated once and never modified."""
    jx, iy = GRIDS[grid]
    return case("N1" if core == "nh" else "C1", jx=jx, iy=iy, nspgx=None, nspgd=None,
                ipptls=2 if nqx == 5 else 1, i_band=1 if band else 0)[:2]


# the single-level patterns (True: negative) on the global (i, j) index planes
def _whole(i, j):
    return np.ones(i.shape, dtype=bool)


def _checker(i, j):
    return (i + j) % 2 == 1


def _columns(i, j):
    return j % 2 == 1


def _rows(i, j):
    return i % 2 == 1


def _rows_n(n):
    # row stripes on the first n odd rows (interior rows 0, 2, .. 2 (n - 1)): exactly n marked rows
    return lambda i, j: (i % 2 == 1) & (i <= 2 * n - 1)


SINGLES = [("whole", _whole), ("checker", _checker), ("columns", _columns), ("rows", _rows),
           ("thr16", _rows_n(NEGFIX_SPARSE)), ("thr17", _rows_n(NEGFIX_SPARSE + 1))]


def pattern_levels(kz, s):
    """The levels of species number s: six single-level patterns on every other level (rotated
    with s, so each species has a pattern on a different level) and the stack of six tiny levels,
    below them for even s and above them for odd s; an untouched level between any two."""
    assert kz >= 18
    single0, tiny0 = (0, 12) if s % 2 == 0 else (7, 0)
    lev = {name: single0 + 2 * ((p + s) % len(SINGLES)) for p, (name, _) in enumerate(SINGLES)}
    lev["tiny"] = list(range(tiny0, tiny0 + 6))
    return lev


def pattern_field(rc, s, only=None):
    """q (kz, iy, jx) of species number s: +1e-5, -1e-5 where a single-level pattern says so
    (the boundary ring included) and -1e-300 on the tiny stack.  only: the patterns to keep."""
    lev = pattern_levels(rc.kz, s)
    i, j = np.meshgrid(np.arange(rc.iy), np.arange(rc.jx), indexing="ij")
    q = np.full((rc.kz, rc.iy, rc.jx), 1.0e-5)
    for name, fn in SINGLES:
        if only is None or name in only:
            q[lev[name]] = np.where(fn(i, j), -1.0e-5, 1.0e-5)
    if only is None or "tiny" in only:
        q[lev["tiny"]] = -1.0e-300
    return q, lev


def _skip(i, j):
    """Period 4 in the interior rows r and columns c: row 0 negative at c = 1, 2 (the second
    dependent: a marked row whose fixed value at c = 2 stays in the sweep's row buffer), row 1
    positive, row 2 negative at c = 2 alone (independent: the row is not marked), row 3 negative
    at c = 2 (dependent on the point below it).  The sweep comes to row 3 from row 0 and must
    take the parallel pass's value of row 2, not row 0's stale one: its `last == i - 1` test."""
    r, c = (i - 1) % 4, (j - 1) % 4
    return ((r == 0) & ((c == 1) | (c == 2))) | ((r >= 2) & (c == 2))


def supplement_field(rc, s):
    """The second pattern set, beyond the first's six: the skip pattern on two levels (1 + s % 2
    and 3 + s % 2 for species s) and a stack of six levels at -1e-307, whose 0.01 * sum lies near
    2^-1017 and whose fixed values near 2^-1020, the last binades above the subnormals, far below
    the wavefront's 2^-960 bound for div_by (fastmath.hpp).  That bound is a cautious one: for the
    divisor 9, q = RN(x / 9) and the remainder x - 9 q are multiples of the subnormal spacing
    whenever x is small, so the remainder stays exact and div_by returns x / 9 correctly rounded
    all the way down (an exact rational emulation of 50 000 operands at each of seven magnitudes
    from 2^-900 to 2^-1072 finds no difference).  An engine that took div_by there would
    therefore pass these levels too; what they pin is that both branches agree with the oracle's
    division at the bottom of the range."""
    lev = {"skip": [1 + s % 2, 3 + s % 2], "deep": list(range(6, 12))}
    i, j = np.meshgrid(np.arange(rc.iy), np.arange(rc.jx), indexing="ij")
    q = np.full((rc.kz, rc.iy, rc.jx), 1.0e-5)
    q[lev["skip"]] = np.where(_skip(i, j), -1.0e-5, 1.0e-5)
    q[lev["deep"]] = -1.0e-307
    return q, lev


def patterned_state(rc, data, qv=False, supplement=False, atm1="signed"):
    """The generated state with the patterns in qc (nqx = 2) or qc, qi, qr, qs (nqx = 5); qv: also
    the whole-plane and checkerboard levels in qv, its other levels kept.  atm2 = q p*.  atm1 =
    q p* as well ("signed"), or |q| p* ("positive").  The forecast atm2 + dt * tendency keeps q's
    signs either way, but the RAW filter after the fix floors its results at zero: with atm1 = atm2
    = -a at a fixed point the new atm2 is -a + 0.53 gnu2 (f + a) < 0 and the new atm1 is f - 0.47
    gnu2 (f + a), negative too unless the fixed value f exceeds 0.03 a (0.05 a on the NH core),
    and f is 0.01 of the mean of nine magnitudes near a.  So the signed form leaves zero at every
    fixed point of the single-level patterns whatever the fix computed, and shows the fix only
    through its marks and on part of the tiny stack; with a positive atm1 both new levels stay
    positive and carry f at every fixed point (`visible` counts them on the oracle)."""
    assert atm1 in ("signed", "positive")
    st = {k: v.copy() for k, v in data["state"].items()}
    ps = st["PSA"][0]
    levels = {}
    for s, nm in enumerate(["QC"] if rc.nqx == 2 else ["QC", "QI", "QR", "QS"]):
        q, levels[nm] = supplement_field(rc, s) if supplement else pattern_field(rc, s)
        q[:, rc.iy - 1, :] = 0.0
        if not rc.i_band:
            q[:, :, rc.jx - 1] = 0.0
        st[f"ATM1_{nm}"] = (np.abs(q) if atm1 == "positive" else q) * ps[None]
        st[f"ATM2_{nm}"] = q * ps[None]
    if qv:
        q, lev = pattern_field(rc, 0, only=("whole", "checker"))
        levels["QV"] = {n: lev[n] for n in ("whole", "checker")}
        for name in ("ATM1_QV", "ATM2_QV"):
            for k in levels["QV"].values():
                st[name][k] = (np.abs(q[k]) if atm1 == "positive" and name == "ATM1_QV" else q[k]) * ps
    return st, levels


# ------------------------------------------------- the marking rule, restated on the oracle
class Marks:
    """Of one species' pre-fix forecast cq (kz, iy, jx) on one tile: neg / dep (kz, R, W), the
    negative and the dependent negative interior points (a negative sweep-predecessor (j-1, i),
    (j-1, i-1), (j, i-1) or (j+1, i-1) inside the tile's interior, as negfix_dependent), rows
    (kz, R) the marked rows, and up (kz, R, W): dependent through a predecessor on row i - 1."""

    def __init__(self, cq, rc, nproc=(1, 1), tile=0):
        from regcm_amd.dycore import tile_extent
        ext, bdy = tile_extent(rc.jx, rc.iy, nproc[0], nproc[1], tile, i_band=rc.i_band)
        j1, j2, i1, i2 = ext[4] + bdy[0], ext[5] - bdy[1], ext[6] + bdy[2], ext[7] - bdy[3]   # 1-based
        self.cq = cq[:, i1 - 2: i2 + 1, :]                     # rows i1 - 1 .. i2 + 1 (the sums' ring)
        self.j1, self.j2 = j1, j2
        self.interior = (slice(None), slice(i1 - 1, i2), slice(j1 - 1, j2))
        self.neg = cq[:, i1 - 1: i2, j1 - 1: j2] < 0
        p = np.pad(self.neg, ((0, 0), (1, 0), (1, 1)))
        above = p[:, :-1, :-2] | p[:, :-1, 1:-1] | p[:, :-1, 2:]
        self.up = self.neg & above
        self.dep = self.neg & (above | p[:, 1:, :-2])
        self.rows = self.dep.any(axis=2)
        self.R, self.W = self.neg.shape[1:]

    def nmarked(self):
        return self.rows.sum(axis=1)

    def takes_wavefront(self, force_sweep):
        """Per plane: negfix_resolve's choice (mode == 0, nm > NEGFIX_SPARSE, R <= the block's
        threads; the launch sizes the LDS for the ring whenever the block holds the rows)."""
        if force_sweep or self.R > NEGFIX_MAX_BLOCK:
            return np.zeros(self.rows.shape[0], dtype=bool)
        return self.nmarked() > NEGFIX_SPARSE

    def ring_boundaries(self, planes, col0=0):
        """The 64-row boundaries b inside R at which some plane of `planes` holds a dependent
        negative on row b (at an interior column index >= col0) with a negative predecessor on
        row b - 1 (lane 0 of wavefront b / 64 takes it from the ring), and all the boundaries
        there are."""
        every = list(range(64, self.R, 64))
        return [b for b in every if self.up[planes][:, b, col0:].any()], every

    def tiny_sums(self, bound=TINY):
        """Dependent negatives whose 0.01 * (the nine |q| summed) is below `bound` whatever the
        predecessors were fixed to: a fixed value is 0.01 / 9 of nine magnitudes, each a forecast
        of the plane (ring included) or an earlier fixed value, so by induction along the sweep no
        larger than M, the plane's largest forecast magnitude, and the sum is at most 0.09 M."""
        big = np.abs(self.cq).max(axis=(1, 2))
        return int(self.dep[0.09 * big < bound].sum())

    def visible(self, new1, new2):
        """Dependent negatives at which the filtered state (the new atm1, atm2) is not floored at
        zero on both levels, so that a comparison of the state sees the fixed value."""
        return int((self.dep & ((new1[self.interior] != 0) | (new2[self.interior] != 0))).sum())

    def skipped_rows(self, planes):
        """Dependent negatives of `planes` on a marked row i whose negative predecessor lies on an
        unmarked row i - 1 at a column where the marked row before those two holds a fixed value
        (the stale value a sweep without the `last == i - 1` test would take)."""
        n = 0
        for k in np.flatnonzero(planes):
            marked = np.flatnonzero(self.rows[k])
            for r0, r in zip(marked[:-1], marked[1:]):
                if r - r0 < 2:
                    continue
                stale = np.pad(self.neg[k, r - 1] & self.dep[k, r0], 1)
                n += int((self.dep[k, r] & (stale[:-2] | stale[1:-1] | stale[2:])).sum())
        return n


def forecasts(o, a2, species):
    """The oracle's pre-fix forecast atm2 + dt * (total tendency) of each species after a tend
    (the interior; the ring keeps atm2 as qx_forecast_fix leaves it)."""
    dt = o.get_time()[1]
    out = {}
    for nm in species:
        ten = o.get(TENDENCY[nm]) if TENDENCY[nm].isupper() else o.get_work(TENDENCY[nm])
        cq = a2[nm].copy()
        ii, jj = slice(1, o.rc.iy - 2), (slice(None) if o.rc.i_band else slice(1, o.rc.jx - 2))
        cq[:, ii, jj] = a2[nm][:, ii, jj] + dt * ten[:, ii, jj]
        out[nm] = cq
    return out


def check_claims(label, marks, levels, claims, force_sweep, dense_species):
    """Assert from the oracle's forecasts what the case claims to exercise; marks: {species:
    [Marks per tile]}.  Prints the figures each assertion rests on."""
    dense_rows, chunk, tiny, tall, skipped, deep_wf = 0, 0, 0, 0, 0, 0
    ring_hit, ring_all, ring_wrap = set(), set(), set()
    for nm, tiles in marks.items():
        for m in tiles:
            wf = m.takes_wavefront(force_sweep or nm not in dense_species)
            if wf.any():
                dense_rows = max(dense_rows, int(m.nmarked()[wf].max()))
                hit, every = m.ring_boundaries(wf)
                ring_hit |= set(hit)
                ring_all |= set(every)
                ring_wrap |= set(m.ring_boundaries(wf, 64)[0])
            sweep = ~wf & (m.nmarked() > 0)
            chunk += int(m.dep[sweep][:, :, 64:].sum())
            tiny += m.tiny_sums()
            skipped += m.skipped_rows(sweep)
            deep_wf += int(m.dep[wf & (0.09 * np.abs(m.cq).max(axis=(1, 2)) < DEEP)].sum())
            if m.R > NEGFIX_MAX_BLOCK:           # the sweep's bitmap words past the largest block's rows
                tall += int(m.rows[m.nmarked() > NEGFIX_SPARSE][:, NEGFIX_MAX_BLOCK:].sum())
    m0 = {nm: tiles[0] for nm, tiles in marks.items()}
    thr = {nm: (int(m.nmarked()[levels[nm]["thr16"]]), int(m.nmarked()[levels[nm]["thr17"]]))
           for nm, m in m0.items() if "thr16" in levels.get(nm, {})}
    print(f"{label}: marked rows per plane (max) "
          f"{ {nm: int(max(m.nmarked().max() for m in t)) for nm, t in marks.items()} }, dependent points "
          f"{ {nm: int(sum(m.dep.sum() for m in t)) for nm, t in marks.items()} }, densest wavefront plane "
          f"{dense_rows} rows, ring boundaries {sorted(ring_hit)} of {sorted(ring_all)}, dependent points at "
          f"columns >= 64 on sweep planes {chunk}, threshold levels {thr}, tiny sums {tiny}, ring boundaries "
          f"met at columns >= 64 {sorted(ring_wrap)}, marked rows past row 512 of densely marked planes {tall}, "
          f"sweep points behind a skipped row {skipped}, sums below 2^-1010 on wavefront planes {deep_wf}")
    assert sum(int(m.dep.sum()) for t in marks.values() for m in t) > 0, label
    if "dense" in claims:
        assert dense_rows > NEGFIX_SPARSE, (label, dense_rows)
    if "ring" in claims:
        assert ring_all and ring_hit == ring_all, (label, sorted(ring_hit), sorted(ring_all))
    if "ringwrap" in claims:
        assert ring_all and ring_wrap == ring_all, (label, sorted(ring_wrap), sorted(ring_all))
    if "tall" in claims:
        assert tall > 0, label
    if "skip" in claims:
        assert skipped > 0, label
    if "deep" in claims:
        assert deep_wf > 0, label
    if "qv" in claims:
        per_level = {n: int(marks["QV"][0].dep[k].sum()) for n, k in levels["QV"].items()}
        print(f"{label}: qv dependent negatives per patterned level {per_level}")
        assert all(v > 0 for v in per_level.values()), (label, per_level)
    if "chunk" in claims:
        assert chunk > 0, label
    if "threshold" in claims:
        assert thr and all(v == (NEGFIX_SPARSE, NEGFIX_SPARSE + 1) for v in thr.values()), (label, thr)
    if "tiny" in claims:
        assert tiny > 0, label


# --------------------------------------------------------------------------------- the cases
def species_of(rc, qv=False):
    return (["QV"] if qv else []) + (["QC"] if rc.nqx == 2 else ["QC", "QI", "QR", "QS"])


def claims_of(grid, force_sweep):
    """What a one-tile case on `grid` reaches.  The threshold pair needs 33 interior rows; the
    wavefront a block with a thread per row; the ring more than one wavefront of rows; the
    sweep's second chunk more than 64 interior columns on a plane the sweep takes."""
    jx, iy = GRIDS[grid]
    R, W = iy - 3, jx - 3
    c = {"tiny"}
    if R >= 2 * NEGFIX_SPARSE + 1:
        c.add("threshold")
    if not force_sweep and R <= NEGFIX_MAX_BLOCK:
        c.add("dense")
        if R > 64:
            c.add("ring")
            if W > 64:
                c.add("ringwrap")         # the ring's slot index (column & 63) wraps
    if R > NEGFIX_MAX_BLOCK:
        c.add("tall")                     # a dense plane falls back to the sweep
    if W > 64:
        c.add("chunk")
    return c


def compare(label, o, e, rc, levels, tol, exact=True):
    """The moisture species bit-identical on the interior (exact) or within tol per patterned
    level; qv's patterned levels and every state field within tol."""
    ii = slice(1, rc.iy - 2)
    jj = slice(None) if rc.i_band else slice(1, rc.jx - 2)
    names = state_names(rc)
    got = {n: e.get(n) for n in names}
    ref = {n: o.get(n) for n in names}
    for nm, lev in levels.items():
        klist = sorted(k for v in lev.values() for k in (v if isinstance(v, list) else [v]))
        for lvl in ("ATM1", "ATM2"):
            a, b = got[f"{lvl}_{nm}"][:, ii, jj], ref[f"{lvl}_{nm}"][:, ii, jj]
            if exact and nm != "QV":
                ndiff = int((a != b).sum())
                print(f"{label}: {lvl}_{nm} differing interior points {ndiff}")
                assert ndiff == 0, (label, f"{lvl}_{nm}", ndiff)
            else:
                for k in klist:
                    den = float(np.max(np.abs(b[k])))
                    err = float(np.max(np.abs(a[k] - b[k]))) / max(den, 1e-300)
                    assert err < tol, (label, f"{lvl}_{nm}", k, err)
    for n in names:
        err = relerr(got[n], ref[n], rc, n)
        assert err < tol, (label, n, err)


def check_visible(label, o, marks, atm1):
    """With a positive atm1 every dependent negative of qc and the species must show its fixed
    value in the oracle's filtered state; the signed form's count is printed for the record."""
    for nm, tiles in marks.items():
        if nm == "QV":                 # filter_raw_qv floors at minqq p*, and qv keeps its own atm1
            continue
        new1, new2 = o.get(f"ATM1_{nm}"), o.get(f"ATM2_{nm}")
        vis, dep = sum(m.visible(new1, new2) for m in tiles), sum(int(m.dep.sum()) for m in tiles)
        print(f"{label}: {nm} fixed values visible in the filtered state at {vis} of {dep} dependent points")
        if atm1 == "positive":
            assert vis == dep, (label, nm, vis, dep)


# both input forms for every case: the signed one as the patterns were first written down, the
# positive one that lets the state show what the fix computed (patterned_state)
both_forms = pytest.mark.parametrize("atm1", ["signed", "positive"])


def run_case(monkeypatch, atm1, core, grid, nqx, env=None, qv=False, band=False, steps=0, force_sweep=False,
             dense_species=("QV", "QC", "QI", "QR", "QS"), claims=None, supplement=False):
    """One engine-against-oracle case: a tend (steps = 0), or step(1) and step(steps - 1) more."""
    rc, data = grid_case(core, grid, nqx, band)
    st, levels = patterned_state(rc, data, qv=qv, supplement=supplement, atm1=atm1)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    o, e = pair(rc, data, st)
    label = f"{core} {grid} nqx={nqx} {env or ''}{' band' if band else ''}{' qv' if qv else ''}" + \
        (" supplement" if supplement else "") + f" atm1 {atm1}"
    sp = species_of(rc, qv)
    claims = (claims_of(grid, force_sweep) if claims is None else claims) | ({"qv"} if qv else set())
    tol1 = 1e-11 if core == "nh" else 1e-12

    def forward(n):
        a2 = {nm: o.get(f"ATM2_{nm}") for nm in sp}
        if steps:
            o.step(n)
            e.step(n)
        else:
            o.tend()
            e.tend()
        return {nm: [Marks(cq, rc)] for nm, cq in forecasts(o, a2, sp).items()}

    marks = forward(1)
    check_claims(label, marks, levels, claims, force_sweep, dense_species)
    check_visible(label, o, marks, atm1)
    compare(label, o, e, rc, levels, tol1)
    for n in range(2, steps + 1):
        marks = forward(1)
        ndep = sum(int(m.dep.sum()) for t in marks.values() for m in t)
        print(f"{label}: step {n} dependent negatives {ndep}")
        assert ndep > 0, (label, n)
    if steps > 1:
        compare(label, o, e, rc, levels, 1e-11, exact=False)


# hydrostatic nqx = 2: every form resolves its planes by the row sweep (the trailing z slices of
# the split corrections; with RCMDYN_NO_QFUSE the extra blocks of k_split_project, without LDS
# when 2 W + 832 doubles exceed the projection's 4 kz SPC: G7)
HYD2 = [("G2", {}), ("G4", {}), ("G6", {}), ("G4", {"RCMDYN_NO_FUSE_BDY": "1"}), ("G4", {"RCMDYN_NO_QFUSE": "1"}),
        ("G7", {"RCMDYN_NO_QFUSE": "1"})]


def _cid(c):
    return "-".join([c[0]] + [k.replace("RCMDYN_", "") + ("" if v == "1" else v) for k, v in c[1].items()]) \
        if isinstance(c, tuple) else str(c)


@both_forms
@pytest.mark.parametrize("case", HYD2, ids=_cid)
def test_negfix_hydrostatic_qc(monkeypatch, case, atm1):
    grid, env = case
    run_case(monkeypatch, atm1, "hyd", grid, 2, env=env, force_sweep=True)


# hydrostatic ipptls = 2: k_negfix_serial_qx resolves qv, qc and the species (a block per plane,
# the wavefront on dense planes); with RCMDYN_NO_QFUSE the species go through k_qx_serial and
# qv / qc through k_split_project's sweeps
HYD5 = [(g, {}) for g in ("G1", "G2", "G3", "G4", "G5", "G6")] + \
       [(g, {"RCMDYN_NO_QFUSE": "1"}) for g in ("G2", "G4", "G5")] + \
       [(g, {"RCMDYN_NEGFIX_MODE": "1"}) for g in ("G4", "G5")]


@both_forms
@pytest.mark.parametrize("case", HYD5, ids=_cid)
def test_negfix_hydrostatic_species(monkeypatch, case, atm1):
    grid, env = case
    dense = ("QI", "QR", "QS") if "RCMDYN_NO_QFUSE" in env else ("QV", "QC", "QI", "QR", "QS")
    run_case(monkeypatch, atm1, "hyd", grid, 5, env=env, force_sweep="RCMDYN_NEGFIX_MODE" in env,
             dense_species=dense)


@both_forms
def test_negfix_hydrostatic_qv_patterned(monkeypatch, atm1):
    """The whole-plane and checkerboard levels also in qv (G4): its planes go through the same
    launch; qv's forecast is not bit-exact, so its patterned levels are held to 1e-12 each."""
    run_case(monkeypatch, atm1, "hyd", "G4", 5, qv=True)


NH_CASES = [("G2", 2, {}), ("G4", 2, {}), ("G6", 2, {}), ("G2", 5, {}), ("G5", 5, {}),
            ("G4", 2, {"RCMDYN_NEGFIX_MODE": "1"})]


@both_forms
@pytest.mark.parametrize("case", NH_CASES, ids=lambda c: f"{c[0]}-nqx{c[1]}" + "".join(f"-{k[7:]}" for k in c[2]))
def test_negfix_nh(monkeypatch, case, atm1):
    """k_nh_negfix_serial (qv / qc, the filters applied in place from the register queue) and,
    with ipptls = 2, k_qx_serial for the species."""
    grid, nqx, env = case
    run_case(monkeypatch, atm1, "nh", grid, nqx, env=env, force_sweep="RCMDYN_NEGFIX_MODE" in env)


# the second pattern set (supplement_field) on G4 through every kernel that resolves planes: the
# sweeps of k_split_correct and k_split_project, k_negfix_serial_qx and k_nh_negfix_serial by the
# wavefront and, with RCMDYN_NEGFIX_MODE=1, by the sweep
SUPPLEMENT = [("hyd", 2, {}), ("hyd", 2, {"RCMDYN_NO_QFUSE": "1"}), ("hyd", 5, {}),
              ("hyd", 5, {"RCMDYN_NEGFIX_MODE": "1"}), ("nh", 2, {}), ("nh", 2, {"RCMDYN_NEGFIX_MODE": "1"})]


@both_forms
@pytest.mark.parametrize("case", SUPPLEMENT, ids=lambda c: f"{c[0]}-nqx{c[1]}" + "".join(f"-{k[7:]}" for k in c[2]))
def test_negfix_supplement(monkeypatch, case, atm1):
    """A sweep that comes to a marked row over an unmarked one, and forecasts at the bottom of the
    normal range: on the sweep planes the first is asserted, on the wavefront planes the second."""
    core, nqx, env = case
    force_sweep = (core == "hyd" and nqx == 2) or "RCMDYN_NEGFIX_MODE" in env
    run_case(monkeypatch, atm1, core, "G4", nqx, env=env, force_sweep=force_sweep, supplement=True,
             claims={"tiny", "chunk", "skip"} if force_sweep else {"tiny", "dense", "ring", "ringwrap", "deep"})


@both_forms
@pytest.mark.parametrize("nthreads", [2, 4])
def test_negfix_decomposed(nthreads, atm1):
    """G3, ipptls = 2, against the oracle run as the same set_nproc tiles: the fix depends on the
    tiles by design (a tile's first interior column reads its neighbour's unfixed forecast).  The
    forecast itself does not, so the marks are restated per tile on the one-tile oracle's."""
    from regcm_amd.config import set_nproc
    rc, data = grid_case("hyd", "G3", 5)
    st, levels = patterned_state(rc, data, atm1=atm1)
    nproc = tuple(set_nproc(nthreads, rc.jx, rc.iy))
    sp = species_of(rc)
    one = oracle(rc, data, st)
    a2 = {nm: one.get(f"ATM2_{nm}") for nm in sp}
    one.tend()
    marks = {nm: [Marks(cq, rc, nproc, t) for t in range(nproc[0] * nproc[1])]
             for nm, cq in forecasts(one, a2, sp).items()}
    label = f"hyd G3 nqx=5 tiles {nproc} atm1 {atm1}"
    tallest = max(m.R for m in marks["QC"])
    check_claims(label, marks, {}, {"dense", "tiny"} | ({"ring"} if tallest > 64 else set()), False, sp)
    o, e = pair(rc, data, st, nproc, tiles=nthreads)
    o.step(1)
    e.step(1)
    check_visible(label, o, marks, atm1)
    compare(label, o, e, rc, levels, 1e-12)


@both_forms
def test_negfix_band(monkeypatch, atm1):
    """Periodic in j (i_band = 1) on the 24 x 68 grid: every column is interior, the first one
    has no sweep-predecessor to its west."""
    run_case(monkeypatch, atm1, "hyd", "G2", 5, band=True)


@both_forms
@pytest.mark.parametrize("grid", ["G2", "G4"])
def test_negfix_three_steps(monkeypatch, grid, atm1):
    """step(3) with ipptls = 2: the row flags and bitmap words are cleared for the next step and
    the steps are graph replays; the oracle shows dependent negatives in steps 2 and 3 as well.
    Bit-identical after step 1, the patterned levels below 1e-11 after step 3."""
    run_case(monkeypatch, atm1, "hyd", grid, 5, steps=3)
