"""The eigenvalue solver (csrc/eigen_device.hpp) on both sides of its magnitude guards.

The solver has short forms for ordinary magnitudes and sends every other lane to the
out-of-line generic solver:
  * eig3_sym_fast<0|1>: `unsafe` = p outside [2^-60, 2^60]; div_by_const has its own `odd`
    test at 2^+-100;
  * eig3_sym_fast2 (mode 2, the library default): `ok` = |tr| in [2^-100, 2^100] or zero and
    p2 in [2^-100, 2^100]; outside it the generic solver runs in mode 0;
  * all three enter the `diag` and `unsafe` repairs per wave on a ballot and select per lane.
Every other GPU test stays 40 binary orders inside these thresholds.  The tests here walk
matrices across each threshold, mix the kinds inside one wave and reach every kernel that
instantiates the solver, at magnitudes where the CPU oracle is finite, exact and covariant
under scaling by powers of two (tests/test_oracle_eigen.py pins that range).

Bars: the project's own relative ones, REL_TOL = 1e-6 |lambda_1| for modes 0 and 1 against
the oracle in the same mode and ASSERTED = 2e-6 for mode 2 against oracle mode 0, through
oracle.parity.assert_eig_parity on the triple.  eig_parity floors |lambda_1| at 1e-30; every
test asserts that its smallest non-zero reference |lambda_1| is above 1e-28, so the floor
never acts.  Where the reference triple is not finite the device triple must have the same
class (NaN, +inf, -inf, finite) per component: the fallback performs the reference's
operations.  The derived scalars are checked as bit-exact functions of the device's OWN
triple (float32 numpy, contraction off as in eig_features), never against the oracle, whose
two contexts disagree at the overflow edge of the product.  Inside a guard the device is also
compared with itself: ev(A * 2^k) == ldexp(ev(A), k) bit for bit, the test of the correctly
rounded short forms next to the ends of their range.  In mode 2 the lanes that the guard sends
to the generic solver are in addition held to mode 0's bar of bit-identical triples against
oracle mode 0: the short forms stay accurate to 2e-6 well beyond their guards, so only this
tells whether the fallback ran (and with which template argument).

Which tests stand on both sides of which guard (each asserts it, from float32 numpy):
  mode 2  p2 <= 2^100    batch k = 48..51 (mixed), <= 47 / >= 59; run p2_high; fd bands 46..59;
                         ramp k0 = -8; differential 2^52; mixed waves
  mode 2  p2 >= 2^-100   batch k = -52..-48; run p2_low; fd bands -62..0; ramp k0 = -70 and the
                         sampled columns; differential 2^-48; mixed waves
  mode 2  |tr|           trace_low_side (2^-123, 0 and 2^-100), trace_high_side (isotropic 2^98, 2^99, 2^100)
  mode 0/1  p <= 2^60    batch k = 59..61; run p_high; fd bands 57..59; ramp k0 = -8; differential 2^64
  mode 0/1  p >= 2^-60   batch k = -62..-59; run p_low; fd band -62; differential 2^-56; mixed waves
  div_by_const `odd`     trace_low_side (|tr| = 2^-123), trace_high_side (|tr| = 3 * 2^100), batch |k| >= 52
  ballots / selects      mixed waves (whole waves, lone lanes 0, 31, 63, 17, round-robin, partial wave)

Measured on an MI355X (maxima over all tests of this file): error against the oracle 0 in
mode 0, 3.6e-7 in mode 1, 3.2e-7 in mode 2; bit-identical fraction 1.0 in mode 0 everywhere
(0.74 / 0.37 at worst in modes 1 / 2, which are not expected to be); device covariance asserted
on 49152 rows of the batch test in modes 0 and 1 (12 magnitudes) and 20480 in mode 2 (5).  No
defect was found.

That the tests bite, from four scratch changes to eigen_device.hpp (wrong values, no faults):
  unsafe select of eig3_sym_fast2 removed      18 fail: every [trig2] case with fallback lanes
  unsafe select of eig3_sym_fast<> removed      6 fail: batch, trace_high_side, mixed_waves [trig0, trig1]
  g1 / g2 of fast2's diagonal select exchanged   1 fails: mixed_waves[trig2]
  ballots replaced by the first lane's flag     13 fail: mixed_waves and trace_high_side in every mode,
                                                batch, p2_high runs, fd, ramp -8, differential [trig2]
In modes 0 and 1 the short form is bit-identical to the generic solver as far as 2^61 and 2^-62,
so there only rows whose reference overflows (k >= 62, the lone lane 63 of the mixed waves) or
whose trace is extreme can tell the two apart."""
import os
import sys

import numpy as np
import pytest

from oracle.parity import assert_eig_parity

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jet_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
REL_TOL = 1e-6    # modes 0 and 1 against the oracle in the same mode (tests/test_gpu_parity.py)
ASSERTED = 2e-6   # mode 2 against oracle mode 0 (tests/test_gpu_trig_default.py)
TOL = {0: REL_TOL, 1: REL_TOL, 2: ASSERTED}
REF_MODE = {0: 0, 1: 1, 2: 0}
LAMBDA_FLOOR = 1e-28
EXACT_FRACTION = 0.999   # mode 0, the bar of test_eigen_batch_matches_oracle


def two(k):
    return np.ldexp(F(1), k)


@pytest.fixture(params=[0, 1, 2], ids=["trig0", "trig1", "trig2"])
def solver(request, ctx, ife):
    """(context, mode) with the context in that trig mode; mode 0 again afterwards."""
    mode = request.param
    if mode == 2:
        yield request.getfixturevalue("ctx_fast"), mode
        return
    ctx.set_option(ife.OPT_TRIG_MODE, mode)
    try:
        yield ctx, mode
    finally:
        ctx.set_option(ife.OPT_TRIG_MODE, 0)


# ---- the guards, recomputed in float32 numpy in the kernel's order -----------------------
def guard_quantities(A):
    """p0, tr, p2, p of eig3_sym_fast / eig3_sym_fast2: every operation rounds to float32 on
    its own, left to right, as the device code does with contraction off."""
    A = np.asarray(A, F)
    a11, a12, a13, a22, a23, a33 = [A[..., i] for i in range(6)]
    with np.errstate(all="ignore"):
        p0 = (a12 * a12 + a13 * a13) + a23 * a23
        tr = (a11 + a22) + a33
        q = tr / F(3)
        d1, d2, d3 = a11 - q, a22 - q, a33 - q
        p2 = ((d1 * d1 + d2 * d2) + d3 * d3) + F(2) * p0
        p = np.sqrt(p2 / F(6))
    return p0, tr, p2, p


def lane_flags(A, mode):
    """(diag, unsafe) per row as the solver of `mode` forms them."""
    p0, tr, p2, p = guard_quantities(A)
    diag = p0 == 0
    with np.errstate(all="ignore"):
        if mode == 2:
            atr = np.abs(tr)
            ok = (atr <= two(100)) & ((atr >= two(-100)) | (atr == 0)) & (p2 >= two(-100)) & (p2 <= two(100))
        else:
            ap = np.abs(p)
            ok = (ap >= two(-60)) & (ap <= two(60))
    return diag, ~diag & ~ok


def strictly_inside(A, mode):
    """Every row strictly inside the range of the short forms of `mode`."""
    p0, tr, p2, p = guard_quantities(A)
    with np.errstate(all="ignore"):
        if mode == 2:
            atr = np.abs(tr)
            return bool(((p2 > two(-100)) & (p2 < two(100)) & (atr > two(-100)) & (atr < two(100))).all())
        return bool(((p >= two(-60)) & (p <= two(60))).all())


# ---- assertions ----------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got, want, what):
    """uint32 views equal, NaN positions equal (a NaN's payload is not compared)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (bits(got) != bits(want)))
    if bad.any():
        rows = np.argwhere(bad)[:8]
        raise AssertionError("%s: %d of %d values differ in bits; first at %s: got %s want %s" % (
            what, int(bad.sum()), bad.size, rows.tolist(), got[bad][:8].tolist(), want[bad][:8].tolist()))


def value_class(x):
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def assert_derived_identity(f6, what):
    """sum, product and Frobenius norm as eig_features forms them from its own triple."""
    f6 = np.ascontiguousarray(f6, F).reshape(-1, 6)
    e0, e1, e2 = f6[:, 0], f6[:, 1], f6[:, 2]
    with np.errstate(all="ignore"):
        want = ((e0 + e1) + e2, (e0 * e1) * e2, np.sqrt((e0 * e0 + e1 * e1) + e2 * e2))
    for k, name in enumerate(("sum", "product", "frobenius")):
        assert_same_bits(f6[:, 3 + k], want[k], "%s: %s of the device triple" % (what, name))


def check_against_oracle(got, ref, mode, what, selections=None):
    """got, ref: (n, >=3) with the triple first.  Finite reference rows: the mode's parity bar;
    the other rows: the same class per component.  Rows flagged in `selections` (diagonal
    matrices, of any magnitude) must have the reference's bits instead.  Returns (parity dict,
    rows not finite)."""
    got = np.ascontiguousarray(got, F).reshape(-1, got.shape[-1])[:, :3]
    ref = np.ascontiguousarray(ref, F).reshape(-1, ref.shape[-1])[:, :3]
    if selections is not None:
        assert_same_bits(got[selections], ref[selections], what + ": diagonal rows are selections")
        got, ref = got[~selections], ref[~selections]
    fin = np.isfinite(ref).all(-1)
    lam = np.abs(ref[fin, 0])
    lam = lam[lam > 0]
    assert lam.size == 0 or lam.min() > LAMBDA_FLOOR, "%s: |lambda_1| %.3g reaches the checker's floor" % (
        what, lam.min())
    p = assert_eig_parity(got[fin], ref[fin], TOL[mode], what)
    gc, rc = value_class(got[~fin]), value_class(ref[~fin])
    assert (gc == rc).all(), "%s: %d of %d non-finite reference triples have another class on the device: %s vs %s" % (
        what, int((gc != rc).any(-1).sum()), int((~fin).sum()), got[~fin][(gc != rc).any(-1)][:4].tolist(),
        ref[~fin][(gc != rc).any(-1)][:4].tolist())
    return p, int((~fin).sum())


def exact_fraction(got, ref):
    got, ref = got.reshape(-1, got.shape[-1])[:, :3], ref.reshape(-1, ref.shape[-1])[:, :3]
    return float((bits(got) == bits(ref)).all(-1).mean())


def assert_fallback_is_the_double_solver(got, ref, unsafe, what):
    """Mode 2 sends its `unsafe` lanes to the generic solver in mode 0, which performs the
    reference's operations with double acos/cos: there the triple is held to mode 0's bar of
    bit-identical triples against oracle mode 0 (`ref`), not only to mode 2's 2e-6.  This is what
    tells the fallback from the short form where the short form is still accurate."""
    got, ref = got.reshape(-1, got.shape[-1])[:, :3], ref.reshape(-1, ref.shape[-1])[:, :3]
    sel = unsafe.reshape(-1) & np.isfinite(ref).all(-1)
    if sel.any():
        f = exact_fraction(got[sel], ref[sel])
        assert f > EXACT_FRACTION, "%s: only %.5f of the %d fallback triples have the double solver's bits" % (
            what, f, int(sel.sum()))
    return int(sel.sum())


_batch_refs = {}


def batch_ref(oracle, key, A, ref_mode):
    """oracle.eig3 of a named batch, computed once per (name, context) and shared."""
    if (key, ref_mode) not in _batch_refs:
        ref = oracle.eig3(A, ref_mode)
        ref.setflags(write=False)
        _batch_refs[key, ref_mode] = ref
    return _batch_refs[key, ref_mode]


def run_batch(ctx, oracle, mode, key, A, what, exact=False):
    """Both batch entry points on A against the oracle; returns (triple, parity dict)."""
    ref = batch_ref(oracle, key, A, REF_MODE[mode])
    ev = ctx.eigenvalues(A)
    ft = ctx.eigenvalue_features(A)
    diag = lane_flags(A, mode)[0]
    p, nonfinite = check_against_oracle(ev, ref, mode, what + " eigenvalues", diag)
    check_against_oracle(ft, ref, mode, what + " features", diag)
    assert_derived_identity(ft, what)
    if mode == 2:
        unsafe = lane_flags(A, 2)[1]
        assert_fallback_is_the_double_solver(ev, ref, unsafe, what + " eigenvalues")
        assert_fallback_is_the_double_solver(ft, ref, unsafe, what + " features")
    p["nonfinite_ref"] = nonfinite
    p["exact"] = exact_fraction(ev, ref)
    if exact and mode == 0:
        assert p["exact"] > EXACT_FRACTION, "%s: only %.5f of the triples bit-identical" % (what, p["exact"])
        assert exact_fraction(ft, ref) > EXACT_FRACTION, what
    return ev, p


# ---- 2. batch entry points across magnitudes ---------------------------------------------------
ROWS_SEED, ROWS = 3, 4096
KS = (-70, -66, -64, -63, -62, -61, -60, -59, -52, -51, -50, -49, -48, -40, 0, 40, 47, 48, 49, 50, 51,
      59, 60, 61, 62, 63, 64, 66, 100, 126)
_rows = {}


def base_rows():
    if "A" not in _rows:
        A = np.random.default_rng(ROWS_SEED).standard_normal((ROWS, 6)).astype(F)
        A.setflags(write=False)
        _rows["A"] = A
    return _rows["A"]


def scaled(A, k):
    with np.errstate(over="ignore"):
        return np.ldexp(np.asarray(A, F), k).astype(F)


def test_batch_entry_points_across_magnitudes(solver, oracle):
    ctx, mode = solver
    A0 = base_rows()
    ev0 = ctx.eigenvalues(A0)
    worst, least_exact, covariant_rows, covariant_ks, unsafe_share = 0.0, 1.0, 0, [], {}
    for k in KS:
        A = scaled(A0, k)
        what = "mode %d k %d" % (mode, k)
        ev, p = run_batch(ctx, oracle, mode, ("rows", k), A, what, exact=-51 <= k <= 61)
        worst = max(worst, p["max_err"])
        if -51 <= k <= 61:
            least_exact = min(least_exact, p["exact"])
        unsafe_share[k] = float(lane_flags(A, mode)[1].mean())
        if strictly_inside(A, mode) and (mode == 2 or k >= -51):
            assert_same_bits(ev, scaled(ev0, k), what + ": device triple of A * 2^k against ldexp of its triple of A")
            covariant_rows += A.shape[0]
            covariant_ks.append(k)
    # both sides of the mode's guards, and waves that hold both kinds
    lo = [k for k in KS if k < 0]
    hi = [k for k in KS if k > 0]
    for side in (lo, hi):
        assert any(unsafe_share[k] == 1.0 for k in side) and any(unsafe_share[k] == 0.0 for k in side)
        assert any(0.0 < unsafe_share[k] < 1.0 for k in side)
    assert {-40, 0, 40} <= set(covariant_ks)
    if mode != 2:
        assert {-51, -50, 50, 51} <= set(covariant_ks)
    print("mode %d: max error %.3g |lambda1| over %d magnitudes; least bit-identical fraction for k in [-51, 61] "
          "%.6f; device covariance asserted on %d rows (k = %s)" % (mode, worst, len(KS), least_exact,
                                                                     covariant_rows, covariant_ks))


# ---- 3. threshold runs ---------------------------------------------------------------------------
RUN = 129  # consecutive floats, 64 on either side of the centre


def float_run(centre):
    c = F(centre)
    down, up = [c], [c]
    for _ in range(RUN // 2):
        down.append(np.nextafter(down[-1], F(0)))
        up.append(np.nextafter(up[-1], F(np.inf)))
    return np.array(down[:0:-1] + up, F)


def structured(a):
    """[0, a, a, 0, 0, 0]: tr = 0, p2 = 4 a^2, p = a sqrt(2/3), r = 0."""
    A = np.zeros((a.size, 6), F)
    A[:, 1] = a
    A[:, 2] = a
    return A


def perturbed(a):
    """A fixed random O(1) row, normalised in double to p2 = 4 like the structured one, times a."""
    row = np.random.default_rng(17).standard_normal(6)
    q = (row[0] + row[3] + row[5]) / 3
    p2 = (row[0] - q) ** 2 + (row[3] - q) ** 2 + (row[5] - q) ** 2 + 2 * (row[1] ** 2 + row[2] ** 2 + row[4] ** 2)
    row = (row * 2.0 / np.sqrt(p2)).astype(F)
    with np.errstate(over="ignore"):
        return (row[None, :] * a[:, None]).astype(F)


# name -> (centre of the parameter, power of two that brings the run to O(1), modes whose guard it walks)
P_RUNS = {
    "p2_high": (2.0 ** 49, 49, (2,)),
    "p2_low": (2.0 ** -51, -51, (2,)),
    "p_high": (2.0 ** 60 * np.sqrt(1.5), 60, (0, 1)),
    "p_low": (2.0 ** -60 * np.sqrt(1.5), -60, (0, 1)),
}


@pytest.mark.parametrize("shape", ["structured", "perturbed"])
@pytest.mark.parametrize("name", list(P_RUNS))
def test_threshold_runs_of_p(solver, oracle, name, shape):
    ctx, mode = solver
    centre, k, guard_modes = P_RUNS[name]
    A = (structured if shape == "structured" else perturbed)(float_run(centre))
    assert A.shape == (RUN, 6)
    p0, tr, p2, p = guard_quantities(A)
    # the guarded quantity stands on both sides of its threshold
    t = two(2 * k + 2) if 2 in guard_modes else two(k)
    g = p2 if 2 in guard_modes else p
    assert (g < t).sum() >= 32 and (g >= t).sum() >= 32 and (g > t).any(), (name, shape)
    for m in guard_modes:
        unsafe = lane_flags(A, m)[1]
        assert unsafe.any() and not unsafe.all(), (name, shape, m)
    what = "mode %d %s %s" % (mode, name, shape)
    ev, pr = run_batch(ctx, oracle, mode, (name, shape), A, what, exact=True)
    assert pr["nonfinite_ref"] == 0, what
    if mode != 2 and strictly_inside(A, mode) and k >= -51:
        assert_same_bits(ev, scaled(ctx.eigenvalues(scaled(A, -k)), k), what + ": covariance")
    print("%s: max error %.3g, bit-identical %.4f, %d unsafe lanes of %d" % (
        what, pr["max_err"], pr["exact"], int(lane_flags(A, mode)[1].sum()), RUN))


def trace_low_rows():
    """512 rows whose |tr| = 2^-123 is non-zero and below 2^-100 with p2 ordinary, interleaved with
    rows of zero trace and of trace above 2^-100 (both on the short form's side)."""
    n = 1024
    A = np.zeros((n, 6), F)
    off = (np.random.default_rng(23).standard_normal((n, 3)) * 2.0 ** -45).astype(F)
    A[:, 1], A[:, 2], A[:, 4] = off[:, 0], off[:, 1], off[:, 2]
    kind = np.arange(n) % 4
    A[:, 0] = two(-101)
    A[:, 3] = np.where(kind == 1, -two(-101), np.where(kind == 3, two(-101), -two(-101) + two(-123)))
    return A, kind


def trace_high_rows():
    """|tr| on both sides of 2^100.  Isotropic diagonals 2^100 and 2^99 (|tr| above 2^100, p2
    ordinary, reference finite: only the |tr| test sends them to the generic solver), 2^98 (below),
    O(1) rows times 2^101 (reference not finite: class equality) and O(1) rows."""
    n = 640
    A = np.random.default_rng(29).standard_normal((n, 6)).astype(F)
    kind = np.arange(n) % 5
    for kk, e in ((0, 100), (1, 99), (2, 98)):
        A[kind == kk, 0] = A[kind == kk, 3] = A[kind == kk, 5] = two(e)
    A[kind == 3] = scaled(A[kind == 3], 101)
    return A, kind


def test_threshold_of_the_trace_low_side(solver, oracle):
    ctx, mode = solver
    A, kind = trace_low_rows()
    p0, tr, p2, p = guard_quantities(A)
    atr = np.abs(tr)
    low = (atr != 0) & (atr < two(-100))
    assert low.sum() == 512 and (atr[low] == two(-123)).all()
    assert (atr == 0).sum() == 256 and (atr >= two(-100)).sum() == 256
    assert ((p2 >= two(-100)) & (p2 <= two(100))).all() and ((p >= two(-60)) & (p <= two(60))).all()
    np.testing.assert_array_equal(lane_flags(A, 2)[1], low)
    assert not lane_flags(A, 0)[1].any()
    what = "mode %d trace below 2^-100" % mode
    ev, pr = run_batch(ctx, oracle, mode, "trace_low", A, what, exact=True)
    assert pr["nonfinite_ref"] == 0
    print("%s: max error %.3g, bit-identical %.4f" % (what, pr["max_err"], pr["exact"]))


def test_threshold_of_the_trace_high_side(solver, oracle):
    ctx, mode = solver
    A, kind = trace_high_rows()
    p0, tr, p2, p = guard_quantities(A)
    with np.errstate(invalid="ignore"):
        above = ~(np.abs(tr) <= two(100))
    assert above[kind <= 1].all() and above[kind == 3].any() and not above[kind == 2].any() and not above[kind == 4].any()
    iso = kind <= 2
    assert ((p2[iso] >= two(-100)) & (p2[iso] <= two(100))).all()      # only the trace decides there
    assert np.isinf(p2[kind == 3]).all()
    np.testing.assert_array_equal(lane_flags(A, 2)[1], above | (kind == 3))
    what = "mode %d trace above 2^100" % mode
    ref = batch_ref(oracle, "trace_high", A, REF_MODE[mode])
    fin = np.isfinite(ref).all(-1)
    assert fin[kind != 3].all() and not fin[kind == 3].any()
    ev, pr = run_batch(ctx, oracle, mode, "trace_high", A, what)
    assert pr["nonfinite_ref"] == int((kind == 3).sum())
    if mode == 0:
        assert exact_fraction(ev[fin], ref[fin]) > EXACT_FRACTION
    print("%s: max error %.3g, bit-identical %.4f, %d rows compared by class" % (
        what, pr["max_err"], pr["exact"], pr["nonfinite_ref"]))


# ---- 4. mixed waves --------------------------------------------------------------------------------
ORDINARY, HIGH, LOW, DIAGONAL, NOT_A_NUMBER, OVERFLOWING = range(6)
WAVE = 64


def mixed_waves():
    """(A, kind): consecutive 64-row groups (the waves of the batch kernel) of each composition."""
    A0 = base_rows()
    p = guard_quantities(A0)[3]
    pool = A0[(p >= 0.6) & (p <= 2.0)]      # times 2^61 above 2^60, times 2^-62 below 2^-60, in every mode
    rng = np.random.default_rng(31)
    taken = [0]

    def row(kind):
        if kind == DIAGONAL:
            d = rng.standard_normal(6).astype(F)
            d[[1, 2, 4]] = 0
            return scaled(d, int(rng.choice([0, 0, 120, -120])))
        r = pool[taken[0]].copy()
        taken[0] += 1
        if kind == HIGH:
            return scaled(r, 61)
        if kind == LOW:
            return scaled(r, -62)
        if kind == OVERFLOWING:
            return scaled(r, 66)         # p2 overflows in every row: the reference is inf / NaN
        if kind == NOT_A_NUMBER:
            r[int(rng.choice([0, 1]))] = np.nan
        return r

    groups = [[ORDINARY] * WAVE, [HIGH] * WAVE, [LOW] * WAVE, [DIAGONAL] * WAVE]
    for lane, k in ((0, HIGH), (31, LOW), (63, OVERFLOWING), (17, DIAGONAL)):
        g = [ORDINARY] * WAVE
        g[lane] = k
        groups.append(g)
    groups.append([(ORDINARY, DIAGONAL, HIGH, LOW, NOT_A_NUMBER)[i % 5] for i in range(WAVE)])
    groups.append([ORDINARY] * 36 + [LOW])                                  # partial: n % 64 == 37
    kind = np.array([k for g in groups for k in g])
    A = np.stack([row(k) for k in kind]).astype(F)
    assert taken[0] <= pool.shape[0]
    return A, kind


def test_mixed_waves(solver, oracle):
    ctx, mode = solver
    A, kind = mixed_waves()
    n = A.shape[0]
    assert n % WAVE == 37
    diag, unsafe = lane_flags(A, mode)
    np.testing.assert_array_equal(diag, kind == DIAGONAL)
    np.testing.assert_array_equal(unsafe, np.isin(kind, (HIGH, LOW, NOT_A_NUMBER, OVERFLOWING)))
    w = lambda flags, g: np.flatnonzero(flags[g * WAVE:(g + 1) * WAVE]).tolist()
    assert [w(unsafe, g) for g in (4, 5, 6)] == [[0], [31], [63]] and w(diag, 7) == [17]
    assert w(unsafe, 9) == [36] and not any(w(diag, g) for g in (4, 5, 6, 9)) and not w(unsafe, 7)
    big = np.abs(A[kind == DIAGONAL]).max(-1)
    assert (big > two(119)).any() and (big < two(-117)).any()
    what = "mode %d mixed waves" % mode
    ev, pr = run_batch(ctx, oracle, mode, "mixed", A, what)
    ref = batch_ref(oracle, "mixed", A, REF_MODE[mode])
    fin = np.isfinite(ref).all(-1)
    np.testing.assert_array_equal(fin, ~np.isin(kind, (NOT_A_NUMBER, OVERFLOWING)))
    if mode == 0:
        assert exact_fraction(ev[fin], ref[fin]) > EXACT_FRACTION
    # the same rows with other neighbours: a fixed permutation
    perm = np.random.default_rng(37).permutation(n)
    evp, prp = run_batch(ctx, oracle, mode, "mixed_permuted", np.ascontiguousarray(A[perm]), what + " permuted")
    assert_same_bits(evp, ev[perm], what + ": a row's triple depends on its neighbours in the wave")
    print("%s: max error %.3g (permuted %.3g), bit-identical %.4f" % (what, pr["max_err"], prp["max_err"],
                                                                      exact_fraction(ev[fin], ref[fin])))


# ---- 5. the kernels that instantiate the solver ----------------------------------------------------
VOL_SHAPE = (12, 20, 136)     # x: two whole 64-voxel row segments and a partial one
SPACINGS = ((1.0, 1.0, 1.0), (0.7, 0.8, 1.25))   # the two stencil instantiations
# exponent of the 8-column band x // 8.  The top bands are 57, 58, 59: with 60 and 61 the float p2
# of the reference overflows inside the mask (p reaches 2^62.2 at unit spacing, more at the other)
BAND_E = (-62, -58, -52, -51, -50, -49, -46, 0, 46, 49, 50, 51, 52, 57, 58, 59)
_vol = {}


def banded_volume(synth, oracle):
    """synth.volume_f32 times a power of two that brings the oracle Hessian's median p to about 1,
    column band x // 8 times 2^E; the mask is zero on the first three rows."""
    if "img" not in _vol:
        vol = synth.volume_f32(VOL_SHAPE, synth.SEED_CONFIG[1])
        med = float(np.median(guard_quantities(oracle.hessian3d(vol))[3]))
        base = scaled(vol, -int(np.round(np.log2(med))))
        assert 0.5 < np.median(guard_quantities(oracle.hessian3d(base))[3]) < 2.0
        e = np.array(BAND_E)[(np.arange(VOL_SHAPE[2]) // 8) % len(BAND_E)]
        img = (base * np.ldexp(F(1), e)[None, None, :]).astype(F)
        mask = np.ones(VOL_SHAPE, np.uint8)
        mask[:, :3, :] = 0
        img.setflags(write=False)
        _vol["base"], _vol["img"], _vol["mask"] = base, img, mask
    return _vol["img"], _vol["mask"]


def segments_with_both_sides(flag, valid):
    """How many 64-voxel row segments hold valid voxels with the flag set and with it clear."""
    nz, ny, nx = flag.shape
    n = 0
    for x0 in range(0, nx, WAVE):
        f, v = flag[:, :, x0:x0 + WAVE], valid[:, :, x0:x0 + WAVE]
        n += int(((f & v).any(-1) & (~f & v).any(-1)).sum())
    return n


def assert_guards_straddled(H, valid, modes, what, sides=("low", "high")):
    """From a float32 Hessian field: each guard of each mode has a row segment with both sides."""
    p0, tr, p2, p = guard_quantities(H)
    for m in modes:
        g = p2 if m == 2 else p
        lo, hi = (two(-100), two(100)) if m == 2 else (two(-60), two(60))
        if "low" in sides:
            assert segments_with_both_sides(g < lo, valid) > 0, "%s: mode %d low guard" % (what, m)
        if "high" in sides:
            assert segments_with_both_sides(g > hi, valid) > 0, "%s: mode %d high guard" % (what, m)


_fd_refs = {}


def fd_ref(oracle, img, mask, spacing, ref_mode):
    if (spacing, ref_mode) not in _fd_refs:
        ref = oracle.fd_hessian_features(img, mask, spacing, ref_mode)
        ref.setflags(write=False)
        _fd_refs[spacing, ref_mode] = ref
    return _fd_refs[spacing, ref_mode]


@pytest.mark.parametrize("spacing", SPACINGS, ids=["unit", "aniso"])
def test_fd_hessian_features_across_the_guards(solver, ife, oracle, synth, spacing):
    ctx, mode = solver
    img, mask = banded_volume(synth, oracle)
    inside = mask != 0
    H = oracle.hessian3d(img, spacing)      # the device Hessian has these bits (test below)
    assert_guards_straddled(H, inside, (0, 1, 2), "fd %s" % (spacing,))
    unsafe2 = lane_flags(H, 2)[1]
    ref = fd_ref(oracle, img, mask, spacing, REF_MODE[mode])
    assert np.isfinite(ref[inside][:, :3]).all(), "the reference is not finite inside the mask"
    first = None
    for ring in (1, 0):
        ctx.set_option(ife.OPT_FEAT_RING, ring)
        try:
            for layout in (ife.INTERLEAVED, ife.PLANAR):
                got = ctx.fd_hessian_features(img, mask, spacing, layout=layout)
                if layout == ife.PLANAR:
                    got = np.ascontiguousarray(np.moveaxis(got, 0, -1))
                what = "mode %d fd hessian spacing %s ring %d layout %d" % (mode, spacing, ring, layout)
                pr, nonfinite = check_against_oracle(got[inside], ref[inside], mode, what)
                assert nonfinite == 0
                if mode == 2:
                    assert assert_fallback_is_the_double_solver(got[inside], ref[inside], unsafe2[inside], what) > 1000
                assert_derived_identity(got, what)
                assert (got[~inside] == 0).all(), what + ": not zero outside the mask"
                if first is None:
                    first = got
                    print("%s: max error %.3g, bit-identical %.5f" % (what, pr["max_err"],
                                                                      exact_fraction(got[inside], ref[inside])))
                    if mode == 0:
                        assert exact_fraction(got[inside], ref[inside]) > EXACT_FRACTION
                else:
                    assert_same_bits(got, first, what + ": differs from the first form")
        finally:
            ctx.set_option(ife.OPT_FEAT_RING, 1)


@pytest.mark.parametrize("k", [0, -80], ids=["banded", "denormal_differences"])
@pytest.mark.parametrize("spacing", SPACINGS, ids=["unit", "aniso"])
def test_hessian_and_gradient_bits_at_extreme_magnitudes(ctx, ife, oracle, synth, spacing, k):
    img, _ = banded_volume(synth, oracle)
    img = scaled(img, k)
    if k:
        tiny = np.abs(np.diff(img[..., :8], axis=-1))
        assert ((tiny > 0) & (tiny < np.finfo(F).tiny)).any()     # differences among the denormals
    h_ref = oracle.hessian3d(img, spacing)
    g_ref = oracle.gradient_magnitude(img, spacing)
    assert_same_bits(ctx.hessian3d(img, spacing), h_ref, "hessian3d")
    assert_same_bits(np.moveaxis(ctx.hessian3d(img, spacing, layout=ife.PLANAR), 0, -1), h_ref, "hessian3d planar")
    assert_same_bits(ctx.gradient_magnitude(img, spacing), g_ref, "gradient magnitude")


RAMP_K0 = (-70, -8)   # |lambda_1| from 2^-59.5 to 2^-0.4, and from 2^2.5 to 2^61.6, finite triples (CPU)
RAMP_SIGMAS = (1.0, 2.5)
_ramp = {}


def ramp_case(oracle, synth, k0):
    """(|volume| + 1) * 2^(k0 + x/2): smoothing would spread a large band over a small one, a
    ramp keeps neighbours within a factor.  (image, mask, {(sigma, context): reference})."""
    if k0 not in _ramp:
        vol = synth.volume_f32(VOL_SHAPE, synth.SEED_CONFIG[1])
        x = np.arange(VOL_SHAPE[2])
        img = ((np.abs(vol) + 1) * np.exp2(k0 + x / 2.0)[None, None, :]).astype(F)
        mask = np.minimum(synth.mask_ellipsoids(VOL_SHAPE), 1).astype(np.uint8)
        inside = mask != 0
        refs = {}
        for sigma in RAMP_SIGMAS:
            for rm in (0, 1):
                ref = oracle.emphysema_features(img, mask, sigma, (1.0, 1.0, 1.0), rm)
                assert np.isfinite(ref[inside][:, :5]).all(), "the reference is not finite inside the mask"
                ref.setflags(write=False)
                refs[sigma, rm] = ref
        # which guards the ramp crosses inside a row segment, from the Hessian of the unmasked field
        S = oracle.normalized_gaussian_convolution(img, mask.astype(F), 1.0)
        H = oracle.hessian3d(S)
        if k0 < -30:
            assert_guards_straddled(H, inside, (2,), "ramp k0 %d" % k0, sides=("low",))
        else:
            assert_guards_straddled(H, inside, (0, 1, 2), "ramp k0 %d" % k0, sides=("high",))
        lam = np.abs(refs[1.0, 0][inside][:, 2])
        assert (np.log2(lam.max()) > 55) if k0 > -30 else (np.log2(lam[lam > 0].min()) < -58)
        # mode 2's fallback lanes at sigma = 1, a voxel's margin away from the thresholds (the
        # Hessian here is the oracle's, of the unmasked smoothed field)
        p0, tr, p2, p = guard_quantities(H)
        far = lane_flags(H, 2)[1] & ((p2 < two(-102)) | (p2 > two(102)))
        _ramp[k0] = (img, mask, refs, far)
    return _ramp[k0]


def check_feature_volume(got, ref, mask, mode, what):
    inside = mask != 0
    assert_same_bits(got[..., 0], ref[..., 0], what + ": S")
    assert_same_bits(got[..., 1], ref[..., 1], what + ": G")
    pr, nonfinite = check_against_oracle(got[inside][:, 2:], ref[inside][:, 2:], mode, what)
    assert nonfinite == 0, what
    assert_derived_identity(got[..., 2:], what)
    assert (got[~inside] == 0).all(), what + ": not zero outside the mask"
    return pr


@pytest.mark.parametrize("k0", RAMP_K0)
def test_emphysema_features_across_the_guards(solver, ife, oracle, synth, k0):
    ctx, mode = solver
    img, mask, refs, far = ramp_case(oracle, synth, k0)
    inside = mask != 0
    got = ctx.emphysema_features(img, mask, list(RAMP_SIGMAS))
    for s, sigma in enumerate(RAMP_SIGMAS):
        what = "mode %d ramp k0 %d sigma %g" % (mode, k0, sigma)
        pr = check_feature_volume(got[s], refs[sigma, REF_MODE[mode]], mask, mode, what)
        if mode == 2 and sigma == 1.0:
            assert assert_fallback_is_the_double_solver(got[s][inside][:, 2:], refs[sigma, 0][inside][:, 2:],
                                                        far[inside], what) > 100
        print("%s: max error %.3g" % (what, pr["max_err"]))
    planar = ctx.emphysema_features(img, mask, list(RAMP_SIGMAS), layout=ife.PLANAR)
    assert_same_bits(np.moveaxis(planar, 1, -1), got, "planar layout")


def test_sampled_columns_across_the_guards(solver, oracle, synth):
    """The fused sampling instantiation: every voxel is foreground (labels 0 and 1), so the
    columns are the feature volumes in raster order."""
    ctx, mode = solver
    img, mask, refs, far = ramp_case(oracle, synth, RAMP_K0[0])
    s = ctx.samples(8 * len(RAMP_SIGMAS))
    try:
        s.add_image(img, mask, list(RAMP_SIGMAS), foreground=(0, 1))
        assert s.count(0) == img.size
        cols = np.stack([s.column(c) for c in range(8 * len(RAMP_SIGMAS))])
    finally:
        s.close()
    for i, sigma in enumerate(RAMP_SIGMAS):
        got = np.ascontiguousarray(cols[i * 8:(i + 1) * 8].T).reshape(VOL_SHAPE + (8,))
        what = "mode %d sampled columns sigma %g" % (mode, sigma)
        check_feature_volume(got, refs[sigma, REF_MODE[mode]], mask, mode, what)
        if mode == 2 and sigma == 1.0:
            inside = mask != 0
            assert assert_fallback_is_the_double_solver(got[inside][:, 2:], refs[sigma, 0][inside][:, 2:],
                                                        far[inside], what) > 100


DIFF_SHAPE, DIFF_SIGMA = (12, 16, 20), 1.0
# 2^52 and 2^-52 put p around the mode 2 guards (2^48.7 and 2^-51.3); 2^-48 has voxels on both
# sides of the lower one; 2^64 and 2^-56 do the same for p = 2^60 and 2^-60 of modes 0 and 1
DIFF_EXPONENTS = (52, -52, -48, 64, -56)
_diff = {}


def diff_case(oracle, synth, k):
    if k not in _diff:
        img = scaled(np.random.default_rng(41).standard_normal(DIFF_SHAPE).astype(F), k)
        mask = np.minimum(synth.mask_ellipsoids(DIFF_SHAPE), 1).astype(np.uint8)
        ref = jet_oracle.features(oracle, img, mask, DIFF_SIGMA)
        H = jet_oracle.jet(oracle, img, mask.astype(F), DIFF_SIGMA)[..., 4:]
        inside = mask != 0
        assert np.isfinite(ref[inside][:, :5]).all(), "the reference is not finite inside the mask"
        flags = {m: lane_flags(H, m)[1][inside] for m in (0, 2)}
        _diff[k] = (img, mask, ref, flags)
    return _diff[k]


@pytest.mark.parametrize("mode", [0, 2])
def test_differential_features_across_the_guards(ctx, ife, oracle, synth, mode):
    cases = {k: diff_case(oracle, synth, k) for k in DIFF_EXPONENTS}
    share = {k: float(c[3][mode].mean()) for k, c in cases.items()}
    if mode == 2:
        assert 0 < share[52] < 1 and share[-52] == 1 and 0 < share[-48] < 1
    else:
        assert share[52] == 0 and share[-52] == 0 and 0 < share[64] < 1 and 0 < share[-56] < 1
    ctx.set_option(ife.OPT_TRIG_MODE, mode)
    try:
        for k, (img, mask, ref, _) in cases.items():
            got = ctx.differential_features(img, mask, [DIFF_SIGMA])[0]
            what = "mode %d differential features times 2^%d" % (mode, k)
            pr = check_feature_volume(got, ref, mask, mode, what)
            if mode == 2:
                inside = mask != 0
                assert_fallback_is_the_double_solver(got[inside][:, 2:], ref[inside][:, 2:], cases[k][3][2], what)
            print("%s: max error %.3g, %.0f %% of the voxels outside the short form" % (what, pr["max_err"],
                                                                                      100 * share[k]))
    finally:
        ctx.set_option(ife.OPT_TRIG_MODE, 0)
