"""The fit kernels where eigenvalues of the KL covariance C fall at or below
the pinv cutoff (kPinvAtol = 1e-3, csrc/kl_fit_steps.h).

Every fit kernel inverts C through its eigen-decomposition and drops the
components with |lambda| <= 1e-3; at r_0 = 100 on well separated directions
-- every other input of the suite -- no eigenvalue comes near, and the
comparisons never come out false.  The inputs here (tests/cutoff_cases.py)
reach them through a large r_0 (rank 17, 4 and 0 of 20; D = 7 .. 128) and
through nearly coincident directions at r_0 = 100 (``twins20``, ``dup12``,
``tie_small``); tests/test_fit_cutoff_cpu.py shows on the oracle that no
eigenvalue is within 1e-4 of the cutoff and that no order, flag or
coefficient hangs on rounding, so no slot is excluded here.

``tie_small`` pins the rule for two unflagged directions (Tie2): a pair whose
|b| passes the cutoff is fitted as (0, atan2(t)); a pair below it gets what
the reference gives (tests/golden/near_tie4.npz), zero coefficients and the
values as residuals.

Tolerances: those of tests/test_fit_walk.py -- orders and ``w_out``
identical, |d coef| <= 1e-8 x max(1, |coef|max), |d resid| <= 1e-8; byte
equality among the options the ABI documents as "same bits".
Needs an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest

import cutoff_cases as cc
import walk_cases as wc
from test_fit_walk import check, fit, options, same_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RUNS = cc.all_runs()
NEAR_RUNS = cc.all_runs(list(cc.NEAR_FILES))
NARROW = [r for r in RUNS if r.val.shape[-1] <= 60]
WIDE = [r for r in RUNS if r.val.shape[-1] > 60]
NARROW_PHASE = [r for r in NARROW if r.type == "phase"]
LANE_MAX_D = 23  # kLaneMaxD, csrc/kl_fit_lane.h
LANE = [r for r in NARROW_PHASE if 3 <= r.val.shape[-1] <= LANE_MAX_D]
TEC = [r for r in NARROW if r.type == "tec"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx(dev):
    from ska_sdp_screen_fitting_amd import get_context
    c = get_context(0)
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    return c


# ------------------------------------------------- 1. the default pipeline

@pytest.mark.parametrize("r", RUNS, ids=wc.run_id)
def test_fit_vs_oracle(ctx, dev, r):
    """Every case on the default pipeline (the wide fit above 60
    directions) against the oracle."""
    got = fit(ctx, dev, r)
    check(got, wc.oracle(r), wc.run_id(r))
    st = ctx.fit_stats()
    tiny = ((r.weight > 0) & (r.weight <= 1e-3)).any()
    if r.val.shape[-1] <= 60:
        # weights of 5e-4: the slow class (truncated_eig_solve) ran
        assert (st["n_general"] > 0) == bool(tiny)
    assert tiny == (r.case in ("mixed20_r0_1e4", "tie_small"))


@pytest.mark.parametrize("r", NEAR_RUNS, ids=wc.run_id)
def test_fit_vs_reference(ctx, dev, r):
    """twins20 and tie_small against the reference's own run."""
    check(fit(ctx, dev, r), cc.reference(r), wc.run_id(r) + " reference")


@pytest.mark.parametrize("r", LANE, ids=wc.run_id)
def test_lane_kernel_ran_and_keeps_every_bit(ctx, dev, r):
    """D <= 23, phase: the lane-per-slot kernel took the unflagged slots (its
    own ``keep`` tests ran), and the pass kernel alone writes the same
    bytes."""
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_FIT_LANE
    on = fit(ctx, dev, r)
    lane = ctx.fit_lane_stats()
    w = r.weight
    eligible = (wc.fitted(r) & (w > 0).all(axis=-1)
                & (w.max(axis=-1) == w.min(axis=-1)))
    print(wc.run_id(r), "lane", lane, "eligible", int(eligible.sum()))
    assert lane["n_lane"] == int(eligible.sum())
    if r.case != "tie_small":      # (its only unflagged slots: one in six)
        assert lane["n_lane"] > 20
    assert lane["n_lane"] > 0
    ctx.set_option(SF_OPT_FIT_LANE, 0)
    try:
        off = fit(ctx, dev, r)
        assert ctx.fit_lane_stats() == {"n_lane": 0, "n_deferred": 0}
    finally:
        ctx.set_option(SF_OPT_FIT_LANE, 1)
    same_bytes(on, off, (wc.run_id(r), "lane on / off"))
    check(off, wc.oracle(r), wc.run_id(r) + " lane off")


# ------------------------------------- 2. the options that keep every bit

SAME_BITS = [dict(PACK=0), dict(LEAN=0), dict(EIG_WAVES=1), dict(EIG_WAVES=4),
             dict(SUBSET_DELETION=2), dict(SUBSET_DELETION=3)]


@pytest.mark.parametrize("r", NARROW, ids=wc.run_id)
def test_fit_options_keep_every_bit(ctx, dev, r):
    """One slot per wavefront, the general layout, 1 and 4 waves per subset
    Jacobi and the deletion modes 2 and 3 (twins20 and dup12: subset spectra
    with a tiny eigenvalue that may or may not separate) write the bytes the
    defaults write."""
    base = fit(ctx, dev, r)
    check(base, wc.oracle(r), wc.run_id(r))
    for o in SAME_BITS:
        with options(ctx, **o):
            same_bytes(fit(ctx, dev, r), base, (wc.run_id(r), o))


@pytest.mark.parametrize("r", WIDE, ids=wc.run_id)
def test_wide_fit_options_keep_every_bit(ctx, dev, r):
    """Above 60 directions: the mask cache off and a pool of one entry."""
    base = fit(ctx, dev, r)
    check(base, wc.oracle(r), wc.run_id(r))
    for o in (dict(WIDE_CACHE=0), dict(WIDE_POOL_MAX=1)):
        with options(ctx, **o):
            same_bytes(fit(ctx, dev, r), base, (wc.run_id(r), o))


# ------------------------------------------ 3. the other ways to a basis

@pytest.mark.parametrize("r", NARROW, ids=wc.run_id)
def test_fit_jacobi_subset_bases(ctx, dev, r):
    """SF_OPT_FIT_SUBSET_DELETION = 0: every subset basis by the Jacobi
    solve."""
    with options(ctx, SUBSET_DELETION=0):
        check(fit(ctx, dev, r), wc.oracle(r), wc.run_id(r) + " jacobi")


@pytest.mark.parametrize("r", NARROW_PHASE, ids=wc.run_id)
def test_fit_general_kernel(ctx, dev, r):
    """SF_OPT_FIT_GENERAL = 1 (kl_fit.hip, kl_fit_exact.h): phase with any
    niter."""
    with options(ctx, GENERAL=1):
        got = fit(ctx, dev, r)
    check(got, wc.oracle(r), wc.run_id(r) + " general")
    if r.case in cc.NEAR_FILES:
        check(got, cc.reference(r), wc.run_id(r) + " general, reference")


@pytest.mark.parametrize("r", TEC, ids=wc.run_id)
def test_fit_general_kernel_tec_single_pass(ctx, dev, r):
    """... and tec with niter 1."""
    want = wc.run_oracle(r, niter=1)
    with options(ctx, GENERAL=1):
        got = fit(ctx, dev, r, niter=1)
    check(got, want, wc.run_id(r) + " general niter 1")
    if r.case == "tie_small":      # its golden is a single pass
        check(got, cc.reference(r), "tie_small tec general, reference")


# ----------------------------------- 4. two unflagged directions (Tie2)

@pytest.mark.parametrize("r", cc.all_runs(["tie_small", "tie_wide"]),
                         ids=wc.run_id)
def test_pairs_below_and_above_the_cutoff(ctx, dev, r):
    """A slot whose only two unflagged directions are the twin pair (|b| =
    2.3e-4), or whose second weight is 5e-4 (tie_small; once with
    cos(phi_2) < 0): every coefficient 0 and the residual the value bit for
    bit (the value - 1 of an amplitude), as the reference has it
    (near_tie4.npz).  Any other pair: the e_2 rule, a residual of 0 (to
    rounding) at the second.  On the pass kernel (D = 4: fast,
    non-uniform and slow class) and the workgroup-per-slot kernel (D = 64);
    phase, tec, amplitude."""
    coef, resid, w_out, orders = fit(ctx, dev, r)
    zero, kept = cc.pair_slots(r)
    assert zero.sum() >= 2 and kept.sum() >= 4
    cc.check_pairs(r, coef, resid, orders)
    if r.val.shape[-1] <= 60 and r.type != "amplitude":
        with options(ctx, GENERAL=1):
            g = fit(ctx, dev, r)
        cc.check_pairs(r, g[0], g[1], g[3])


# ------------------------------------------------------------ 5. rank 0

def test_rank_zero(ctx, dev):
    """r_0 = 1e6 at D = 20: no eigenvalue passes.  Every coefficient is 0,
    the residual of a fitted slot is the referenced phase bit for bit
    (phi - 0), the flags and orders are the oracle's."""
    r = cc.runs("r0_1e6")[0]
    coef, resid, w_out, orders = fit(ctx, dev, r)
    assert np.all(coef == 0.0)
    fitted = wc.fitted(r)
    want = cc.referenced(r)
    assert np.array_equal(resid[fitted].view(np.uint8),
                          np.ascontiguousarray(want[fitted]).view(np.uint8))
    _, _, o_w, o_orders = wc.oracle(r)
    np.testing.assert_array_equal(w_out, o_w)
    np.testing.assert_array_equal(orders, o_orders)
    assert (w_out == 0).sum() > (r.weight == 0).sum()


# ----------------------------------------- 5. the pseudo-inverse itself

@pytest.mark.parametrize("name", ["r0_1e4", "r0_1e5", "r0_1e6", "twins20",
                                  "dup12", "d50_r0_1e4", "d80_r0_1e4",
                                  "d128_r0_1e4"])
def test_get_basis_truncated(ctx, name):
    """sf_get_basis on a truncated basis, narrow and wide: pinv_c is
    pinv(C, atol = 1e-3) and C pinv_c the projector of that rank."""
    r = cc.runs(name)[0]
    D = r.val.shape[-1]
    if D > 60:
        ctx.set_basis_wide(r.pp, r.r_0, r.beta)
    else:
        ctx.set_basis(r.pp, r.r_0, r.beta)
    c, pinv_c, u, eig = ctx.get_basis()
    want = wc.okl.pinv_abs(c)
    err = np.abs(pinv_c - want).max()
    trace = np.trace(c @ pinv_c)
    print(f"{name}: D {D} rank {cc.RANK[name]} |pinv|max {np.abs(want).max():.3g} "
          f"err {err:.3g} trace {trace!r} |eig| kept "
          f"{int((np.abs(eig) > 1e-3).sum())}")
    assert int((np.abs(eig) > 1e-3).sum()) == cc.RANK[name] < D
    assert err <= 1e-9 * np.abs(want).max()
    assert abs(trace - cc.RANK[name]) <= 1e-9
