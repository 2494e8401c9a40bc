"""KL eigenvalues at and below the pinv cutoff, on the CPU: the checks that
make the inputs of tests/cutoff_cases.py fair ones for the kernels' tests
(tests/test_fit_cutoff.py), and the oracle against the reference's own runs
of ``twins20`` and ``tie_small`` (tests/golden/make_golden_near.py).

Every fit drops the components of C with a singular value <= 1e-3
(``pinv(C, rcond=1e-3)``, scipy >= 1.7: an absolute cutoff).  Whether a
value near 1e-3 is kept is a decision like a flag: a kernel may only be held
to the oracle where the oracle's own result does not hang on rounding.  So,
for every Run:

 (a) the rank of the full C is the stated one and below D, and no singular
     value lies within 1e-4 (relative) of the cutoff;
 (b) the oracle's orders and flags are the same at r_0 x (1 +- 1e-6) -- which
     moves every eigenvalue of every subset by -+ 1.7e-6 relative -- and under
     a 1e-10 (relative) perturbation of the values, and its coefficients and
     residuals move by less than the kernels' tolerance (1e-8 x max(1,
     |coef|max), 1e-8);
 (c) at rank 0 the coefficients are zero and the residuals the referenced
     values.
No slot is excluded from any of these.

Tolerance of the oracle against the reference: that of
tests/test_oracle_golden.py (coefficients 1e-9 x max(1, |coef|max),
residuals 1e-9); orders and flagged weights identical.
"""

import numpy as np
import pytest

import cutoff_cases as cc
import walk_cases as wc
from oracle import geometry as og
from oracle import kl as okl

RUNS = cc.all_runs()
NEAR_RUNS = cc.all_runs(list(cc.NEAR_FILES))
CUTOFF = okl.PINV_ATOL


def test_every_case_of_the_issue_is_there():
    shapes = {(r.case, r.group): (r.val.shape, r.r_0) for r in RUNS}
    small = (7, 3, 5)
    want = {("r0_1e4", "phase"): (small + (20,), 1e4),
            ("r0_1e5", "phase"): (small + (20,), 1e5),
            ("r0_1e6", "phase"): (small + (20,), 1e6),
            ("d7_r0_1e5", "phase"): (small + (7,), 1e5),
            ("d23_r0_1e5", "phase"): (small + (23,), 1e5),
            ("d50_r0_1e4", "phase"): ((4, 1, 3, 50), 1e4),
            ("d80_r0_1e4", "phase"): ((4, 1, 3, 80), 1e4),
            ("d128_r0_1e4", "phase"): ((4, 1, 3, 128), 1e4),
            ("mixed20_r0_1e4", "phase"): (small + (20,), 1e4),
            ("tec14_r0_1e4", "tec"): ((6, 2, 4, 14), 1e4),
            ("amp14_r0_1e4", "amp"): ((6, 2, 8, 14), 1e4),
            ("twins20", "phase"): (small + (20,), 100.0),
            ("twins20", "tec"): (small + (20,), 100.0),
            ("twins20", "amp"): ((7, 2, 10, 20), 100.0),
            ("dup12", "phase"): (small + (12,), 100.0),
            ("tie_small", "phase"): (small + (4,), 100.0),
            ("tie_small", "tec"): (small + (4,), 100.0),
            ("tie_small", "amp"): ((7, 3, 10, 4), 100.0),
            ("tie_wide", "phase"): ((4, 1, 3, 64), 100.0),
            ("tie_wide", "tec"): ((4, 1, 3, 64), 100.0),
            ("tie_wide", "amp"): ((4, 1, 6, 64), 100.0)}
    assert shapes == want
    for r in RUNS:
        if r.case not in ("tie_small", "tie_wide"):
            assert (r.niter, r.nsigma, r.adjust) == (3, 3.0, True)
    mixed = cc.runs("mixed20_r0_1e4")[0].weight
    assert set(np.unique(mixed).tolist()) == {0.0, float(np.float32(5e-4)), 400.0}
    assert 5 <= (mixed == np.float32(5e-4)).sum() <= 40


@pytest.mark.parametrize("r", RUNS, ids=wc.run_id)
def test_validity_a_rank_and_margin(r):
    sv = cc.singular_values(r)
    D = r.val.shape[-1]
    rank = int((sv > CUTOFF).sum())
    margin = np.abs(sv / CUTOFF - 1.0).min()
    print(wc.run_id(r), "rank", rank, "of", D, "nearest to the cutoff",
          margin, "smallest", sv.min())
    assert rank == cc.RANK[r.case] < D
    assert margin > 1e-4


def test_twins20_geometry_and_flags():
    """The pairs are 1 and 2 units apart (b = -2.3e-4 and -7.4e-4); every
    kind of slot is there; a subset without one twin of each pair has full
    rank, one without a whole pair or with a pair left has not."""
    r = cc.runs("twins20")[0]
    for (twin, partner, dist), b in zip(cc.TWINS20, (2.3e-4, 7.4e-4)):
        d = np.linalg.norm(r.pp[twin] - r.pp[partner])
        assert abs(d - dist) < 0.05
        c = okl.calculate_svd(r.pp[[twin, partner]], r.r_0, r.beta)[0]
        assert c[0, 1] < 0 and abs(-c[0, 1] / b - 1) < 0.1 and -c[0, 1] < CUTOFF
    (t1, p1, _), (t2, p2, _) = cc.TWINS20
    un = r.weight > 0
    fit = wc.fitted(r)
    one_each = fit & ~un[..., t1] & ~un[..., t2] & un[..., p1] & un[..., p2]
    one = fit & ~un[..., t1] & un[..., t2] & un[..., p1] & un[..., p2]
    both = fit & ~un[..., t1] & ~un[..., p1] & un[..., t2] & un[..., p2]
    whole = fit & un.all(axis=-1)
    print("twins20 slots: one twin of each pair", one_each.sum(), "one twin",
          one.sum(), "both of a pair", both.sum(), "unflagged", whole.sum())
    assert min(one_each.sum(), one.sum(), both.sum()) >= 8 and whole.sum() >= 20
    for sel, full in ((one_each, True), (one, False), (both, False)):
        for idx in np.argwhere(sel):
            keep = np.where(un[tuple(idx)])[0]
            sv = cc.singular_values(r, keep)
            assert (sv.min() > CUTOFF) == full, (idx, sv.min())
            assert np.abs(sv / CUTOFF - 1.0).min() > 1e-4


def test_dup12_has_a_zero_eigenvalue():
    r = cc.runs("dup12")[0]
    a, b = cc.DUP12
    assert np.array_equal(r.pp[a], r.pp[b])
    c = okl.calculate_svd(r.pp, r.r_0, r.beta)[0]
    assert np.array_equal(c[a], c[b]) and c[a, b] == 0.0
    sv = cc.singular_values(r)
    assert sv[-1] < 1e-12 and sv[-2] > 0.1


@pytest.mark.parametrize("r", cc.all_runs(["tie_small", "tie_wide"]),
                         ids=wc.run_id)
def test_tie_pairs(r):
    """Slots whose only two unflagged directions are the twin pair (|b|
    below the cutoff) beside slots whose only two are an ordinary pair; in
    tie_small in the fast, the non-uniform and the slow (a weight of 5e-4)
    class."""
    un = r.weight > 0
    two = wc.fitted(r) & (un.sum(axis=-1) == 2)
    twin, partner, _ = cc.TIE_TWIN
    tw = two & un[..., twin] & un[..., partner]
    print(wc.run_id(r), "two unflagged", two.sum(), "of which twins", tw.sum())
    small = r.case == "tie_small"
    assert tw.sum() >= (10 if small else 2)
    assert (two & ~tw).sum() >= (20 if small else 4)
    b = okl.calculate_svd(r.pp[[twin, partner]], r.r_0, r.beta)[0][0, 1]
    assert 2.0e-4 < -b < 2.6e-4
    for idx in np.argwhere(two & ~tw):
        keep = np.where(un[tuple(idx)])[0]
        assert cc.singular_values(r, keep).min() > 1.0
        # the U of the pair is the exact permutation (no rounding residue
        # for the screen's atan2 to amplify: make_golden_ties.py)
        u = okl.calculate_svd(r.pp[keep], r.r_0, r.beta)[2]
        assert np.all((u == 0.0) | (np.abs(u) == 1.0))
    if small:
        w2 = r.weight[two]
        assert (w2.max(axis=-1) != np.where(w2 > 0, w2, np.inf).min(axis=-1)).any()
        assert (r.weight[tw] == np.float32(5e-4)).any()


def perturbed(r):
    rng = np.random.default_rng(1)
    val = r.val * (1.0 + 1e-10 * rng.standard_normal(r.val.shape))
    return (("r_0 x (1 + 1e-6)", dict(r_0=r.r_0 * (1.0 + 1e-6))),
            ("r_0 x (1 - 1e-6)", dict(r_0=r.r_0 * (1.0 - 1e-6))),
            ("values x (1 + 1e-10 n)", dict(val=val)))


@pytest.mark.parametrize("r", RUNS, ids=wc.run_id)
def test_validity_b_the_oracle_alone_decides(r):
    coef, resid, w_out, orders = wc.oracle(r)
    scale = max(1.0, np.abs(coef).max())
    for what, kw in perturbed(r):
        c2, r2, w2, o2 = wc.run_oracle(r, **kw)
        # r_0 scales C and 1 / C against each other: the screen C pinv(C) x
        # stays, the coefficients pinv(C) x scale by (1 +- 1e-6)^beta, which
        # is taken out before they are compared
        if "r_0" in kw:
            c2 = c2 * (kw["r_0"] / r.r_0) ** -r.beta
        cerr, rerr = np.abs(c2 - coef).max(), np.abs(r2 - resid).max()
        print(wc.run_id(r), what, "d coef", cerr, "allowed", 1e-8 * scale,
              "d resid", rerr)
        np.testing.assert_array_equal(o2, orders)
        np.testing.assert_array_equal(w2, w_out)
        assert cerr <= 1e-8 * scale
        assert rerr <= 1e-8


def test_validity_c_rank_zero():
    r = cc.runs("r0_1e6")[0]
    coef, resid, w_out, _ = wc.oracle(r)
    assert np.all(coef == 0.0)
    fit = wc.fitted(r)
    assert np.array_equal(resid[fit], cc.referenced(r)[fit])
    assert (w_out == 0).sum() > (r.weight == 0).sum()


# ------------------------------------------- the reference's own runs

@pytest.mark.parametrize("name", list(cc.NEAR_FILES))
def test_golden_inputs_are_the_cases(name):
    g, inp = cc.near_golden(name), cc.inputs(name)
    pp, _, _ = og.piercepoints(inp["dir_radec"])
    np.testing.assert_allclose(pp, g["piercepoints"], rtol=0, atol=1e-8)
    assert float(g["r_0"]) == 100.0 and float(g["beta"]) == 5.0 / 3.0
    for k in ("dir_radec", "ant_pos"):
        assert np.array_equal(g[k], inp[k])
    for group, d in inp["groups"].items():
        for k in ("weight", "ref_ant", "order", "niter", "nsigma"):
            assert np.array_equal(g[f"{group}_{k}"], d[k]), (group, k)
        # make_solutions' matrix products: the last bit is the BLAS's
        np.testing.assert_allclose(g[f"{group}_val"], d["val"], rtol=0,
                                   atol=1e-14)
        assert bool(g[f"{group}_adjust"]) == d["adjust"]


def test_golden_files_stay_small():
    """None larger than the largest walk golden."""
    import os
    size = lambda f: os.path.getsize(os.path.join(cc.GOLDEN, f + ".npz"))  # noqa: E731
    cap = max(size(f) for f in wc.GOLDEN_FILES)
    for files in cc.NEAR_FILES.values():
        for f in files:
            assert size(f) <= cap, (f, size(f), cap)


@pytest.mark.parametrize("r", NEAR_RUNS, ids=wc.run_id)
def test_oracle_vs_reference(r):
    coef, resid, w_out, orders = wc.oracle(r)
    g_coef, g_resid, g_w, g_orders = cc.reference(r)
    np.testing.assert_array_equal(orders, g_orders)
    np.testing.assert_array_equal(w_out, g_w)
    scale = max(1.0, np.abs(g_coef).max())
    cerr = np.abs(coef - g_coef).max()
    rerr = np.abs(resid - g_resid).max()
    print(wc.run_id(r), "coef err", cerr, "resid err", rerr, "scale", scale)
    assert cerr <= 1e-9 * scale
    assert rerr <= 1e-9


@pytest.mark.parametrize("r", cc.runs("tie_small"), ids=wc.run_id)
def test_reference_zeroes_a_pair_below_the_cutoff(r):
    """What the reference itself gives on a slot whose two unflagged
    directions are the twin pair, or whose second weight is 5e-4: pinv(C_sub)
    or inv_u is 0, so the screen is atan2(0, 0) = 0 (not +-pi: the zeros its
    BLAS leaves are +0, also where cos(phi_2) < 0), every coefficient 0 and
    the residual the value itself (minus 10^0 for an amplitude).  Any other
    pair keeps the e_2 rule.  The oracle gives the same."""
    zero, kept = cc.pair_slots(r)
    tiny2 = zero & (r.weight[..., 2] == 0)
    print(wc.run_id(r), "zero fits", zero.sum(), "of which an ordinary pair",
          tiny2.sum(), "e_2 fits", kept.sum())
    assert tiny2.sum() >= 4 and (zero & ~tiny2).sum() >= 10 and kept.sum() >= 20
    if r.type == "phase":
        # ... one of them with cos(phi_2) < 0
        assert (np.cos(cc.referenced(r)[tiny2][:, 1]) < -0.5).sum() == 1
    g_coef, g_resid, _, g_orders = cc.reference(r)
    cc.check_pairs(r, g_coef, g_resid, g_orders)
    coef, resid, _, orders = wc.oracle(r)
    cc.check_pairs(r, coef, resid, orders)
