"""The order walk of ``adjust_order`` and fit parameters off their defaults,
on the CPU: the oracle against the reference's own runs
(tests/golden/make_golden_walk.py), and the checks that make these inputs
fair ones for the kernels' tests (tests/test_fit_walk.py).

With weights near 1 / sigma^2 the reduced chi^2 of a fit is near 1 and the
walk (stationscreen.py:700-782) moves the order: re-fits, sign flips, the
double-bound stop.  With the weights of ``make_solutions`` it never does.

Validity of every case and parameter set, asserted on the oracle:
 (a) the walk moves: at least a quarter of the fitted slots end at an order
     other than min(station_order, n_unflagged - 1) (scaled weights,
     adjust_order on); the cascade reaches 0, 1, 2 and 3 unflagged
     directions at least 3 times each;
 (b) no decision is marginal: values perturbed by 1e-10 (relative) change
     no order and no flag;
 (c) no slot is ill-conditioned (test_oracle_golden.ill_conditioned_slots).
So no slot is excluded from any comparison.

Tolerance of the oracle against the reference: that of
tests/test_oracle_golden.py (coefficients 1e-9 x max(1, |coef|max),
residuals 1e-9); orders and flagged weights identical.
"""

import numpy as np
import pytest

import walk_cases as wc
from test_oracle_golden import ill_conditioned_slots

RUNS = wc.all_runs()
GOLDEN_RUNS = [r for r in RUNS if r.coef is not None]


def test_every_case_of_the_issue_is_there():
    got = {(r.case, r.group, r.niter, r.nsigma, r.adjust) for r in RUNS}
    T, F = True, False
    want = {("walk20", "phase", *p) for p in
            [(2, 5.0, T), (4, 3.0, T), (4, 3.0, F), (1, 5.0, F), (4, 1e9, T)]}
    want |= {("walk20mixed", "phase", *p) for p in [(2, 5.0, T), (4, 3.0, T)]}
    want |= {("cascade12", "phase", *p) for p in [(8, 1.5, T), (8, 1.5, F)]}
    want |= {("walk50", "phase", *p) for p in [(2, 5.0, T), (4, 3.0, T)]}
    want |= {("walk20beta", "phase", 3, 3.0, T)}
    want |= {("walk14tec", c, *p) for c in ("ref", "noref")
             for p in [(3, 5.0, T), (4, 3.0, T), (4, 3.0, F)]}
    want |= {("walk14amp", "amp", *p) for p in [(3, 5.0, T), (4, 3.0, T), (4, 3.0, F)]}
    want |= {("walk80", c, *p) for c in ("phase", "tec")
             for p in [(3, 5.0, T), (4, 3.0, T)]}
    want |= {("oracle60", "phase", 4, 3.0, T), ("oracle128", "phase", 4, 3.0, T)}
    assert got == want
    shapes = {r.case: r.val.shape for r in RUNS}
    assert shapes["walk20"] == (8, 2, 5, 20) and shapes["cascade12"] == (8, 2, 5, 12)
    assert shapes["walk50"] == (6, 1, 4, 50) and shapes["walk80"] == (4, 1, 3, 80)
    assert shapes["walk14tec"] == (6, 2, 4, 14) and shapes["walk14amp"] == (6, 2, 8, 14)
    assert shapes["oracle60"] == (4, 1, 3, 60) and shapes["oracle128"] == (2, 1, 3, 128)
    beta = {r.case: r.beta for r in RUNS}
    assert beta.pop("walk20beta") == 1.0 and set(beta.values()) == {5.0 / 3.0}
    mixed = wc.runs("walk20mixed")[0].weight
    assert set(np.unique(mixed).tolist()) == {0.0, float(np.float32(5e-4)),
                                              100.0, 400.0, 1600.0}
    assert 5 <= (mixed == np.float32(5e-4)).sum() <= 40


@pytest.mark.parametrize("r", GOLDEN_RUNS, ids=wc.run_id)
def test_oracle_vs_reference(r):
    coef, resid, w_out, orders = wc.oracle(r)
    np.testing.assert_array_equal(orders, r.orders)
    np.testing.assert_array_equal(w_out, r.w_out)
    scale = max(1.0, np.abs(r.coef).max())
    cerr = np.abs(coef - r.coef).max()
    rerr = np.abs(resid - r.resid).max()
    print(wc.run_id(r), "coef err", cerr, "resid err", rerr, "scale", scale)
    assert cerr <= 1e-9 * scale
    assert rerr <= 1e-9


@pytest.mark.parametrize("r", RUNS, ids=wc.run_id)
def test_validity_a_the_walk_moves(r):
    _, _, w_out, orders = wc.oracle(r)
    n_fit = int(wc.fitted(r).sum())
    n_walk = int(wc.walked(r, w_out, orders).sum())
    print(wc.run_id(r), "walked", n_walk, "of", n_fit)
    if r.scaled and r.adjust and r.niter > 1:
        assert 4 * n_walk >= n_fit
    else:
        # weights 1 (chi^2 ~ 0.003), adjust_order off or a single pass: no
        # slot leaves min(station_order, n_unflagged - 1)
        assert n_walk == 0
    if r.case == "cascade12":
        n = (w_out > 0).sum(axis=-1)[wc.fitted(r)]
        assert [int((n == k).sum()) for k in range(4)] == [10, 7, 6, 12]
        assert all((n == k).sum() >= 3 for k in range(4))
        # ... through flags of later passes, not of the input
        assert (r.weight > 0).sum(axis=-1).min() >= 10


@pytest.mark.parametrize("r", RUNS, ids=wc.run_id)
def test_validity_b_no_marginal_decision(r):
    _, _, w_out, orders = wc.oracle(r)
    rng = np.random.default_rng(1)
    val = r.val * (1.0 + 1e-10 * rng.standard_normal(r.val.shape))
    _, _, w2, o2 = wc.run_oracle(r, val=val)
    np.testing.assert_array_equal(o2, orders)
    np.testing.assert_array_equal(w2, w_out)


@pytest.mark.parametrize("r", RUNS, ids=wc.run_id)
def test_validity_c_no_ill_conditioned_slot(r):
    _, _, w_out, orders = wc.oracle(r)
    g = dict(piercepoints=r.pp, ref_ant=r.ref if r.type != "amplitude" else -1,
             orders=orders, w_out=w_out)
    assert ill_conditioned_slots(g, r.r_0, r.beta) == set()


def test_the_parameters_act_on_walk20():
    """adjust_order, nsigma and niter each change the reference's result on
    walk20 (so a kernel that ignored one would be caught), and a single pass
    is the same with and without adjust_order."""
    by = {(r.niter, r.nsigma, r.adjust): r for r in wc.runs("walk20")}
    on, off = by[(4, 3.0, True)], by[(4, 3.0, False)]
    assert not np.array_equal(on.orders, off.orders)
    assert not np.array_equal(on.coef, off.coef)
    assert not np.array_equal(on.w_out, by[(2, 5.0, True)].w_out)
    free = by[(4, 1e9, True)]
    np.testing.assert_array_equal(free.w_out, free.weight)
    assert (off.w_out == 0).sum() > (off.weight == 0).sum()
    one = by[(1, 5.0, False)]
    for a, b in zip(wc.run_oracle(one), wc.run_oracle(one, adjust_order=True)):
        assert np.array_equal(a, b)


def test_oracle_r0_and_beta_reach_the_basis():
    """r_0 has no golden (the reference fixes it at 100): the oracle at
    r_0 = 250 is a different, equally valid fit -- no ill-conditioned slot,
    stable under the 1e-10 perturbation -- for the kernels' test to use."""
    r = wc.runs("walk20")[1]
    a = wc.oracle(r)
    b = wc.run_oracle(r, r_0=250.0)
    assert not np.array_equal(a[0], b[0])
    g = dict(piercepoints=r.pp, ref_ant=r.ref, orders=b[3], w_out=b[2])
    assert ill_conditioned_slots(g, 250.0, r.beta) == set()
    assert 4 * wc.walked(r, b[2], b[3]).sum() >= wc.fitted(r).sum()
    rng = np.random.default_rng(1)
    val = r.val * (1.0 + 1e-10 * rng.standard_normal(r.val.shape))
    c = wc.run_oracle(r, val=val, r_0=250.0)
    np.testing.assert_array_equal(c[3], b[3])
    np.testing.assert_array_equal(c[2], b[2])
