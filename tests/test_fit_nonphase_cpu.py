"""tec and amplitude fits in every direction regime and in station shards, on
the CPU: the oracle against the reference's own runs, the checks that make
the oracle-only inputs of tests/nonphase_cases.py fair ones for the kernels'
tests (tests/test_fit_nonphase.py), and what a tec shard with ref_ant = -1
has to compute.

Validity, asserted on the oracle as in tests/test_fit_walk_cpu.py:
 (a) oracle-only runs: the walk moves -- at least a quarter of the fitted
     slots end at an order other than min(station_order, n_unflagged - 1) --
     and a later pass flags at least one direction (the block sigma acts);
 (b) every run: values perturbed by 1e-10 (relative) change no order and no
     flag;
 (c) every run: no slot is ill-conditioned
     (test_oracle_golden.ill_conditioned_slots).
So no slot is excluded from any comparison, here or on the GPU.

The shard expectation (quirk Q15, stationscreen.py:993-996): a tec soltab
with ref_ant = -1 is referenced to the LAST station of the whole soltab.  A
station shard therefore equals the unsharded run only with that station's
values in hand; on its own it computes something else, except the shard that
holds the last station.

Tolerance of the oracle against the reference: that of
tests/test_fit_walk_cpu.py (coefficients 1e-9 x max(1, |coef|max), residuals
1e-9); orders and flagged weights identical.
"""

import numpy as np
import pytest

import nonphase_cases as nc
import walk_cases as wc
from test_oracle_golden import ill_conditioned_slots

RUNS = nc.all_runs()
GOLDEN_RUNS = list(nc.golden_runs())
ORACLE_RUNS = nc.all_oracle_runs()
NOREF = [r for r in RUNS if r.type == "tec" and r.ref == -1]


def test_every_case_of_the_issue_is_there():
    T, F = True, False
    got = {(r.case, r.group, r.niter, r.nsigma, r.adjust) for r in GOLDEN_RUNS}
    want = {("tec14", c, 3, 5.0, T) for c in ("ref", "noref")}
    want |= {("walk14tec", c, *p) for c in ("ref", "noref")
             for p in [(3, 5.0, T), (4, 3.0, T), (4, 3.0, F)]}
    want |= {("walk14amp", "amp", *p) for p in [(3, 5.0, T), (4, 3.0, T), (4, 3.0, F)]}
    want |= {("ties4tec", "ref", 3, 5.0, T), ("wide_fit80amp", "amp", 3, 5.0, T)}
    want |= {("wide_fit80tec", c, 3, 5.0, T) for c in ("ref", "noref")}
    assert got == want
    assert all(r.coef is not None for r in GOLDEN_RUNS)
    assert sorted(nc.ORACLE_T) == [8, 33, 60, 61, 128]
    for D, T_ in nc.ORACLE_T.items():
        tec_ref, tec_noref, amp = nc.oracle_runs(D)
        assert T_ * D > 256
        assert tec_ref.val.shape == tec_noref.val.shape == (T_, 2, 4, D)
        assert amp.val.shape == (T_, 2, 8, D) and amp.n_pol == 2
        assert (tec_ref.type, tec_ref.ref) == ("tec", 1)
        assert (tec_noref.type, tec_noref.ref) == ("tec", -1)
        assert (amp.type, amp.ref) == ("amplitude", -1)
        assert np.all(amp.val > 0)
        for r in (tec_ref, tec_noref, amp):
            assert r.coef is None
            assert r.order == (3 if D == 8 else min(20, D - 1))
            assert (r.niter, r.nsigma, r.adjust) == (4, 3.0, True)
        for r in (tec_ref, tec_noref):
            (f0, a0), (f1, a1) = r.skipped
            assert np.isnan(r.val[:, f0, a0]).all()
            assert np.isnan(r.val).sum() == T_ * D
            assert not r.weight[:, f1, a1].any()
            assert r.weight[:, f0, a0].any()


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


@pytest.mark.parametrize("r", ORACLE_RUNS, ids=wc.run_id)
def test_validity_a_the_walk_moves_and_later_passes_flag(r):
    _, _, w_out, orders = wc.oracle(r)
    fit = nc.fit_mask(r)
    n_fit = int(fit.sum())
    n_walk = int((wc.walked(r, w_out, orders) & fit).sum())
    n_flag = int(((w_out == 0) & (r.weight > 0)).sum())
    print(wc.run_id(r), "walked", n_walk, "of", n_fit, "later-pass flags", n_flag)
    assert 4 * n_walk >= n_fit
    assert n_flag >= 1
    # a later pass flags fitted slots only
    assert not ((w_out != r.weight).any(axis=-1) & ~fit).any()


@pytest.mark.parametrize("r", ORACLE_RUNS, ids=wc.run_id)
def test_skipped_blocks_stay_empty(r):
    coef, resid, w_out, orders = wc.oracle(r)
    for f, a in r.skipped:
        assert not coef[:, f, a].any() and not resid[:, f, a].any()
        assert not orders[:, f, a].any()
        np.testing.assert_array_equal(w_out[:, f, a], r.weight[:, f, a])
    assert not np.isnan(coef).any() and not np.isnan(resid).any()
    assert len(r.skipped) == (2 if r.type == "tec" else 0)


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


def test_the_station_split():
    assert nc.shards(3) == [(0, 1), (1, 3)]
    assert nc.shards(4) == [(0, 1), (1, 2), (2, 4)]
    assert nc.shards(6) == [(0, 1), (1, 4), (4, 6)]
    assert nc.shards(8) == [(0, 1), (1, 6), (6, 8)]


@pytest.mark.parametrize("r", NOREF, ids=wc.run_id)
def test_noref_tec_shard_needs_the_global_last_station(r):
    """With the last station of the soltab appended a shard reproduces its
    slice of the unsharded run exactly; alone, every shard that lacks that
    station computes something else."""
    full = wc.expected(r) if r.coef is None else wc.oracle(r)
    A = r.val.shape[2]
    for a0, a1 in nc.shards(A):
        last_inside = a1 == A
        sub = nc.sub_run(r, a0, a1, None if last_inside else A - 1)
        got = wc.run_oracle(sub)
        for x, y, name in zip(got, full, ("coef", "resid", "w_out", "orders")):
            assert np.array_equal(x[:, :, :a1 - a0], y[:, :, a0:a1],
                                  equal_nan=True), (a0, a1, name)
        alone = nc.oracle_alone(r, a0, a1)
        if last_inside:
            for x, y in zip(alone, got):
                assert np.array_equal(x, y)
        else:
            assert not np.array_equal(alone[0], full[0][:, :, a0:a1])
            assert not np.array_equal(alone[1], full[1][:, :, a0:a1])
