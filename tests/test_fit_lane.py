"""The lane-per-slot phase fit (csrc/kl_fit_lane.hip, SF_OPT_FIT_LANE).

A phase fit with 3..23 directions gives every slot that starts with no flagged
direction and one weight to a kernel that fits one slot per lane, and hands
the slot back to the pass kernel where its order walk moves or a phase is not
finite.  The ABI promises the bytes of the pass kernel, so every test here
fits twice, option on (the default) and off, and compares the bytes of coef,
resid, w_out and order_out and the number of masks decomposed; where the
oracle applies the result is also held against it with the criterion of
tests/test_fit_walk.py (orders and w_out identical, |d coef| <= 1e-8 x
max(1, |coef|max), |d resid| <= 1e-8).

Shapes: 105 slots (5 stations x 7 times x 3 frequencies) -- two wavefronts of
the lane kernel, the second with 41 slots, the reference station's slots in
both.  sf_get_fit_lane_stats' counts are held against what the input fixes:
n_lane is the number of fitted slots with every weight positive, and a slot
whose final order is not min(station order, unflagged - 1) walked
(walk_cases.walked), so it was handed back.
Needs an MI355X: every test is marked ``gpu``.
"""

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import walk_cases as wc
from test_fit_walk import check, same_bytes
from test_wide_fit import wide_fit

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LANE_MAX_D = 23  # kLaneMaxD, csrc/kl_fit_lane.h


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


@functools.lru_cache(maxsize=None)
def solutions(n_dir, scale=1.0, outlier_frac=0.02, tiny_weight_frac=0.0):
    """A Run (walk_cases) of 5 x 7 x 3 slots of make_solutions; shared, do
    not modify."""
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    s = make_solutions(n_ant=5, n_time=7, n_freq=3, n_dir=n_dir, seed=11,
                       flag_frac=0.02, outlier_frac=outlier_frac,
                       tiny_weight_frac=tiny_weight_frac)
    weight = (s.weight * np.float32(scale)).astype(np.float32)
    pp, _, _ = wc.og.piercepoints(s.dir_radec)
    ref = wc.okl.reference_station(weight)
    order = min(20, n_dir - 1)
    return SimpleNamespace(
        case=f"lane{n_dir}", group="phase", k=0, type="phase", ref=ref,
        scaled=scale != 1.0, n_pol=1, val=s.val, weight=weight,
        ant_pos=s.ant_pos, pp=pp, order=order,
        st=wc._st_orders(s.ant_pos, ref, order), beta=5.0 / 3.0, r_0=100.0,
        niter=2, nsigma=5.0, adjust=True, coef=None, resid=None, w_out=None,
        orders=None)


def eligible(r, weight=None):
    """[T, F, A] bool: fitted slots the classify kernel gives to the lanes."""
    w = r.weight if weight is None else weight
    return wc.fitted(r) & (w > 0).all(axis=-1) & (w.max(axis=-1) == w.min(axis=-1))


def fit_on_off(ctx, dev, r, val=None, weight=None, **kw):
    """The fit with the lane kernel on and off -> (on, off, lane stats of the
    on fit); asserts the bytes and the mask counts equal."""
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_FIT_LANE
    val = r.val if val is None else val
    weight = r.weight if weight is None else weight
    prm = dict(niter=r.niter, nsigma=r.nsigma, adjust_order=r.adjust)
    prm.update(kw)
    D = val.shape[-1]
    if D > 60:
        ctx.set_basis_wide(r.pp, r.r_0, r.beta)
    else:
        ctx.set_basis(r.pp, r.r_0, r.beta)
    on = wide_fit(ctx, dev, val, weight, r.pp, r.st, r.ref, bind=False, **prm)
    lane = ctx.fit_lane_stats()
    masks_on = ctx.fit_stats()["n_masks"]
    ctx.set_option(SF_OPT_FIT_LANE, 0)
    try:
        off = wide_fit(ctx, dev, val, weight, r.pp, r.st, r.ref, bind=False, **prm)
        lane_off = ctx.fit_lane_stats()
        masks_off = ctx.fit_stats()["n_masks"]
    finally:
        ctx.set_option(SF_OPT_FIT_LANE, 1)
    shown = {k: v for k, v in prm.items() if k != "ref_phase"}
    print(f"D {D} {shown}: lane {lane} n_masks on {masks_on} off {masks_off}")
    same_bytes(on, off, ("lane on / off", D, prm))
    assert masks_on == masks_off
    assert lane_off == {"n_lane": 0, "n_deferred": 0}
    return on, off, lane


@pytest.mark.parametrize("scale", [1.0, 400.0], ids=["w1", "w400"])
@pytest.mark.parametrize("adjust", [True, False], ids=["adj", "fix"])
@pytest.mark.parametrize("nsigma", [5.0, 3.0])
@pytest.mark.parametrize("niter", [1, 2, 4])
def test_lane_fit_keeps_every_bit(ctx, dev, niter, nsigma, adjust, scale):
    """D = 20 at niter 1, 2, 4, nsigma 5 and 3, the walk on and off, with
    weights of 1 (the walk stays) and of 400 (it moves): the bytes of the pass
    kernel, the oracle's result, and the counts the input fixes."""
    r = solutions(20, scale)
    prm = dict(niter=niter, nsigma=nsigma, adjust_order=adjust)
    on, _, lane = fit_on_off(ctx, dev, r, **prm)
    want = wc.run_oracle(r, **prm)
    check(on, want, f"lane20 x{scale:g} {prm}")
    n_lane = int(eligible(r).sum())
    assert n_lane > 40  # 49 of the 84 fitted slots start unflagged
    assert lane["n_lane"] == n_lane
    walked = int((wc.walked(r, want[2], want[3]) & eligible(r)).sum())
    print(f"eligible {n_lane} of which walked (oracle) {walked}")
    assert lane["n_deferred"] >= walked
    assert lane["n_lane"] > lane["n_deferred"]
    if scale == 400.0 and adjust and niter > 1:
        # the walk moves: some lane slots go back, most stay
        assert walked > 0
        assert lane["n_deferred"] > 0
    if not adjust or niter == 1:
        assert lane["n_deferred"] == 0  # no walk, finite phases


@pytest.mark.parametrize("n_dir", [3, 7, 14, LANE_MAX_D])
def test_lane_fit_direction_counts(ctx, dev, n_dir):
    """The ends of the instantiated range (3 and the cap), 7 and 14."""
    r = solutions(n_dir, 400.0)
    prm = dict(niter=3, nsigma=3.0, adjust_order=True)
    on, _, lane = fit_on_off(ctx, dev, r, **prm)
    check(on, wc.run_oracle(r, **prm), f"lane{n_dir}")
    assert lane["n_lane"] == int(eligible(r).sum()) > 0


@pytest.mark.parametrize("n_dir", [LANE_MAX_D + 1, 33])
def test_no_lane_kernel_above_the_cap(ctx, dev, n_dir):
    """One direction above the cap and D = 33 (one slot per wavefront in the
    pass kernel): no lane slots, no list, the same fit."""
    r = solutions(n_dir, 400.0)
    _, _, lane = fit_on_off(ctx, dev, r, niter=3, nsigma=3.0, adjust_order=True)
    assert lane == {"n_lane": 0, "n_deferred": 0}


def test_non_finite_phases_go_back(ctx, dev):
    """A NaN and an infinite phase in two unflagged slots among ordinary
    ones: both slots are handed back before pass 0."""
    r = solutions(20)
    el = np.argwhere(eligible(r))
    val = r.val.copy()
    val[tuple(el[3])][5] = np.nan
    val[tuple(el[40])][0] = np.inf
    _, _, lane = fit_on_off(ctx, dev, r, val=val, niter=2, nsigma=5.0,
                            adjust_order=False)
    assert lane["n_lane"] == int(eligible(r).sum())
    assert lane["n_deferred"] == 2


def test_lane_fit_with_reference_phases(ctx, dev):
    """Both ways of referencing: ref_ant a station of the array, and the
    reference phases passed in -- the same bytes."""
    r = solutions(20, 400.0)
    prm = dict(niter=3, nsigma=3.0, adjust_order=True)
    by_ant, _, lane_a = fit_on_off(ctx, dev, r, **prm)
    refph = torch.from_numpy(np.ascontiguousarray(r.val[:, :, r.ref, :])).to(dev)
    by_ph, _, lane_p = fit_on_off(ctx, dev, r, ant_offset=0, ref_phase=refph, **prm)
    same_bytes(by_ph, by_ant, "ref_phase / ref_ant")
    assert lane_a == lane_p and lane_a["n_lane"] > 0


def test_lane_fit_beside_slow_and_non_uniform_slots(ctx, dev):
    """Tiny weights (the slow class) and slots with unequal weights (the
    general layout of the fast pass) in the same call: neither is a lane
    slot, and the lane slots beside them keep their bytes."""
    r = solutions(20, tiny_weight_frac=0.02)
    weight = r.weight.copy()
    plain = np.argwhere(eligible(r))
    for i in (1, 10, 20):
        weight[tuple(plain[i])][::2] = np.float32(3.0)
    prm = dict(niter=3, nsigma=3.0, adjust_order=True)
    on, _, lane = fit_on_off(ctx, dev, r, weight=weight, **prm)
    assert ctx.fit_stats()["n_general"] > 0
    n_lane = int(eligible(r, weight).sum())
    assert 0 < n_lane == int(eligible(r).sum()) - 3
    assert lane["n_lane"] == n_lane
    assert ((r.weight > 0) & (r.weight < 1e-3)).any()


def test_lane_fit_many_outliers(ctx, dev):
    """outlier_frac 0.2: most lane slots lose directions in pass 0 and go on
    through the later passes in the lane (new masks every pass)."""
    r = solutions(20, outlier_frac=0.2)
    prm = dict(niter=4, nsigma=3.0, adjust_order=True)
    on, _, lane = fit_on_off(ctx, dev, r, **prm)
    check(on, wc.run_oracle(r, **prm), "lane20 outliers 0.2")
    el = eligible(r)
    assert lane["n_lane"] == int(el.sum()) > 0
    lost = el & ((on[2] > 0).sum(axis=-1) < 20)
    print(f"lane slots {int(el.sum())}, of which lost a direction {int(lost.sum())}")
    assert lost.sum() * 2 > el.sum()
