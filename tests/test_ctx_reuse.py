"""One context walked through what its device buffers go through: growth, then
reuse of the larger buffers by a smaller call, new geometries of other sizes,
a fit pool that doubles while it holds entries, scratch of the tessellated
fill and the smoother, and create / destroy in a loop.  Every result is
compared bit for bit with a fresh context that did only that step (the pool
growth: with the oracle, at the tolerances of tests/test_wide_fit.py).
Needs an MI355X: every test is marked ``gpu``.
"""

import functools

import numpy as np
import pytest

from conftest import FIELD
from oracle import kl as okl
from test_wide_fit import check

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture
def ctx(dev):
    """Factory of private contexts on torch's stream, closed after the test."""
    from ska_sdp_screen_fitting_amd._lib import Context
    made = []

    def make():
        c = Context(0)
        c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        made.append(c)
        return c
    yield make
    for c in made:
        c.close()


@functools.lru_cache(maxsize=None)
def synth(D, T, F, A, seed=0, flag_frac=0.1, outlier_frac=0.05):
    """(solutions, piercepoints, reference station, station orders, screen
    centre); the directions depend on D and the seed only."""
    from ska_sdp_screen_fitting_amd import geometry
    from ska_sdp_screen_fitting_amd.stationscreen import station_orders
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    s = make_solutions(n_ant=A, n_time=T, n_freq=F, n_dir=D, seed=7000 + D + seed,
                       flag_frac=flag_frac, outlier_frac=outlier_frac)
    pp, mra, mdec = geometry.piercepoints(s.dir_radec)
    ref = okl.reference_station(s.weight)
    st = station_orders(s.ant_pos, ref, min(20, D - 1))
    return s, pp, ref, st, (mra, mdec)


def fit(c, dev, sol, outputs=True, niter=3, nsigma=5.0):
    """Phase fit of a synth() set on the bound basis -> host (coef, resid,
    w_out, order), or (coef,) with the other outputs left to the context."""
    s, _, ref, st, _ = sol
    T, F, A, _ = s.val.shape
    ph = torch.from_numpy(s.val).to(dev)
    wt = torch.from_numpy(s.weight).to(dev)
    coef = torch.full_like(ph, -7.0)
    outs = {}
    if outputs:
        outs = dict(resid=torch.full_like(ph, -7.0), w_out=torch.full_like(wt, -7.0),
                    order_out=torch.full((T, F, A), -7, dtype=torch.int32, device=dev))
    c.fit(ph, wt, T, F, A, st, niter=niter, nsigma=nsigma, ref_ant=ref, coef=coef, **outs)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (coef, *outs.values()))


def same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: output {k}")


# ------------------------------------------------- 1. growth, then reuse

def test_growth_then_reuse(ctx, dev):
    """(2, 1, 3), then (8, 2, 3) with the scratch outputs, then (2, 1, 3)
    again in the buffers the middle call left: the pairs replaced together,
    the reserve that finds room, the mask table at its earlier, larger power
    of two."""
    D = 12
    calls = [((2, 1, 3), True), ((8, 2, 3), False), ((2, 1, 3), True)]
    pp = synth(D, 2, 1, 3)[1]
    one = ctx()
    one.set_basis(pp)
    walked = []
    for shape, outputs in calls:
        sol = synth(D, *shape)
        assert np.array_equal(sol[1], pp)
        walked.append(fit(one, dev, sol, outputs=outputs))
        assert one.fit_stats()["n_masks"] > 0  # masks entered the pool
    for (shape, outputs), got in zip(calls, walked):
        fresh = ctx()
        fresh.set_basis(pp)
        same(got, fit(fresh, dev, synth(D, *shape), outputs=outputs), f"{shape}")
    same(walked[2], walked[0], "third call vs first")


# --------------------------------------------------- 2. geometry changes

def grid16(D):
    from ska_sdp_screen_fitting_amd import geometry
    mra, mdec = synth(D, 2, 1, 3)[4]
    x, y = geometry.grid_coords(FIELD["rad"], FIELD["dec"], FIELD["width"], 0.2, mra, mdec)
    return x[:16], y[:16]


def geometry_step(c, dev, kind, D):
    """Bind a geometry of D directions, fit where it has a basis, bind the
    16 x 16 grid and evaluate: (fit outputs or None, cube)."""
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_FIT_WIDE_CACHE, ScreenFitError
    sol = synth(D, 2, 1, 3)
    S = 2 * 1 * 3
    out = torch.full((S, 4, 16, 16), -7.0, dtype=torch.float32, device=dev)
    getattr(c, kind)(sol[1])
    with pytest.raises(ScreenFitError):  # the previous geometry's grid is gone
        c.eval(torch.zeros((S, D), dtype=torch.float64, device=dev), S, out)
    if kind == "set_piercepoints":
        with pytest.raises(ScreenFitError):
            fit(c, dev, sol)
        fitted = None
        coef = np.random.default_rng(D).normal(0.0, 0.01, (S, D))
    else:
        c.set_option(SF_OPT_FIT_WIDE_CACHE, 1)
        fitted = fit(c, dev, sol)
        coef = fitted[0].reshape(S, D)
    c.set_grid(*grid16(D))
    c.eval(torch.from_numpy(coef).to(dev), S, out)
    torch.cuda.synchronize()
    cube = out.cpu().numpy()
    assert not (cube == -7.0).any()
    return fitted, cube


def test_geometry_changes(ctx, dev):
    """12 directions, 70 (wide basis, mask cache on), 100 (piercepoints only:
    the fit raises), 5: the pool reset by its D, the wide workspace and cache
    dropped, every geometry buffer bound again at its exact size."""
    steps = [("set_basis", 12), ("set_basis_wide", 70), ("set_piercepoints", 100),
             ("set_basis", 5)]
    one = ctx()
    for kind, D in steps:
        fitted, cube = geometry_step(one, dev, kind, D)
        want_fit, want_cube = geometry_step(ctx(), dev, kind, D)
        if fitted is not None:
            same(fitted, want_fit, f"{kind} D={D} fit")
        np.testing.assert_array_equal(cube.view(np.uint32), want_cube.view(np.uint32),
                                      err_msg=f"{kind} D={D} cube")
    masks, entries = one.fit_pool()
    assert len(masks) > 0 and entries.shape == (len(masks), 5 * 5 + 5)


# ------------------------------------------- 3. pool growth, contents kept

def usable_masks(weight, ref):
    """Distinct flag masks of the fitted slots with a flagged direction and
    two or more unflagged ones."""
    D = weight.shape[-1]
    w = np.delete(weight, ref, axis=2).reshape(-1, D) > 0
    n = w.sum(1)
    return np.unique((w[(n >= 2) & (n < D)] * (1 << np.arange(D))).sum(1))


@functools.lru_cache(maxsize=None)
def pool_case(D, T):
    """Random flags (40 %) over the 2 T fitted slots of (T, 1, 3), outliers
    (10 %) for a second pass at 2 sigma to flag, and the oracle's fit.  Slots
    left with fewer than three unflagged directions get their flags lifted: the
    covariance of two directions has the eigenvalues +c and -c, a tie in the
    |lambda| order of the basis columns, so the oracle's order-1 fit of such a
    slot is one of two equally valid ones."""
    niter, nsigma = 2, 2.0
    s, pp, ref, st, mid = synth(D, T, 1, 3, seed=1, flag_frac=0.4, outlier_frac=0.1)
    w = s.weight.copy()
    w[(w > 0).sum(-1) < 3] = 1.0
    s = type(s)(**{**vars(s), "weight": w})
    r = okl.run_phase(s.val, s.weight, s.ant_pos, pp, ref, min(20, D - 1), niter=niter,
                      nsigma=nsigma)
    assert ((r["w_out"] > 0).sum(-1) >= 3).all()
    return (s, pp, ref, st, mid), r, niter, nsigma


@pytest.mark.parametrize("D,T", [(11, 1000), (12, 1500)])
def test_pool_growth_keeps_contents(ctx, dev, D, T):
    """The pool starts at 1024 entries and doubles with its masks and bases
    kept.  D directions have 2^D - D - 2 usable masks (a flagged direction,
    two or more unflagged): 246 at D = 8 and 1012 at D = 10 can never pass
    1024, so D = 11 (2035) is the smallest case.  At D = 12 the input stays
    below 2048 masks and those of the second pass take the count past it:
    that doubling copies bases which slots with an unchanged mask still read.
    niter = 2, so every mask fitted is the input's or the oracle's final one,
    and the oracle counts them."""
    sol, r, niter, nsigma = pool_case(D, T)
    first = usable_masks(sol[0].weight, sol[2])
    both = np.union1d(first, usable_masks(r["w_out"], sol[2]))
    print(f"D={D}: {len(first)} masks in the input, {len(both)} with the second pass")
    assert 1024 < len(first) <= 2048
    assert D == 11 or len(both) > 2048
    c = ctx()
    c.set_basis(sol[1])
    got = fit(c, dev, sol, niter=niter, nsigma=nsigma)
    n_masks = c.fit_stats()["n_masks"]
    print(f"D={D}: n_masks {n_masks}")
    check(got, r["coef"], r["resid"], r["w_out"], r["orders"], f"pool growth D={D}")
    assert n_masks >= len(both) > 1024


# ------------------------------------------------ 4. tess and smooth scratch

TESS_D, TESS_S = 11, 5


@functools.lru_cache(maxsize=None)
def tess_inputs(n):
    rng = np.random.default_rng(100 + n)
    lab = rng.integers(1, TESS_D + 1, size=(n, n)).astype(np.int32)
    ph = rng.uniform(-9.0, 9.0, size=(TESS_S, TESS_D))
    ax = 10.0 ** rng.normal(0.0, 0.3, size=(TESS_S, TESS_D))
    ay = 10.0 ** rng.normal(0.0, 0.3, size=(TESS_S, TESS_D))
    cube = rng.normal(0.0, 1.0, size=(TESS_S, 4, n, n)).astype(np.float32)
    return lab, ph, ax, ay, cube


def tess(c, dev, n, sigma):
    lab, ph, ax, ay, _ = (torch.from_numpy(a).to(dev) for a in tess_inputs(n))
    out = torch.full((TESS_S, 4, n, n), -5.0, dtype=torch.float32, device=dev)
    c.tess_fill(lab, n, n, ph, TESS_D, TESS_S, out, amp_xx=ax, amp_yy=ay, smooth_pix=sigma)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not (got == -5.0).any()
    return got.view(np.uint32)


def smooth(c, dev, n, sigma):
    cube = torch.from_numpy(tess_inputs(n)[4]).to(dev)
    c.smooth(cube, n, n, TESS_S * 4, sigma)
    torch.cuda.synchronize()
    return cube.cpu().numpy().view(np.uint32)


def test_tess_and_smooth_scratch(ctx, dev):
    """8 x 8, 32 x 32, 8 x 8 again, unsmoothed (the value table alone) and at
    R = 25, the first radius past the fused kernel's (gather, then the pass
    buffer of sf_smooth); then sf_smooth alone at two sigmas (the weights on
    the device replaced, then found again)."""
    assert int(4 * 6.25 + 0.5) == 25  # kTessMaxR = 24
    calls = [(tess, n, sigma) for n in (8, 32, 8) for sigma in (0.0, 6.25)]
    calls += [(smooth, 32, 1.5), (smooth, 32, 3.0), (smooth, 8, 3.0), (smooth, 8, 1.5)]
    one = ctx()
    for run, n, sigma in calls:
        got = run(one, dev, n, sigma)
        want = run(ctx(), dev, n, sigma)
        assert np.array_equal(got, want), (run.__name__, n, sigma, int((got != want).sum()))


# ------------------------------------------------------- 5. context churn

def test_context_churn(dev):
    """Eight contexts created, used for one small fit and destroyed."""
    from ska_sdp_screen_fitting_amd._lib import Context
    sol = synth(5, 1, 1, 2)
    results = []
    for _ in range(8):
        c = Context(0)
        try:
            c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            c.set_basis(sol[1])
            results.append(fit(c, dev, sol))
        finally:
            c.close()
    assert np.isfinite(results[0][0]).all() and (results[0][0] != -7.0).all()
    for got in results[1:]:
        same(got, results[0], "churn")
