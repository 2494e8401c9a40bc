"""The fit kernels under an active order walk and off-default parameters.

``adjust_order`` moves a slot's order toward reduced chi^2 ~ 1 in the passes
after the first (OrderWalk::step, csrc/kl_fit_steps.h; stationscreen.py:
700-782): up to three re-fits per slot and pass, sign flips, the double-bound
stop.  With the weights of ``make_solutions`` it never moves; the inputs here
(tests/walk_cases.py: the reference's own runs of
tests/golden/make_golden_walk.py, and the oracle at D = 60 / 128) carry
weights near 1 / sigma^2, where it moves about half of the slots, small
``nsigma`` with many passes (cascade12: outlier flags of later passes take
slots down to 3, 2, 1 and 0 unflagged directions), ``adjust_order`` off,
``niter`` 1..8 and beta = 1.  tests/test_fit_walk_cpu.py shows on the oracle
that no slot of these inputs is ill-conditioned or marginal, so no slot is
excluded here.

Tolerances: those at the top of tests/test_gpu_parity.py -- orders and
``w_out`` identical, |d coef| <= 1e-8 x max(1, |coef|max), |d resid| <= 1e-8;
byte equality among the options the ABI documents as "same bits".
Needs an MI355X: every test is marked ``gpu``.
"""

import contextlib

import numpy as np
import pytest

import walk_cases as wc
from test_wide_fit import wide_fit

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SF_EINVAL = -22
RUNS = wc.all_runs()
NARROW = [r for r in RUNS if r.val.shape[-1] <= 60]
WIDE = [r for r in RUNS if r.val.shape[-1] > 60]
NARROW_PHASE = [r for r in NARROW if r.type == "phase"]


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


def opt(name):
    from ska_sdp_screen_fitting_amd import _lib
    return getattr(_lib, "SF_OPT_FIT_" + name)


# the defaults of the fit options (include/screenfit.h)
DEFAULTS = {"GENERAL": 0, "PACK": 1, "LEAN": 1, "EIG_WAVES": 0,
            "SUBSET_DELETION": 1, "WIDE_CACHE": 1, "WIDE_POOL_MAX": 0}


@contextlib.contextmanager
def options(ctx, **values):
    try:
        for k, v in values.items():
            ctx.set_option(opt(k), v)
        yield
    finally:
        for k in values:
            ctx.set_option(opt(k), DEFAULTS[k])


def fit(ctx, dev, r, outputs=True, **kw):
    """sf_set_basis[_wide] at the Run's r_0 / beta + sf_kl_fit with its
    parameters -> host (coef, resid, w_out, orders)."""
    prm = dict(niter=r.niter, nsigma=r.nsigma, adjust_order=r.adjust,
               r_0=r.r_0)
    prm.update(kw)
    r_0 = prm.pop("r_0")
    if r.val.shape[-1] > 60:
        ctx.set_basis_wide(r.pp, r_0, r.beta)
    else:
        ctx.set_basis(r.pp, r_0, r.beta)
    return wide_fit(ctx, dev, r.val, r.weight, r.pp, r.st, r.ref,
                    screen_type=wc.SCREEN_TYPES[r.type], bind=False,
                    outputs=outputs, **prm)


def check(got, want, what):
    """The module's tolerances; every figure printed before it is asserted."""
    coef, resid, w_out, orders = want
    cerr = np.abs(got[0] - coef).max()
    rerr = np.abs(got[1] - resid).max()
    scale = max(1.0, np.abs(coef).max())
    print(f"{what}: coef err {cerr:.3g} (allowed {1e-8 * scale:.3g}) resid err "
          f"{rerr:.3g} orders differ {(got[3] != orders).sum()} weights differ "
          f"{(got[2] != w_out).sum()}")
    np.testing.assert_array_equal(got[3], orders)
    np.testing.assert_array_equal(got[2], w_out)
    assert cerr <= 1e-8 * scale
    assert rerr <= 1e-8


def same_bytes(a, b, what):
    for x, y, name in zip(a, b, ("coef", "resid", "w_out", "orders")):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8),
                              np.ascontiguousarray(y).view(np.uint8)), (what, name)


# ------------------------------------------------- 1. the default pipeline

@pytest.mark.parametrize("r", RUNS, ids=wc.run_id)
def test_fit_vs_reference(ctx, dev, r):
    """Every case and parameter set on the default pipeline (the wide fit
    above 60 directions) against the reference's own run (the oracle's at
    D = 60 / 128)."""
    got = fit(ctx, dev, r)
    check(got, wc.expected(r), wc.run_id(r))
    st = ctx.fit_stats()
    if r.case == "walk20mixed":
        # weights of 5e-4: the slow class (general layout) ran
        assert st["n_general"] > 0
    elif r.val.shape[-1] <= 60:
        assert st["n_general"] == 0


# ------------------------------------- 2. the options that keep every bit

SAME_BITS = [dict(PACK=0), dict(LEAN=0), dict(EIG_WAVES=1), dict(EIG_WAVES=4),
             dict(SUBSET_DELETION=2), dict(SUBSET_DELETION=3)]


@pytest.mark.parametrize("r", NARROW, ids=wc.run_id)
def test_fit_options_keep_every_bit(ctx, dev, r):
    """One slot per wavefront, the general layout, 1 and 4 waves per subset
    Jacobi and the deletion modes 2 and 3 write the bytes the defaults write
    -- while the walk re-fits and while the cascade makes new masks in every
    pass."""
    base = fit(ctx, dev, r)
    check(base, wc.expected(r), wc.run_id(r))
    for o in SAME_BITS:
        with options(ctx, **o):
            same_bytes(fit(ctx, dev, r), base, (wc.run_id(r), o))


@pytest.mark.parametrize("r", NARROW, ids=wc.run_id)
def test_fit_jacobi_subset_bases(ctx, dev, r):
    """SF_OPT_FIT_SUBSET_DELETION = 0 (every subset basis by the Jacobi
    solve): the reference's result within the tolerances, the same bytes on
    1, 3 (default) and 4 waves per mask."""
    with options(ctx, SUBSET_DELETION=0):
        base = fit(ctx, dev, r)
        check(base, wc.expected(r), wc.run_id(r) + " jacobi")
        for nw in (1, 4):
            with options(ctx, EIG_WAVES=nw):
                same_bytes(fit(ctx, dev, r), base, (wc.run_id(r), nw))


@pytest.mark.parametrize("r", NARROW_PHASE, ids=wc.run_id)
def test_fit_general_kernel(ctx, dev, r):
    """SF_OPT_FIT_GENERAL = 1 (kl_fit.hip, the per-slot Jacobi): phase with
    any niter."""
    with options(ctx, GENERAL=1):
        got = fit(ctx, dev, r)
    check(got, wc.expected(r), wc.run_id(r) + " general")


@pytest.mark.parametrize("group", ["ref", "noref"])
def test_fit_general_kernel_tec_single_pass(ctx, dev, group):
    """... and tec with niter 1 only, as the ABI states: more passes are
    SF_EINVAL."""
    from ska_sdp_screen_fitting_amd._lib import ScreenFitError
    r = [x for x in wc.runs("walk14tec") if x.group == group][0]
    want = wc.run_oracle(r, niter=1)
    with options(ctx, GENERAL=1):
        got = fit(ctx, dev, r, niter=1)
        with pytest.raises(ScreenFitError, match=str(SF_EINVAL)):
            fit(ctx, dev, r, niter=2)
    check(got, want, f"tec {group} general niter 1")
    same_bytes(got[2:3], (r.weight,), "one pass flags nothing")


@pytest.mark.parametrize("r", WIDE, ids=wc.run_id)
def test_wide_fit_options_keep_every_bit(ctx, dev, r):
    """Above 60 directions: the mask cache off, on, and a pool of one entry
    (every other mask decomposed by its slots)."""
    base = fit(ctx, dev, r)
    check(base, wc.expected(r), wc.run_id(r))
    for o in (dict(WIDE_CACHE=0), dict(WIDE_CACHE=1), dict(WIDE_POOL_MAX=1)):
        with options(ctx, **o):
            same_bytes(fit(ctx, dev, r), base, (wc.run_id(r), o))


# ------------------------------------------------ 3. the parameters act

def walk20(niter, nsigma, adjust):
    return [r for r in wc.runs("walk20")
            if (r.niter, r.nsigma, r.adjust) == (niter, nsigma, adjust)][0]


def test_adjust_order_is_not_ignored(ctx, dev):
    r = walk20(4, 3.0, True)
    on = fit(ctx, dev, r)
    off = fit(ctx, dev, r, adjust_order=False)
    check(off, wc.expected(walk20(4, 3.0, False)), "walk20 adjust_order off")
    assert not np.array_equal(on[3], off[3])
    assert not np.array_equal(on[0], off[0])
    # a single pass never walks
    one = walk20(1, 5.0, False)
    same_bytes(fit(ctx, dev, one), fit(ctx, dev, one, adjust_order=True),
               "niter 1")


def test_huge_nsigma_flags_nothing(ctx, dev):
    r = walk20(4, 1e9, True)
    got = fit(ctx, dev, r)
    same_bytes(got[2:3], (r.weight,), "nsigma 1e9")
    assert wc.walked(r, got[2], got[3]).sum() * 4 >= wc.fitted(r).sum()


def test_r0_reaches_the_fit(ctx, dev):
    """r_0 = 250 (the reference fixes 100, so: the oracle), under the walk."""
    r = walk20(4, 3.0, True)
    want = wc.run_oracle(r, r_0=250.0)
    got = fit(ctx, dev, r, r_0=250.0)
    check(got, want, "walk20 r_0 250")
    assert not np.array_equal(got[0], fit(ctx, dev, r)[0])


# ------------------------------------------------------- 4. the cascade

@pytest.mark.parametrize("r", wc.runs("cascade12"), ids=wc.run_id)
def test_cascade_empty_slots_and_masks(ctx, dev, r):
    got = fit(ctx, dev, r)
    o_coef, _, o_w, o_orders = wc.oracle(r)
    n = (got[2] > 0).sum(axis=-1)
    empty = wc.fitted(r) & (n == 0)
    assert empty.sum() == 10
    # a slot that lost its last direction keeps the last fit it had
    np.testing.assert_array_equal(got[3][empty], o_orders[empty])
    assert np.abs(got[0][empty] - o_coef[empty]).max() <= 1e-8 * max(
        1.0, np.abs(o_coef).max())
    assert np.abs(got[0][empty]).max() > 0
    np.testing.assert_array_equal(got[2], o_w)
    # every partial mask the passes made was decomposed (or was a tie / a
    # single direction, which need no basis: still counted as a mask)
    bits = (got[2][wc.fitted(r)] > 0) @ (1 << np.arange(12))
    partial = {int(b) for b in bits if 0 < bin(int(b)).count("1") < 12}
    st = ctx.fit_stats()
    print("cascade12: distinct partial masks in w_out", len(partial),
          "n_masks", st["n_masks"])
    assert st["n_masks"] >= len(partial)


# ---------------------------------------------------------- 5. the ABI

@pytest.mark.parametrize("name", ["walk20", "walk80"])
def test_null_outputs_keep_the_coefficients(ctx, dev, name):
    r = [x for x in wc.runs(name) if x.niter == 4 and x.adjust
         and x.nsigma == 3.0][0]
    full = fit(ctx, dev, r)
    lone = fit(ctx, dev, r, outputs=False)
    assert np.array_equal(lone.view(np.uint8), full[0].view(np.uint8))


def test_sharded_walk_equals_unsharded(ctx, dev):
    """Station shards with the reference phases passed in (ant_offset +
    ref_phase), under the walk."""
    r = walk20(4, 3.0, True)
    full = fit(ctx, dev, r)
    refph = torch.from_numpy(np.ascontiguousarray(r.val[:, :, r.ref, :])).to(dev)
    ctx.set_basis(r.pp, r.r_0, r.beta)
    for a0, a1 in ((0, 2), (2, 4), (4, 5)):
        part = wide_fit(ctx, dev, r.val[:, :, a0:a1], r.weight[:, :, a0:a1],
                        r.pp, r.st[a0:a1], r.ref, niter=r.niter, bind=False,
                        nsigma=r.nsigma, adjust_order=r.adjust, ant_offset=a0,
                        ref_phase=refph)
        same_bytes(part, [x[:, :, a0:a1] for x in full], (a0, a1))


def test_niter_range(ctx, dev):
    """niter outside 1..64 is SF_EINVAL; 64 passes run."""
    from ska_sdp_screen_fitting_amd._lib import ScreenFitError
    r = walk20(4, 3.0, True)
    ctx.set_basis(r.pp, r.r_0, r.beta)
    val, wt = r.val[:1, :1, :2], r.weight[:1, :1, :2]
    for bad in (0, 65):
        with pytest.raises(ScreenFitError, match=rf"\({SF_EINVAL}\).*niter"):
            wide_fit(ctx, dev, val, wt, r.pp, [12, 12], -1, niter=bad,
                     bind=False)
    got = wide_fit(ctx, dev, val, wt, r.pp, [12, 12], -1, niter=64, bind=False,
                   nsigma=3.0)
    want = wc.okl.run_phase(val, wt, r.ant_pos[:2], r.pp, -1, 12, niter=64,
                            nsigma=3.0, scale_order=False)
    check(got, (want["coef"], want["resid"], want["w_out"], want["orders"]),
          "niter 64")


# --------------------------------------------------- 6. the host's run()

@pytest.mark.parametrize("name,prm", [
    ("walk20", dict(niter=4, nsigma=3.0, adjust_order=False)),
    ("walk20beta", dict(niter=3, nsigma=3.0, adjust_order=True, beta=1.0))])
def test_stationscreen_run_passes_the_parameters(dev, name, prm):
    """The package's stationscreen.run on a soltab of the case: niter,
    nsigma, adjust_order and beta reach the device."""
    from ska_sdp_screen_fitting_amd import stationscreen
    from ska_sdp_screen_fitting_amd.h5parm import Solset, Soltab
    r = [x for x in wc.runs(name) if (x.niter, x.nsigma, x.adjust) ==
         (prm["niter"], prm["nsigma"], prm["adjust_order"])][0]
    g = wc.load_golden(name)
    T, F, A, D = r.val.shape
    ants = [f"ST{a:04d}" for a in range(A)]
    dirs = [f"[Patch_{k}]" for k in range(D)]
    ss = Solset("sol000", ants, g["ant_pos"], dirs, g["dir_radec"])
    st = Soltab("phase000", "phase", ["time", "freq", "ant", "dir"],
                [np.arange(T) * 8.0, 1.2e8 + np.arange(F) * 4e6, np.array(ants),
                 np.array(dirs)], r.val, r.weight, solset=ss)
    assert stationscreen.run(st, "phase_screen000", order=r.order, ref_ant=r.ref,
                             **prm) == 0
    scr = ss.get_soltab("phase_screen000")
    res = ss.get_soltab("phase_screen000resid")
    assert scr.attrs["beta"] == r.beta
    check((scr.val, res.val, scr.weight, res.weight[..., 0].astype(np.int32)),
          wc.expected(r), name + " stationscreen.run")
