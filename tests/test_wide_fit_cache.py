"""The mask cache of the wide fit (61..128 directions, csrc/kl_fit_wide.hip):
every distinct flag mask of a call's input is decomposed once into a pool of
subset bases keyed by the 128-bit mask (SF_OPT_FIT_WIDE_CACHE, _POOL_MB,
_POOL_MAX, sf_get_fit_pool_wide).

The cache changes no output bit: every case compares the cache on with the
cache off as bytes.  The oracle checks use tests/test_wide_fit.py's criteria
(its ``check``); the pool contents use the tolerances of its
test_wide_basis_vs_oracle for the global basis: eigenvalues 1e-12 relative to
|lambda|max, vectors 1e-9 -- V^T V = I to 1e-9, and V diag(lambda) V^T = C_sub
to 2e-9 |lambda|max (vectors off by dV move the product by at most
2 |dV| |lambda|max).
Needs an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest

from oracle import kl as okl
from test_wide_fit import (AMPLITUDE, PHASE, TEC, check, phase_orders,
                           stack_pols, synth, wide_fit)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FULL = (1 << 64) - 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx(dev):
    from ska_sdp_screen_fitting_amd import _lib, get_context
    c = get_context(0)
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    yield c
    c.set_option(_lib.SF_OPT_FIT_WIDE_CACHE, 1)
    c.set_option(_lib.SF_OPT_FIT_WIDE_POOL_MB, 0)
    c.set_option(_lib.SF_OPT_FIT_WIDE_POOL_MAX, 0)


def fit(ctx, dev, cache, *args, **kw):
    """wide_fit with the cache on / off -> (outputs, n_masks)."""
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_FIT_WIDE_CACHE
    ctx.set_option(SF_OPT_FIT_WIDE_CACHE, int(cache))
    try:
        got = wide_fit(ctx, dev, *args, **kw)
        return got, ctx.fit_stats()["n_masks"]
    finally:
        ctx.set_option(SF_OPT_FIT_WIDE_CACHE, 1)


def same_bytes(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def mask_words(unfl):
    """[..., D] bool -> (lo, hi) uint64 arrays: bit d of (lo, hi) = unfl[d]."""
    D = unfl.shape[-1]
    bits = np.zeros(unfl.shape[:-1] + (128,), np.uint64)
    bits[..., :D] = unfl
    sh = np.arange(64, dtype=np.uint64)
    lo = (bits[..., :64] << sh).sum(-1, dtype=np.uint64)
    hi = (bits[..., 64:] << sh).sum(-1, dtype=np.uint64)
    return lo, hi


def distinct_masks(weight, ref):
    """The distinct masks with 0 < n < D among the fitted slots (the synthetic
    sets have no skipped block: only the reference station is left out)."""
    D = weight.shape[-1]
    keep = np.ones(weight.shape[2], bool)
    if ref >= 0:
        keep[ref] = False
    unfl = weight[:, :, keep] > 0
    n = unfl.sum(-1)
    lo, hi = mask_words(unfl[(n > 0) & (n < D)])
    return {(int(a), int(b)) for a, b in zip(lo, hi)}


# ----------------------------------------------- 1. bit identity, on vs off

def masks_change(w_in, w_after):
    return bool((((w_in > 0) != (w_after > 0)).any(-1)).any())


@pytest.mark.parametrize("D", [61, 65, 128])
def test_cache_phase_bits(ctx, dev, D):
    s, pp = synth(D)
    ref = okl.reference_station(s.weight)
    st = phase_orders(s, ref)
    # the oracle's weights after pass 0: a mask changed, so pass 1 meets a
    # mask that was not the slot's own in pass 0
    r = okl.run_phase(s.val, s.weight, s.ant_pos, pp, ref, 20)
    assert masks_change(s.weight, r["w_out"])
    on, n_on = fit(ctx, dev, 1, s.val, s.weight, pp, st, ref)
    off, n_off = fit(ctx, dev, 0, s.val, s.weight, pp, st, ref)
    print(f"D={D}: decompositions on {n_on} off {n_off}")
    same_bytes(on, off)
    assert n_on <= n_off
    check(on, r["coef"], r["resid"], r["w_out"], r["orders"], f"cache D={D}")


def test_cache_tec_bits(ctx, dev):
    s, pp = synth(80, n_freq=2)
    ref = okl.reference_station(s.weight)
    st = phase_orders(s, ref)
    r = okl.run_soltab(s.val, s.weight, s.ant_pos, pp, ref, 20, "tec", niter=2)
    assert masks_change(s.weight, r["w_out"])
    on, n_on = fit(ctx, dev, 1, s.val, s.weight, pp, st, ref, screen_type=TEC,
                   niter=2)
    off, n_off = fit(ctx, dev, 0, s.val, s.weight, pp, st, ref, screen_type=TEC,
                     niter=2)
    same_bytes(on, off)
    assert n_on <= n_off


def test_cache_amplitude_bits(ctx, dev):
    from ska_sdp_screen_fitting_amd.synthetic import make_amplitudes
    s, pp = synth(80, n_freq=2)
    make_amplitudes(s, seed=2080, flag_frac=0.02, outlier_frac=0.005)
    amp, wt = s.amp_val, s.meta["amp_weight"]
    # two passes of the oracle: its w_out holds the flags of pass 0
    r = okl.run_amplitude(amp, wt, pp, 12, niter=2)
    assert masks_change(wt, r["w_out"])
    P, A = amp.shape[-1], amp.shape[2]
    args = (stack_pols(amp), stack_pols(wt), pp, [12] * (A * P), -1)
    on, n_on = fit(ctx, dev, 1, *args, screen_type=AMPLITUDE, niter=3)
    off, n_off = fit(ctx, dev, 0, *args, screen_type=AMPLITUDE, niter=3)
    same_bytes(on, off)
    assert n_on <= n_off


def test_cache_second_pass_refits(ctx, dev):
    """Weights of 400 at D = 80: the reduced chi^2 of pass 0 is above 1, so
    the order walk of pass 1 moves and refits (with weights of 1 the walk
    stays at the station's order and pass 1 fits nothing).  A refitted slot
    whose mask pass 0 changed into one no input slot carries is a lookup miss
    and decomposes in its own workgroup; a refitted slot with an input mask
    hits the pool.  The oracle tells which slots those are: the order moved
    between its niter = 1 and niter = 2 fits."""
    s, pp = synth(80, n_freq=2)
    w = (s.weight * np.float32(400.0)).astype(np.float32)
    ref = okl.reference_station(w)
    st = phase_orders(s, ref)
    r1 = okl.run_phase(s.val, w, s.ant_pos, pp, ref, 20, niter=1)
    r2 = okl.run_phase(s.val, w, s.ant_pos, pp, ref, 20, niter=2)
    moved = r1["orders"] != r2["orders"]
    inputs = distinct_masks(w, ref)
    unfl = r2["w_out"] > 0
    lo, hi = mask_words(unfl)
    n = unfl.sum(-1)
    misses = sum(1 for i in np.ndindex(moved.shape)
                 if moved[i] and 0 < n[i] < 80
                 and (int(lo[i]), int(hi[i])) not in inputs)
    assert misses > 0 and moved.sum() > 0
    on, n_on = fit(ctx, dev, 1, s.val, w, pp, st, ref)
    off, n_off = fit(ctx, dev, 0, s.val, w, pp, st, ref)
    print(f"second pass: distinct input masks {len(inputs)} slots refitted "
          f"{int(moved.sum())} of them with a new mask {misses}; "
          f"decompositions on {n_on} off {n_off}")
    same_bytes(on, off)
    check(on, r2["coef"], r2["resid"], r2["w_out"], r2["orders"], "weights 400")
    # every miss decomposes once (a slot whose walk moved and came back to its
    # first order is not counted here and may add one more)
    assert len(inputs) + misses <= n_on <= n_off


# ------------------------------------------------------- 2. 128-bit keys

CRAFTED_FLAGS = [(3,), (100,), (3, 100), (70, 100), (3, 70)]


def crafted_keys():
    keys = set()
    for fl in CRAFTED_FLAGS:
        lo, hi = FULL, FULL
        for d in fl:
            if d < 64:
                lo &= ~(1 << d)
            else:
                hi &= ~(1 << (d - 64))
        keys.add((lo, hi))
    return keys


@pytest.fixture(scope="module")
def crafted(ctx, dev):
    """D = 128; frequency f flags CRAFTED_FLAGS[f] at every time and station:
    equal lo with different hi, equal hi with different lo.  One oracle fit,
    the cache-off outputs and the cache-on outputs with their pool."""
    s, pp = synth(128, n_ant=3, n_freq=len(CRAFTED_FLAGS), flag_frac=0.0,
                  outlier_frac=0.0, seed=5128)
    w = s.weight.copy()
    assert (w == 1).all()
    for f, fl in enumerate(CRAFTED_FLAGS):
        w[:, f, :, list(fl)] = 0.0
    ref = okl.reference_station(w)
    st = phase_orders(s, ref)
    args = (s.val, w, pp, st, ref)
    off, n_off = fit(ctx, dev, 0, *args, niter=1)
    on, n_on = fit(ctx, dev, 1, *args, niter=1)
    masks, ent = ctx.fit_pool_wide()
    oracle = okl.run_phase(s.val, w, s.ant_pos, pp, ref, 20, niter=1)
    return dict(s=s, pp=pp, w=w, ref=ref, st=st, args=args, off=off, n_off=n_off,
                on=on, n_on=n_on, masks=masks, ent=ent, oracle=oracle)


def test_cache_128_bit_keys(crafted):
    c = crafted
    assert c["n_on"] == 5
    fitted = (c["w"].shape[2] - 1) * c["w"].shape[0] * c["w"].shape[1]
    assert c["n_off"] == fitted  # every flagged slot decomposed its own
    got = {(int(a), int(b)) for a, b in c["masks"]}
    assert len(c["masks"]) == 5 and got == crafted_keys()
    # sorted by (hi, lo)
    assert [(int(b), int(a)) for a, b in c["masks"]] == sorted(
        (hi, lo) for lo, hi in crafted_keys())
    r = c["oracle"]
    check(c["on"], r["coef"], r["resid"], r["w_out"], r["orders"], "crafted D=128")
    same_bytes(c["on"], c["off"])


# ------------------------------------------------------ 3. pool contents

def check_pool(masks, ent, pp, what):
    D = pp.shape[0]
    c0 = okl.calculate_svd(pp, 100.0, 5.0 / 3.0)[0]
    assert len(masks) > 0
    worst = np.zeros(3)
    for (lo, hi), e in zip(masks, ent):
        m = int(lo) | (int(hi) << 64)
        idx = np.array([d for d in range(D) if (m >> d) & 1])
        n = len(idx)
        assert 0 < n < D
        v = e[:D * D].reshape(D, D)[:n, :n]
        lam = e[D * D:D * D + n]
        # nothing outside the leading block
        assert not e[:D * D].reshape(D, D)[n:].any()
        assert not e[:D * D].reshape(D, D)[:, n:].any()
        assert not e[D * D + n:].any()
        csub = c0[np.ix_(idx, idx)]
        want = np.linalg.eigvalsh(csub)
        want = want[np.argsort(-np.abs(want), kind="stable")]
        lmax = np.abs(want).max()
        assert (np.diff(np.abs(lam)) <= 0).all()
        errs = np.array([np.abs(lam - want).max() / lmax,
                         np.abs((v * lam) @ v.T - csub).max() / lmax,
                         np.abs(v.T @ v - np.eye(n)).max()])
        worst = np.maximum(worst, errs)
        assert errs[0] <= 1e-12
        assert errs[1] <= 2e-9
        assert errs[2] <= 1e-9
    print(f"{what}: {len(masks)} entries, worst |dlam|/lmax {worst[0]:.3g} "
          f"|V lam V^T - C_sub|/lmax {worst[1]:.3g} |V^T V - I| {worst[2]:.3g}")


def test_cache_pool_contents_crafted(crafted):
    check_pool(crafted["masks"], crafted["ent"], crafted["pp"], "crafted D=128")


def test_cache_pool_contents_random(ctx, dev):
    s, pp = synth(65)
    ref = okl.reference_station(s.weight)
    _, n_on = fit(ctx, dev, 1, s.val, s.weight, pp, phase_orders(s, ref), ref,
                  niter=1)
    masks, ent = ctx.fit_pool_wide()
    want = distinct_masks(s.weight, ref)
    assert {(int(a), int(b)) for a, b in masks} == want and n_on == len(want)
    check_pool(masks, ent, pp, "random D=65")


# ------------------------------------------------- 4. decomposition count

def test_cache_decomposition_count(ctx, dev):
    s, pp = synth(80, n_ant=4, n_freq=2)
    w = s.weight.copy()
    w[1] = w[0]  # masks that repeat: fewer distinct masks than flagged slots
    ref = okl.reference_station(w)
    st = phase_orders(s, ref)
    want = len(distinct_masks(w, ref))
    keep = np.arange(w.shape[2]) != ref
    flagged = int((((w[:, :, keep] > 0).sum(-1) < 80)
                   & ((w[:, :, keep] > 0).sum(-1) > 0)).sum())
    assert 0 < want < flagged
    on1, n1 = fit(ctx, dev, 1, s.val, w, pp, st, ref, niter=1)
    off1, m1 = fit(ctx, dev, 0, s.val, w, pp, st, ref, niter=1)
    print(f"niter 1: distinct {want} flagged slots {flagged} on {n1} off {m1}")
    assert n1 == want and m1 == flagged
    same_bytes(on1, off1)
    on2, n2 = fit(ctx, dev, 1, s.val, w, pp, st, ref, niter=2)
    off2, m2 = fit(ctx, dev, 0, s.val, w, pp, st, ref, niter=2)
    print(f"niter 2: on {n2} off {m2}")
    assert want <= n2 <= m2
    same_bytes(on2, off2)


# --------------------------------------------- 5. more masks than workgroups

def test_cache_more_masks_than_workgroups(ctx, dev):
    """640 slots at D = 61, each flagging its own pair of directions: more
    pool entries than an MI355X has compute units, so the subset kernel's
    persistent grid strides."""
    s, pp = synth(61, n_ant=4, n_time=16, n_freq=10, flag_frac=0.0,
                  outlier_frac=0.0, seed=5061)
    w = s.weight.copy()
    pairs = [(i, j) for i in range(61) for j in range(i + 1, 61)][::2][:640]
    assert len(pairs) == 640
    w.reshape(640, 61)[np.arange(640)[:, None], np.array(pairs)] = 0.0
    assert ((w > 0).sum(-1) == 59).all()
    args = (s.val, w, pp, [10] * 4, -1)  # no reference station: 640 fitted slots
    on, n_on = fit(ctx, dev, 1, *args, niter=1)
    assert len(ctx.fit_pool_wide()[0]) == 640
    off, n_off = fit(ctx, dev, 0, *args, niter=1)
    assert n_on == 640 and n_off == 640
    same_bytes(on, off)


# -------------------------------------------------------------- 6. overflow

def test_cache_pool_overflow(ctx, dev, crafted):
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_FIT_WIDE_POOL_MAX
    ctx.set_option(SF_OPT_FIT_WIDE_POOL_MAX, 2)
    try:
        on, n_on = fit(ctx, dev, 1, *crafted["args"], niter=1)
        masks, ent = ctx.fit_pool_wide()
    finally:
        ctx.set_option(SF_OPT_FIT_WIDE_POOL_MAX, 0)
    same_bytes(on, crafted["off"])
    assert len(masks) == 2
    assert {(int(a), int(b)) for a, b in masks} < crafted_keys()
    check_pool(masks, ent, crafted["pp"], "overflow D=128")
    print(f"overflow: {n_on} decompositions (cache off {crafted['n_off']})")
    assert 5 <= n_on <= crafted["n_off"]


def test_cache_pool_byte_cap(ctx, dev, crafted):
    """1 MiB holds 7 entries at D = 128 (134,144 bytes each): all five masks;
    the option is honoured and reset."""
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_FIT_WIDE_POOL_MB
    ctx.set_option(SF_OPT_FIT_WIDE_POOL_MB, 1)
    try:
        on, n_on = fit(ctx, dev, 1, *crafted["args"], niter=1)
        assert len(ctx.fit_pool_wide()[0]) == 5 and n_on == 5
    finally:
        ctx.set_option(SF_OPT_FIT_WIDE_POOL_MB, 0)
    same_bytes(on, crafted["off"])


# ------------------------------------------------------------------ 7. ABI

def test_cache_abi(ctx, dev, crafted):
    from ska_sdp_screen_fitting_amd import _lib
    from ska_sdp_screen_fitting_amd._lib import ScreenFitError
    for opt, bad in ((_lib.SF_OPT_FIT_WIDE_CACHE, (-1, 2)),
                     (_lib.SF_OPT_FIT_WIDE_POOL_MB, (-1, 65537)),
                     (_lib.SF_OPT_FIT_WIDE_POOL_MAX, (-1,))):
        for v in bad:
            with pytest.raises(ScreenFitError):
                ctx.set_option(opt, v)
    ctx.set_option(_lib.SF_OPT_FIT_WIDE_POOL_MB, 65536)
    ctx.set_option(_lib.SF_OPT_FIT_WIDE_POOL_MB, 0)

    # a D = 60 fit before and after a wide fit: the same bytes (the wide pool
    # leaves the <= 60 path's pool alone), and no wide pool on that context
    s60, pp60 = synth(60)
    ref60 = okl.reference_station(s60.weight)
    st60 = phase_orders(s60, ref60)

    def fit60():
        ctx.set_basis(pp60)
        got = wide_fit(ctx, dev, s60.val, s60.weight, pp60, st60, ref60, bind=False)
        with pytest.raises(ScreenFitError):
            ctx.fit_pool_wide()
        return got, ctx.fit_pool()

    before, pool_before = fit60()
    # the wide fit: a second identical call gives identical bytes
    again, n_again = fit(ctx, dev, 1, *crafted["args"], niter=1)
    same_bytes(again, crafted["on"])
    assert n_again == 5 and len(ctx.fit_pool_wide()[0]) == 5
    # the cache off leaves no pool; the fast path's hook keeps refusing
    fit(ctx, dev, 0, *crafted["args"], niter=1)
    assert len(ctx.fit_pool_wide()[0]) == 0
    with pytest.raises(ScreenFitError):
        ctx.fit_pool()
    after, pool_after = fit60()
    same_bytes(before, after)
    assert np.array_equal(pool_before[0], pool_after[0])
    assert np.array_equal(pool_before[1].view(np.uint64), pool_after[1].view(np.uint64))

    # evaluation-only geometry: no wide basis, no pool
    ctx.set_piercepoints(crafted["pp"])
    with pytest.raises(ScreenFitError):
        ctx.fit_pool_wide()
