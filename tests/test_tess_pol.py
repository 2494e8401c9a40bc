"""sf_tess_fill_pol (csrc/tess.hip): the tessellated fill with polarized
phases -- planes 2 / 3 take cos / sin of a second phase array -- through every
smoothing path, against the oracle (oracle/voronoi.py: planes 0 / 1 of a call
with the XX phases, planes 2 / 3 of a call with the YY phases) at the
tolerances of tests/test_wide_tess.py: unsmoothed <= 1 ulp, smoothed
atol 1e-6.  Needs an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest

from oracle import voronoi as ov
from test_wide_tess import BE, SCRUB, raster, scrub, ulps, values

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# gather; interior lookups / wide tile at R = 2 and 5; run-time radius R = 12
# with four planes; gather + sf_smooth (R = 28 > 24)
SIGMAS = (0.0, 0.5, 1.25, 3.0, 7.0)


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


def fill(ctx, dev, lab, ph, ph_yy=None, ax=None, ay=None, sigma=0.0, flags=SCRUB,
         opts=(), entry="pol", check_labels=True):
    """entry "pol": Context.tess_fill (sf_tess_fill_pol); "plain": the C entry
    sf_tess_fill itself (no phase_yy)."""
    from ska_sdp_screen_fitting_amd import _lib
    ny, nx = lab.shape
    S, D = ph.shape
    t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
         for a in (lab, ph, ph_yy, ax, ay)]
    out = torch.full((S, 4, ny, nx), -5.0, dtype=torch.float32, device=dev)
    for o, v in opts:
        ctx.set_option(o, v)
    try:
        if entry == "plain":
            assert ph_yy is None
            rc = ctx.lib.sf_tess_fill(
                ctx.h, t[0].data_ptr(), nx, ny, t[1].data_ptr(),
                None if t[3] is None else t[3].data_ptr(),
                None if t[4] is None else t[4].data_ptr(), D, S, out.data_ptr(), S,
                float(sigma), flags)
            assert rc == 0, ctx.lib.sf_last_error()
        else:
            # a raw pointer skips the wrapper's label range check
            ctx.tess_fill(t[0] if check_labels else t[0].data_ptr(), nx, ny, t[1], D, S,
                          out, amp_xx=t[3], amp_yy=t[4], smooth_pix=sigma, flags=flags,
                          phase_yy=t[2])
        torch.cuda.synchronize()
    finally:
        defaults = {_lib.SF_OPT_TESS_BOX: -1}
        for o, _ in opts:
            ctx.set_option(o, defaults.get(o, 0))
    got = out.cpu().numpy()
    return got.byteswap() if flags & BE else got


def want_planes(lab, ph, ph_yy, ax=None, ay=None, sigma=0.0):
    wx = ov.gather_planes(lab, ph, ax, ay)
    wy = ov.gather_planes(lab, ph_yy, ax, ay)
    w = np.concatenate([wx[:, 0:2], wy[:, 2:4]], axis=1)
    return ov.smooth(w, sigma) if sigma > 0 else w


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# 7: the fixture; 64 | 65: both sides of the 65-entry table cap; 128: the maximum
@pytest.mark.parametrize("nx,ny", [(17, 17), (33, 17)])
@pytest.mark.parametrize("D", [7, 64, 65, 128])
def test_tess_pol_vs_oracle(ctx, dev, D, nx, ny):
    rng = np.random.default_rng(D * 100 + nx)
    lab = raster(rng, nx, ny, D)
    S = 37  # more than one slot chunk of every kernel (8, 16, 32)
    ph, ax, ay = values(rng, S, D)
    ph_yy = rng.uniform(-20.0, 20.0, size=(S, D))
    for amps in ((None, None), (ax, ay)):
        for sigma in SIGMAS:
            want = want_planes(lab, ph, ph_yy, *amps, sigma=sigma)
            got = fill(ctx, dev, lab, ph, ph_yy, *amps, sigma=sigma)
            if sigma == 0:
                err = ulps(got, want).max()
                assert err <= 1
                # the two plane pairs really differ
                assert np.abs(got[:, 0:2] - got[:, 2:4]).max() > 0.5
            else:
                err = np.abs(got - want).max()
                assert err <= 1e-6
            print(f"D={D} {nx}x{ny} sigma={sigma} amps={amps[0] is not None} err={err:.3g}")


@pytest.mark.parametrize("D", [7, 65])
def test_tess_pol_equals_tess_fill(ctx, dev, D):
    """phase_yy = None IS sf_tess_fill, and phase_yy equal to phase (four-plane
    kernels where sf_tess_fill runs the two-plane ones) writes its bits."""
    nx, ny, S = 33, 17, 21
    rng = np.random.default_rng(D)
    lab = raster(rng, nx, ny, D)
    ph, ax, ay = values(rng, S, D, nan=True)
    for amps in ((None, None), (ax, None), (ax, ay)):
        for sigma in SIGMAS:
            for flags in (SCRUB, BE):
                ref = fill(ctx, dev, lab, ph, None, *amps, sigma=sigma, flags=flags,
                           entry="plain")
                none = fill(ctx, dev, lab, ph, None, *amps, sigma=sigma, flags=flags)
                same = fill(ctx, dev, lab, ph, ph, *amps, sigma=sigma, flags=flags)
                assert np.array_equal(bits(none), bits(ref)), (sigma, flags)
                assert np.array_equal(bits(same), bits(ref)), (sigma, flags)


@pytest.mark.parametrize("D", [64, 128])
def test_tess_pol_kernels_agree(ctx, dev, D):
    """SF_OPT_TESS_TILE = 1 (the fused 16 x 16 tile kernel, which builds its own
    table) and SF_OPT_TESS_BOX = 0 / 1 write the bits of the default."""
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_TESS_BOX, SF_OPT_TESS_TILE
    nx, ny, S = 53, 37, 45
    rng = np.random.default_rng(D + 1)
    lab = raster(rng, nx, ny, D)
    ph, ax, ay = values(rng, S, D, nan=True)
    ph_yy = rng.uniform(-20.0, 20.0, size=(S, D))
    ph_yy[3, 1] = np.nan
    for amps in ((None, None), (ax, ay)):
        for sigma in (0.0, 0.5, 1.25, 3.0):
            for flags in (SCRUB, BE):
                ref = fill(ctx, dev, lab, ph, ph_yy, *amps, sigma=sigma, flags=flags)
                variants = [((SF_OPT_TESS_TILE, 1),)]
                if sigma > 0:
                    variants += [((SF_OPT_TESS_BOX, 0),), ((SF_OPT_TESS_BOX, 1),)]
                for opts in variants:
                    got = fill(ctx, dev, lab, ph, ph_yy, *amps, sigma=sigma, flags=flags,
                               opts=opts)
                    assert np.array_equal(bits(got), bits(ref)), (sigma, flags, opts)
    # and NaN phases stay in their plane pair
    want = want_planes(lab, ph, ph_yy, ax, ay)
    got = fill(ctx, dev, lab, ph, ph_yy, ax, ay, flags=0)
    nan = np.isnan(want)
    assert nan[:, 0:2].any() and nan[:, 2:4].any()
    assert not np.array_equal(nan[:, 0:2], nan[:, 2:4])
    assert np.array_equal(np.isnan(got), nan)
    assert ulps(got, want)[~nan].max() <= 1


@pytest.mark.parametrize("D", [7, 65])
def test_tess_pol_label_out_of_range(ctx, dev, D):
    """A label outside 1..D reads no table entry: NaN in all four planes,
    1 / 0 under the scrub."""
    nx, ny, S = 33, 17, 5
    rng = np.random.default_rng(D + 2)
    lab = raster(rng, nx, ny, D)
    ph, ax, ay = values(rng, S, D)
    ph_yy = rng.uniform(-20.0, 20.0, size=(S, D))
    want = want_planes(lab, ph, ph_yy, ax, ay)
    lab = lab.copy()
    bad = [(0, 0), (5, 7), (16, 32)]
    for (y, x), v in zip(bad, (0, D + 1, -3)):
        lab[y, x] = v
        want[:, :, y, x] = np.nan
    for sigma in (0.0, 0.5):
        w = ov.smooth(want, sigma) if sigma > 0 else want
        nan = np.isnan(w)
        raw = fill(ctx, dev, lab, ph, ph_yy, ax, ay, sigma=sigma, flags=0,
                   check_labels=False)
        assert np.array_equal(np.isnan(raw), nan)
        for y, x in bad:
            assert np.isnan(raw[:, :, y, x]).all()
        scr = fill(ctx, dev, lab, ph, ph_yy, ax, ay, sigma=sigma, flags=SCRUB,
                   check_labels=False)
        exp = scrub(w)
        for y, x in bad:
            assert np.all(scr[:, 0::2, y, x] == 1.0) and np.all(scr[:, 1::2, y, x] == 0.0)
        if sigma == 0:
            assert ulps(scr, exp).max() <= 1
        else:
            np.testing.assert_allclose(scr, exp, rtol=0, atol=1e-6)
