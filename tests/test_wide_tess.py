"""Tessellated (Voronoi) fill with 65..128 directions (SF_MAX_EVAL_DIR): the
table + gather kernels, the fused smoothing kernels with the 129-entry LDS
tables, gather + sf_smooth, and make_aterm_image end to end
(voronoi_screen.py:132-216, screen.py:353-378) -- against the oracle
(oracle/voronoi.py) at the tolerances of tests/test_tessellated.py.
Needs an MI355X: every test is marked ``gpu``.
"""

import os

import numpy as np
import pytest

from conftest import FIELD
from oracle import voronoi as ov

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SCRUB = 1       # SF_EVAL_NAN_SCRUB
BE = 1 << 10    # SF_EVAL_BIG_ENDIAN


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


def raster(rng, nx, ny, D):
    """Noise labels (most pixels are cell boundaries) next to a constant
    region (interior pixels); every label 1..D occurs."""
    lab = rng.integers(1, D + 1, size=(ny, nx)).astype(np.int32)
    lab[: ny // 2, : nx // 2] = D
    flat = lab.reshape(-1)
    flat[-D:] = np.arange(1, D + 1)
    assert set(np.unique(lab)) == set(range(1, D + 1))
    return lab


def values(rng, S, D, nan=False):
    ph = rng.uniform(-20.0, 20.0, size=(S, D))
    ax = 10.0 ** rng.normal(0.0, 0.3, size=(S, D))
    ay = 10.0 ** rng.normal(0.0, 0.3, size=(S, D))
    if nan:
        ph[S // 2, D - 1] = np.nan
        ax[S - 1, 70 % D] = np.nan
    return ph, ax, ay


def scrub(planes):
    out = planes.copy()
    for p in range(4):
        v = out[..., p, :, :]
        v[np.isnan(v)] = 0.0 if p % 2 else 1.0
    return out


def fill(ctx, dev, lab, ph, ax=None, ay=None, sigma=0.0, flags=SCRUB, opts=()):
    ny, nx = lab.shape
    S, D = ph.shape
    t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
         for a in (lab, ph, ax, ay)]
    out = torch.full((S, 4, ny, nx), -5.0, dtype=torch.float32, device=dev)
    for o, v in opts:
        ctx.set_option(o, v)
    try:
        ctx.tess_fill(t[0], nx, ny, t[1], D, S, out, amp_xx=t[2], amp_yy=t[3],
                      smooth_pix=sigma, flags=flags)
        torch.cuda.synchronize()
    finally:
        from ska_sdp_screen_fitting_amd import _lib
        defaults = {_lib.SF_OPT_TESS_BOX: -1}
        for o, _ in opts:
            ctx.set_option(o, defaults.get(o, 0))
    got = out.cpu().numpy()
    return got.byteswap() if flags & BE else got


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32))


@pytest.mark.parametrize("nx,ny", [(33, 17), (64, 64)])
@pytest.mark.parametrize("D", [65, 100, 128])
def test_wide_tess_unsmoothed(ctx, dev, D, nx, ny):
    """fp64 cos / sin (x amplitude) cast once to fp32: <= 1 ulp from numpy."""
    rng = np.random.default_rng(D * 100 + nx)
    lab = raster(rng, nx, ny, D)
    for S in (1, 45):
        ph, ax, ay = values(rng, S, D)
        got = fill(ctx, dev, lab, ph)
        assert ulps(got, ov.gather_planes(lab, ph)).max() <= 1
        got = fill(ctx, dev, lab, ph, ax, ay)
        assert ulps(got, ov.gather_planes(lab, ph, ax, ay)).max() <= 1
    # NaN phases / amplitudes with and without the scrub, FITS byte order
    ph, ax, ay = values(rng, 45, D, nan=True)
    want = ov.gather_planes(lab, ph, ax, ay)
    assert np.isnan(want).any()
    for flags in (SCRUB, SCRUB | BE, 0, BE):
        got = fill(ctx, dev, lab, ph, ax, ay, flags=flags)
        exp = scrub(want) if flags & SCRUB else want
        nan = np.isnan(exp)
        assert np.array_equal(np.isnan(got), nan)
        assert ulps(got, exp)[~nan].max() <= 1


@pytest.mark.parametrize("nx,ny", [(33, 17), (64, 64)])
def test_wide_tess_smoothed(ctx, dev, nx, ny):
    """Fused kernels (interior lookups and wide tile) at 0.5 / 2 px, gather +
    sf_smooth at 10 px, vs scipy's gaussian_filter of the oracle's gather."""
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_TESS_BOX
    D, S = 100, 21
    rng = np.random.default_rng(nx)
    lab = raster(rng, nx, ny, D)
    ph, ax, ay = values(rng, S, D)
    plain = ov.gather_planes(lab, ph)
    gain = ov.gather_planes(lab, ph, ax, ay)
    for sigma in (0.5, 2.0):
        w2, w4 = ov.smooth(plain, sigma), ov.smooth(gain, sigma)
        for box in (0, 1):
            opts = ((SF_OPT_TESS_BOX, box),)
            got = fill(ctx, dev, lab, ph, sigma=sigma, opts=opts)
            np.testing.assert_allclose(got, w2, rtol=0, atol=1e-6)
            got = fill(ctx, dev, lab, ph, ax, ay, sigma=sigma, opts=opts)
            np.testing.assert_allclose(got, w4, rtol=0, atol=1e-6)
    got = fill(ctx, dev, lab, ph, ax, ay, sigma=10.0)
    np.testing.assert_allclose(got, ov.smooth(gain, 10.0), rtol=0, atol=1e-6)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("sigma", [0.0, 0.5])
def test_wide_tess_kernels_agree(ctx, dev, D, sigma):
    """Every kernel choice writes the same bits (the fused 16 x 16 tile kernel,
    interior lookups, wide tile; slot chunks and waves of the gather), at
    SF_MAX_EVAL_DIR and -- unchanged -- at D = 64, where they also match the
    oracle."""
    from ska_sdp_screen_fitting_amd._lib import (SF_OPT_TESS_BOX, SF_OPT_TESS_SLOTS,
                                                 SF_OPT_TESS_TILE, SF_OPT_TESS_WAVES)
    nx, ny, S = 53, 37, 45
    rng = np.random.default_rng(D + int(sigma * 10))
    lab = raster(rng, nx, ny, D)
    ph, ax, ay = values(rng, S, D, nan=True)
    for yy in (None, ay):
        for flags in (SCRUB, BE):
            ref = fill(ctx, dev, lab, ph, ax, yy, sigma=sigma, flags=flags)
            variants = [((SF_OPT_TESS_TILE, 1),)]
            if sigma > 0:
                variants += [((SF_OPT_TESS_BOX, 0),), ((SF_OPT_TESS_BOX, 1),)]
            else:
                # 64 slots x 129 entries x 16 B > 64 KiB: the LDS chunk clamp
                variants += [((SF_OPT_TESS_SLOTS, k), (SF_OPT_TESS_WAVES, w))
                             for k, w in ((3, 8), (16, 16), (64, 4), (256, 16))]
            for opts in variants:
                got = fill(ctx, dev, lab, ph, ax, yy, sigma=sigma, flags=flags,
                           opts=opts)
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), opts
    want = ov.gather_planes(lab, ph, ax, ay)
    got = fill(ctx, dev, lab, ph, ax, ay, sigma=sigma, flags=0)
    if sigma > 0:
        want = ov.smooth(want, sigma)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.abs(got - want)[~nan].max() <= 1e-6
    else:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert ulps(got, want)[~nan].max() <= 1


def test_wide_tess_limit(ctx, dev):
    from ska_sdp_screen_fitting_amd._lib import SF_MAX_EVAL_DIR, ScreenFitError
    D = SF_MAX_EVAL_DIR + 1
    lab = np.ones((8, 8), np.int32)
    with pytest.raises(ScreenFitError):
        fill(ctx, dev, lab, np.zeros((2, D)))


def test_make_aterm_image_80_directions_tessellated(tmp_path, dev):
    """make_aterm_image(screen_type="tessellated") on a synthetic H5parm with
    80 directions, vs the oracle's gather and 0.5 px smoothing."""
    from ska_sdp_screen_fitting_amd import fits as sffits
    from ska_sdp_screen_fitting_amd.h5parm import (Solset, Soltab,
                                                   get_reference_station,
                                                   write_h5parm)
    from ska_sdp_screen_fitting_amd.make_aterm_images import make_aterm_image
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    from ska_sdp_screen_fitting_amd.voronoi_screen import (read_patch_positions,
                                                           tessellation_template)
    s = make_solutions(n_ant=3, n_time=4, n_freq=2, n_dir=80, seed=81)
    ss = Solset("sol000", s.ant_names, s.ant_pos, s.dir_names, s.dir_radec)
    axes = ["time", "freq", "ant", "dir"]
    st = Soltab("phase000", "phase", axes,
                [s.times, s.freqs, np.array(s.ant_names), np.array(s.dir_names)],
                s.val, s.weight, solset=ss)
    ss.soltabs["phase000"] = st
    h5 = str(tmp_path / "wide.h5")
    write_h5parm(h5, [ss])

    def sexa(v, sep):
        d = int(v)
        m = int((v - d) * 60)
        sec = ((v - d) * 60 - m) * 60
        return f"{d}{sep}{m:02d}{sep}{sec:09.6f}"

    sky = str(tmp_path / "sky.txt")
    with open(sky, "w", encoding="utf8") as fh:
        fh.write("FORMAT = Name, Type, Patch, Ra, Dec, I\n\n")
        for name, (ra, dec) in zip(s.dir_names, np.rad2deg(s.dir_radec.astype(np.float64))):
            fh.write(f" , , {name.strip('[]')}, {sexa(ra / 15.0, ':')}, {sexa(dec, '.')}\n")
    outroot = str(tmp_path / "wide")
    make_aterm_image(h5, soltabname="phase000", screen_type="tessellated",
                     outroot=outroot, bounds_deg=[124.565, 66.165, 127.895, 62.835],
                     bounds_mid_deg=[FIELD["rad"], FIELD["dec"]], skymodel=sky,
                     solsetname="sol000", padding_fraction=0, cellsize_deg=0.2,
                     smooth_deg=0.1, ncpu=0)
    _, cube = sffits.read_cube(outroot + "_0.fits")
    assert cube.shape == (4, 2, 3, 4, 17, 17)
    pos = read_patch_positions(sky)
    radec = np.array([pos[n.strip("[]")] for n in s.dir_names])
    lab, _ = tessellation_template(radec, FIELD["rad"], FIELD["dec"],
                                   FIELD["width"], 0.2)
    assert lab.min() >= 1 and lab.max() <= 80 and len(np.unique(lab)) > 40
    ref = get_reference_station(st, 10)
    corr = s.val - s.val[:, :, ref:ref + 1, :]
    want = ov.smooth(ov.gather_planes(lab, corr), 0.5)
    np.testing.assert_allclose(cube, want, rtol=0, atol=1e-6)
    assert os.path.isfile(outroot + "_template.fits")
