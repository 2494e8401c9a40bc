"""sf_tess_fill_values (csrc/tess_values.hip) and the tessellated TEC products
on the GPU: the unsmoothed gather to the bit, every fused radius and the first
split radius against scipy and against plane 0 of sf_tess_fill, the call's
contract through the raw library, and make_tec_aterm_image end to end.
Expected values come from numpy and scipy (tests/tess_values_cases.py).  Needs
an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest
from scipy import ndimage

from oracle import voronoi as ov
from tess_values_cases import (BOUNDS, N_A, N_F, N_T, NAN_AT, REF, S, SHAPES, SKY,
                               gathered, inputs, screen_of, smoothed, write_tec_h5)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SCRUB = 1       # SF_EVAL_NAN_SCRUB
NT = 1 << 9     # SF_EVAL_NT_STORES
BE = 1 << 10    # SF_EVAL_BIG_ENDIAN
FILL = np.float32(-5.0)


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


def test_flag_values():
    from ska_sdp_screen_fitting_amd import _lib
    assert (_lib.SF_EVAL_NAN_SCRUB, _lib.SF_EVAL_NT_STORES, _lib.SF_EVAL_BIG_ENDIAN) == \
        (SCRUB, NT, BE)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_inputs(nx, ny, D):
    lab, v = inputs(nx, ny, D)
    return (torch.from_numpy(lab.copy()).to("cuda:0"),
            torch.from_numpy(v.copy()).to("cuda:0"))


def fill(ctx, nx, ny, D, sigma=0.0, flags=0, ring=None, offset=0):
    """[min(S, ring), ny, nx] float32 from a buffer pre-filled with -5,
    ``offset`` floats past a 16-byte boundary."""
    lab, v = device_inputs(nx, ny, D)
    n = min(S, ring or S) * nx * ny
    buf = torch.full((n + 4,), float(FILL), dtype=torch.float32, device=lab.device)
    out = buf[offset:offset + n]
    ctx.tess_fill_values(lab, nx, ny, v, D, S, out, ring_slots=ring, smooth_pix=sigma,
                         flags=flags)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:offset] == FILL) and np.all(got[offset + n:] == FILL)
    return got[offset:offset + n].reshape(-1, ny, nx)


def assert_same(got, want):
    """Bit-equal where finite, the same NaN mask."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D", [1, 11, 70, 128])
def test_unsmoothed(ctx, D, shape):
    nx, ny = shape
    want = gathered(nx, ny, D)
    nan = np.isnan(want)
    assert nan.any() and not nan.all()
    raw = fill(ctx, nx, ny, D)
    assert_same(raw, want)
    scrubbed = fill(ctx, nx, ny, D, flags=SCRUB)
    assert np.all(bits(scrubbed)[nan] == 0)            # exactly +0.0f
    assert np.array_equal(bits(scrubbed)[~nan], bits(want)[~nan])
    be = fill(ctx, nx, ny, D, flags=SCRUB | BE)
    assert np.array_equal(bits(be), bits(scrubbed).byteswap())
    # one float past the aligned base: scalar stores
    assert np.array_equal(bits(fill(ctx, nx, ny, D, flags=SCRUB, offset=1)), bits(scrubbed))
    assert np.array_equal(bits(fill(ctx, nx, ny, D, flags=SCRUB | NT)), bits(scrubbed))
    assert np.array_equal(bits(fill(ctx, nx, ny, D, flags=SCRUB | NT | BE)), bits(be))
    # a ring shorter than the call: every entry holds the last slot mapping to it
    last = [max(s for s in range(S) if s % 8 == e) for e in range(8)]
    ring = fill(ctx, nx, ny, D, flags=SCRUB, ring=8)
    assert ring.shape == (8, ny, nx)
    assert np.array_equal(bits(ring), bits(scrubbed[last]))


def test_unsmoothed_options(ctx):
    """Every (slots per item, waves per workgroup) the options can select
    writes the same bits, whole and through a short ring."""
    from ska_sdp_screen_fitting_amd._lib import SF_OPT_TESS_SLOTS, SF_OPT_TESS_WAVES
    nx, ny, D = 40, 12, 11
    want = fill(ctx, nx, ny, D, flags=SCRUB)
    last = [max(s for s in range(S) if s % 8 == e) for e in range(8)]
    try:
        for slots in (1, 3, 16, 256):
            for waves in (4, 8, 16):
                ctx.set_option(SF_OPT_TESS_SLOTS, slots)
                ctx.set_option(SF_OPT_TESS_WAVES, waves)
                assert np.array_equal(bits(fill(ctx, nx, ny, D, flags=SCRUB)), bits(want))
                got = fill(ctx, nx, ny, D, flags=SCRUB, ring=8)
                assert np.array_equal(bits(got), bits(want[last]))
    finally:
        ctx.set_option(SF_OPT_TESS_SLOTS, 0)
        ctx.set_option(SF_OPT_TESS_WAVES, 0)


def scaled_error(got, want):
    fin = np.isfinite(want)
    return float((np.abs(got - want)[fin] / np.maximum(1.0, np.abs(want[fin]))).max())


def check_smoothed(ctx, nx, ny, D, sigma):
    """1e-6 scaled from scipy with scipy's NaN mask; the bits of plane 0 of
    sf_tess_fill(phase = 0, amp_xx = values); NaN -> 0 under the scrub."""
    want = smoothed(nx, ny, D, sigma)
    nan = np.isnan(want)
    assert nan.any() and not nan.all()
    raw = fill(ctx, nx, ny, D, sigma)
    assert np.array_equal(np.isnan(raw), nan)
    err = scaled_error(raw, want)
    print(f"D={D} {nx}x{ny} sigma={sigma}: max scaled error {err:.3g}")
    assert err <= 1e-6
    lab, v = device_inputs(nx, ny, D)
    jones = torch.full((S, 4, ny, nx), float(FILL), dtype=torch.float32, device=lab.device)
    ctx.tess_fill(lab, nx, ny, torch.zeros_like(v), D, S, jones, amp_xx=v,
                  smooth_pix=sigma, flags=0)
    torch.cuda.synchronize()
    assert_same(raw, jones[:, 0].cpu().numpy())
    scrubbed = fill(ctx, nx, ny, D, sigma, flags=SCRUB)
    assert np.all(bits(scrubbed)[nan] == 0)
    assert np.array_equal(bits(scrubbed)[~nan], bits(raw)[~nan])
    return scrubbed


@pytest.mark.parametrize("R", range(1, 25))
def test_every_fused_radius(ctx, R):
    sigma = R / 4.0  # exact in binary: int(4 sigma + 0.5) == R
    assert int(4 * sigma + 0.5) == R
    for D in (11, 70):
        for nx, ny in SHAPES:
            check_smoothed(ctx, nx, ny, D, sigma)


def test_fused_flags_and_ring(ctx):
    """Byte order, the store variants and a short ring on the tile kernel."""
    sigma = 0.5
    last = [max(s for s in range(S) if s % 8 == e) for e in range(8)]
    for D in (11, 70):
        for nx, ny in SHAPES:
            scrubbed = fill(ctx, nx, ny, D, sigma, flags=SCRUB)
            be = fill(ctx, nx, ny, D, sigma, flags=SCRUB | BE)
            assert np.array_equal(bits(be), bits(scrubbed).byteswap())
            for fl, off in ((SCRUB | NT, 0), (SCRUB, 1)):
                got = fill(ctx, nx, ny, D, sigma, flags=fl, offset=off)
                assert np.array_equal(bits(got), bits(scrubbed))
            ring = fill(ctx, nx, ny, D, sigma, flags=SCRUB, ring=8)
            assert np.array_equal(bits(ring), bits(scrubbed[last]))


def test_first_split_radius(ctx):
    """R = 25 > the fused limit: gather, then the two separable passes."""
    from ska_sdp_screen_fitting_amd import ScreenFitError
    sigma = 6.25
    assert int(4 * sigma + 0.5) == 25
    for D in (11, 70):
        for nx, ny in SHAPES:
            scrubbed = check_smoothed(ctx, nx, ny, D, sigma)
            be = fill(ctx, nx, ny, D, sigma, flags=SCRUB | BE)
            assert np.array_equal(bits(be), bits(scrubbed).byteswap())
    with pytest.raises(ScreenFitError, match=r"\(-22\).*ring_slots >= S"):
        fill(ctx, 40, 12, 11, sigma, ring=8)


def raw_call(ctx, lab, nx, ny, v, D, n_slots, out, ring, sigma, flags):
    return ctx.lib.sf_tess_fill_values(
        ctx.h, lab.data_ptr(), nx, ny, v.data_ptr(), D, n_slots, out.data_ptr(), ring,
        float(sigma), flags)


def test_contract(ctx, dev):
    nx, ny, D = 40, 12, 11
    lab_h, v_h = inputs(nx, ny, D)
    lab_h = lab_h.copy()
    lab_h[5, 7], lab_h[9, 30] = 0, D + 1          # outside 1..D
    bad = np.zeros((ny, nx), bool)
    bad[5, 7] = bad[9, 30] = True
    lab = torch.from_numpy(lab_h).to(dev)
    v = torch.from_numpy(v_h.copy()).to(dev)
    want = v_h[:, np.clip(lab_h, 1, D) - 1].astype(np.float32)
    want[:, bad] = np.nan
    # the binding refuses such labels before they reach the library
    out = torch.full((S, ny, nx), float(FILL), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="outside 1..11"):
        ctx.tess_fill_values(lab, nx, ny, v, D, S, out)
    for flags in (0, SCRUB):
        out.fill_(float(FILL))
        assert raw_call(ctx, lab, nx, ny, v, D, S, out, S, 0.0, flags) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        if flags:
            assert np.all(bits(got)[:, bad] == 0)
            exp = np.where(np.isnan(want), np.float32(0.0), want)
            assert np.array_equal(bits(got), bits(exp))
        else:
            assert np.all(np.isnan(got[:, bad]))
            assert_same(got, want)
    # smoothed: the NaN of a bad label spreads as scipy's does, no further
    sm = np.stack([ndimage.gaussian_filter(im, 0.5) for im in want])
    out.fill_(float(FILL))
    assert raw_call(ctx, lab, nx, ny, v, D, S, out, S, 0.5, 0) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(sm))
    assert scaled_error(got, sm) <= 1e-6
    # refusals leave the buffer alone
    out.fill_(float(FILL))
    good = torch.from_numpy(inputs(nx, ny, D)[0].copy()).to(dev)
    for flags in (2, 1 << 8, 1 << 11, 1 << 31):    # not SCRUB / NT / BE (1 << 8: FAST_SINCOS)
        assert raw_call(ctx, good, nx, ny, v, D, S, out, S, 0.0, flags) == -22
    assert raw_call(ctx, good, nx, ny, v, 0, S, out, S, 0.0, 0) == -22
    assert raw_call(ctx, good, nx, ny, v, 129, S, out, S, 0.0, 0) == -22
    assert raw_call(ctx, good, nx, ny, v, D, S, out, 0, 0.0, 0) == -22
    assert raw_call(ctx, good, nx, ny, v, D, S, out, 1 << 31, 0.0, 0) == -22
    assert raw_call(ctx, good, nx, ny, v, D, S, out, S, -1.0, 0) == -22
    assert raw_call(ctx, good, nx, ny, v, D, S, out, S, 1.0e4 + 1.0, 0) == -22
    assert raw_call(ctx, good, nx, ny, v, D, 0, out, S, 0.0, 0) == 0   # S = 0: no-op
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == FILL)


# ------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def tec_h5(tmp_path_factory):
    path = tmp_path_factory.mktemp("tessvalues") / "tec7.h5"
    return str(path), write_tec_h5(path)


def template_labels(s):
    from conftest import FIELD
    from ska_sdp_screen_fitting_amd.voronoi_screen import (read_patch_positions,
                                                           tessellation_template)
    pos = read_patch_positions(SKY)
    radec = np.array([pos[d.strip("[]")] for d in s["dirs"]])
    return tessellation_template(radec, FIELD["rad"], FIELD["dec"], FIELD["width"], 0.2)[0]


def test_tec_cube_end_to_end(dev, tmp_path, tec_h5):
    import os
    from ska_sdp_screen_fitting_amd import fits as sffits
    from ska_sdp_screen_fitting_amd import make_tec_aterm_image
    path, s = tec_h5
    outroot = str(tmp_path / "tess")
    make_tec_aterm_image(path, soltabname="tec000", outroot=outroot, skymodel=SKY,
                         screen_type="tessellated", aterm_type="tec", smooth_deg=0.1,
                         **BOUNDS)
    for suffix in ("_0.fits", "_template.fits", ".txt"):
        assert os.path.exists(outroot + suffix), suffix
    assert open(outroot + ".txt").read().split() == [outroot + "_0.fits"]
    hdr, cube = sffits.read_cube(outroot + "_0.fits")
    assert cube.shape == (N_T, N_F, N_A, 17, 17) and cube.dtype == np.dtype(">f4")
    cards = sffits.tec_header(126.23, 64.50, 17, 17, 0.2, s["freqs"], s["times"], N_A)
    assert list(hdr) == [k for k, _ in cards]
    for k, v in cards:
        if isinstance(v, float):
            assert hdr[k] == float(sffits.card(k, v)[10:30]), k
        else:
            assert hdr[k] == v, k
    lab = template_labels(s)
    assert lab.shape == (17, 17) and set(np.unique(lab)) == set(range(1, 8))
    ref = s["val"] - s["val"][:, :, REF:REF + 1]
    img = ref[..., lab - 1].astype(np.float32)          # [T, F, A, 17, 17]
    want = np.stack([ndimage.gaussian_filter(im, 0.5) for im in img.reshape(-1, 17, 17)])
    want = want.reshape(img.shape)
    nan = np.isnan(want)
    assert nan.any() and not nan[NAN_AT[:3]].all()
    got = np.asarray(cube, np.float32)
    assert np.all(bits(got)[nan] == 0)
    assert scaled_error(got, want) <= 1e-6
    assert np.all(got[:, :, REF] == 0.0)
    assert np.any(got != 0.0)
    # make_matrix: the unsmoothed, unscrubbed slice of the same images
    scr = screen_of(path)
    scr.process()
    m = scr.make_matrix(1, 3, 0, 2, 0.2, out_dir=str(tmp_path))
    assert m.shape == (2, 17, 17) and m.dtype == np.float64
    assert_same(m.astype(np.float32), img[1:3, 0, 2])
    assert np.isnan(m).any()
    # smooth_deg = 0: the cube's slice IS make_matrix, bit for bit (NaN scrubbed)
    outroot0 = str(tmp_path / "tess0")
    make_tec_aterm_image(path, soltabname="tec000", outroot=outroot0, skymodel=SKY,
                         screen_type="tessellated", aterm_type="tec", **BOUNDS)
    cube0 = np.asarray(sffits.read_cube(outroot0 + "_0.fits")[1], np.float32)
    assert np.array_equal(bits(cube0[1:3, 0, 2]),
                          bits(np.where(np.isnan(m), 0.0, m).astype(np.float32)))


def test_gain_cube_end_to_end(dev, tmp_path, tec_h5):
    from ska_sdp_screen_fitting_amd import fits as sffits
    from ska_sdp_screen_fitting_amd import make_tec_aterm_image
    from ska_sdp_screen_fitting_amd.kl_tec_screen import TEC_TO_PHASE
    from ska_sdp_screen_fitting_amd.screen import nearest_index
    path, s = tec_h5
    nu = np.array([1.2e8, 1.5e8, 1.8e8])
    lab = template_labels(s)
    ref = s["val"] - s["val"][:, :, REF:REF + 1]
    phi = s["phi"] - s["phi"][:, :, REF:REF + 1]
    fidx = nearest_index(s["freqs"], nu)
    for name, phi0 in ((None, None), ("phase000", np.repeat(phi, N_F, axis=1))):
        outroot = str(tmp_path / f"gain_{name}")
        make_tec_aterm_image(path, soltabname="tec000", outroot=outroot, skymodel=SKY,
                             screen_type="tessellated", aterm_type="gain", freqs_hz=nu,
                             smooth_deg=0.1, phase_soltab_name=name, **BOUNDS)
        hdr, cube = sffits.read_cube(outroot + "_0.fits")
        assert cube.shape == (N_T, 3, N_A, 4, 17, 17)
        phase = ref[:, fidx] * (TEC_TO_PHASE / nu)[None, :, None, None]
        if phi0 is not None:
            phase = phase + phi0[:, fidx]
        want = ov.smooth(ov.gather_planes(lab, phase.reshape(-1, 7)), 0.5)
        want = want.reshape(N_T, 3, N_A, 4, 17, 17)
        nan = np.isnan(want)
        assert nan.any()
        for p in range(4):
            want[:, :, :, p][nan[:, :, :, p]] = 0.0 if p % 2 else 1.0
        err = float(np.abs(np.asarray(cube, np.float64) - want).max())
        print(f"gain cube, phase soltab {name}: max |d| {err:.3g}")
        assert err <= 1e-6
        assert np.all(np.asarray(cube)[:, :, REF, 0::2] == 1.0)
        assert np.all(np.asarray(cube)[:, :, REF, 1::2] == 0.0)


def test_one_direction_is_tessellated(dev, tmp_path):
    """screen_type="kl" with one direction takes the tessellated path (Q14):
    every pixel of a slot is that slot's referenced value."""
    from ska_sdp_screen_fitting_amd import fits as sffits
    from ska_sdp_screen_fitting_amd import make_tec_aterm_image
    path = str(tmp_path / "tec1.h5")
    s = write_tec_h5(path, n_dir=1)
    outroot = str(tmp_path / "one")
    make_tec_aterm_image(path, soltabname="tec000", outroot=outroot, skymodel=SKY,
                         screen_type="kl", aterm_type="tec", **BOUNDS)
    hdr, cube = sffits.read_cube(outroot + "_0.fits")
    assert cube.shape == (N_T, N_F, N_A, 17, 17)
    ref = (s["val"] - s["val"][:, :, REF:REF + 1])[..., 0].astype(np.float32)
    assert np.any(ref != 0.0)
    assert np.array_equal(bits(np.asarray(cube, np.float32)),
                          bits(np.broadcast_to(ref[..., None, None], cube.shape)))
