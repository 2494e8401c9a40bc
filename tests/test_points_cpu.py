"""Sampling screens at sky positions: the host side (no GPU).

The library exports sf_set_points / sf_kl_eval_points /
sf_kl_eval_point_values and rejects NULL contexts; ``geometry.screen_xy`` is
the projection of ``piercepoints`` (bit for bit), ``geometry.patch_pixels`` the
pixel lookup of the reference's acceptance test (tests/test_fit_screens.py);
and the quantity ``KLScreen.patch_errors`` returns, restated in numpy from the
reference's own coefficients, is below the reference's threshold 0.1 in every
direction of its fixture.
"""

import ctypes

import numpy as np
import pytest

from conftest import FIELD, load_golden

SYMBOLS = ("sf_set_points", "sf_kl_eval_points", "sf_kl_eval_point_values")


def test_library_exports_the_point_symbols():
    from ska_sdp_screen_fitting_amd._lib import EXPORTED, LIB_PATH
    lib = ctypes.CDLL(LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in EXPORTED


def test_null_context_rejected():
    from ska_sdp_screen_fitting_amd._lib import load_library
    lib = load_library()
    xy = np.zeros((3, 2))
    assert lib.sf_set_points(None, xy.ctypes.data, 3) == -22
    assert lib.sf_last_error()
    assert lib.sf_kl_eval_points(None, None, None, None, 1, None, 0) == -22
    assert lib.sf_kl_eval_point_values(None, None, 1, None) == -22


@pytest.mark.parametrize("name", ["fixture_kl", "synth20", "wide80"])
def test_screen_xy_is_the_piercepoint_projection(name):
    """Bit for bit the (x, y) of ``geometry.piercepoints`` -- so a screen
    sampled at a direction's own position is the fit's model there.  The
    golden's ``piercepoints`` array is the reference's (astropy.wcs) and
    differs from this closed form in the last digits (4e-11 of up to 4e3
    pixels of 0.0005 deg measured; 1e-9 pixel = 5e-13 deg allowed)."""
    from ska_sdp_screen_fitting_amd import geometry
    g = load_golden(name)
    src = np.asarray(g["dir_radec"], np.float32)
    pp, mid_ra, mid_dec = geometry.piercepoints(src)
    assert mid_ra == float(g["mid_ra"]) and mid_dec == float(g["mid_dec"])
    x, y = geometry.screen_xy(np.rad2deg(src[:, 0]), np.rad2deg(src[:, 1]),
                              float(g["mid_ra"]), float(g["mid_dec"]))
    np.testing.assert_array_equal(x, pp[:, 0])
    np.testing.assert_array_equal(y, pp[:, 1])
    assert geometry._pp_xy is geometry.screen_xy
    np.testing.assert_allclose(x, g["piercepoints"][:, 0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(y, g["piercepoints"][:, 1], rtol=0, atol=1e-9)


def test_patch_pixels_fixture():
    from ska_sdp_screen_fitting_amd import geometry
    g = load_golden("fixture_kl")
    ra, de = g["radec_patch"][:, 0], g["radec_patch"][:, 1]
    ix, iy, inside = geometry.patch_pixels(ra, de, FIELD["rad"], FIELD["dec"],
                                           FIELD["width"], 0.2)
    assert list(zip(ix.tolist(), iy.tolist())) == [
        (1, 11), (14, 11), (11, 8), (15, 0), (2, 0), (5, 3), (8, 5)]
    assert inside.all()
    ix, iy, inside = geometry.patch_pixels(ra, de, FIELD["rad"], FIELD["dec"],
                                           FIELD["width"], 0.02602)
    want = np.round(g["patch_pix128"]).astype(int)
    np.testing.assert_array_equal(ix, want[0])
    np.testing.assert_array_equal(iy, want[1])
    assert inside.all()


def test_patch_pixels_masks_positions_off_the_field():
    from ska_sdp_screen_fitting_amd import geometry
    ra = np.array([FIELD["rad"], FIELD["rad"]])
    de = np.array([FIELD["dec"], FIELD["dec"] + 3.0])
    _, _, inside = geometry.patch_pixels(ra, de, FIELD["rad"], FIELD["dec"],
                                         FIELD["width"], 0.2)
    assert inside.tolist() == [True, False]


def numpy_patch_errors(g, coef, x, y, cellsize_deg):
    """KLScreen.patch_errors(cellsize) restated: the screen of ``coef`` at
    pixel (iy, ix) of the grid (x, y) -- the point (x[ix], y[iy]), Q8 --
    against cos / sin of the referenced input phases."""
    from ska_sdp_screen_fitting_amd import geometry
    src = np.asarray(g["dir_radec"], np.float32)
    ix, iy, inside = geometry.patch_pixels(
        np.rad2deg(src[:, 0]), np.rad2deg(src[:, 1]), FIELD["rad"], FIELD["dec"],
        FIELD["width"], cellsize_deg)
    assert inside.all()
    pp, r0, beta = g["piercepoints"], float(g["r_0"]), float(g["beta"])
    d2 = ((pp[None, :, 0] - x[ix][:, None]) ** 2 + (pp[None, :, 1] - y[iy][:, None]) ** 2
          + pp[None, :, 2] ** 2)
    c = -((d2 / r0 ** 2) ** (beta / 2)) / 2          # [P = D][D]
    scr = np.einsum("tfad,pd->tfap", g["coef"] if coef is None else coef, c)
    val = np.asarray(g["val"])
    ref = int(g["ref_ant"])
    phi = val - val[:, :, ref:ref + 1, :]
    use = (np.asarray(g["weight"]) != 0) & np.isfinite(val)
    err = np.zeros(len(ix))
    for got, want in ((np.cos(scr), np.cos(phi)), (np.sin(scr), np.sin(phi))):
        diff = np.where(use, np.abs(got - want), 0.0)
        err = np.maximum(err, diff.reshape(-1, len(ix)).max(axis=0))
    return err


def test_reference_coefficients_pass_the_reference_criterion():
    """tests/test_fit_screens.py::test_fit_kl_screens of the reference:
    |cube at the patch pixel - cos / sin of the corrections| < 0.1."""
    g = load_golden("fixture_kl")
    err = numpy_patch_errors(g, None, g["x17"], g["y17"], 0.2)
    print("patch errors per direction:", np.round(err, 4))
    assert err.shape == (7,)
    assert np.all(err < 0.1)
    # the figures measured with the reference's outputs (4 decimals)
    np.testing.assert_allclose(
        err, [0.0248, 0.0143, 0.0340, 0.0077, 0.0746, 0.0585, 0.0416], atol=5e-5)
