"""Tessellated TEC screens, the parts that need no GPU: the sf_tess_fill_values
symbol, VoronoiTecScreen.fit (referencing, soltab checks, the phase soltab),
the gain cube's phase assembly, get_memory_usage and the screen_type check of
make_tec_aterm_image."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from tess_values_cases import N_A, N_F, N_T, NAN_AT, REF, screen_of, write_tec_h5

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def tec_h5(tmp_path_factory):
    path = tmp_path_factory.mktemp("tessvalues") / "tec7.h5"
    return path, write_tec_h5(path)


def test_symbol_declared_exported_and_listed():
    from ska_sdp_screen_fitting_amd._lib import EXPORTED, LIB_PATH, load_library
    header = open(os.path.join(REPO, "include", "screenfit.h")).read()
    assert re.search(r"^int sf_tess_fill_values\s*\(", header, flags=re.M)
    assert hasattr(ctypes.CDLL(LIB_PATH), "sf_tess_fill_values")
    assert "sf_tess_fill_values" in EXPORTED
    lib = load_library()
    assert lib.sf_tess_fill_values(None, None, 4, 4, None, 1, 1, None, 1, 0.0, 0) == -22
    assert b"sf_tess_fill_values" in lib.sf_last_error()


def test_fit_references_values(tec_h5):
    path, s = tec_h5
    scr = screen_of(path)
    scr.fit()
    assert scr.ref_ind == REF
    val = s["val"]
    assert scr.vals_ph.shape == (N_T, N_F, N_A, 7) and scr.vals_ph.dtype == np.float64
    np.testing.assert_array_equal(scr.vals_ph, val - val[:, :, REF:REF + 1])
    assert np.all(scr.vals_ph[:, :, REF] == 0.0)
    assert np.isnan(scr.vals_ph[NAN_AT]) and np.isnan(scr.vals_ph).sum() == 1
    assert scr.vals_phi0 is None
    np.testing.assert_array_equal(scr.times_ph, s["times"])
    np.testing.assert_array_equal(scr.freqs_ph, s["freqs"])
    assert [str(d) for d in scr.source_names] == s["dirs"]
    assert [str(a) for a in scr.station_names] == s["ants"]
    assert len(scr.source_positions) == 7 and len(scr.station_positions) == N_A


def test_fit_refuses_other_soltabs(tec_h5):
    path, _ = tec_h5
    with pytest.raises(ValueError, match="of type 'phase' cannot be fitted"):
        screen_of(path, tec_soltab_name="phase000").fit()
    with pytest.raises(ValueError, match="no pol axis"):
        screen_of(path, phase_soltab_name="phasepol000").fit()
    with pytest.raises(ValueError, match="is not a phase soltab"):
        screen_of(path, phase_soltab_name="tec000").fit()


def test_fit_phase_soltab(tec_h5):
    path, s = tec_h5
    scr = screen_of(path, phase_soltab_name="phase000")
    scr.fit()
    phi = s["phi"] - s["phi"][:, :, REF:REF + 1]
    assert scr.vals_phi0.shape == (N_T, N_F, N_A, 7)   # the one frequency, broadcast
    np.testing.assert_array_equal(scr.vals_phi0[:, 0], phi[:, 0])
    np.testing.assert_array_equal(scr.vals_phi0[:, 1], phi[:, 0])
    assert np.all(scr.vals_phi0[:, :, REF] == 0.0)
    two = screen_of(path, phase_soltab_name="phase2f000")
    two.fit()
    np.testing.assert_array_equal(two.vals_phi0[:, 1], 2.0 * phi[:, 0])


@pytest.mark.parametrize("f_tec", [1, 2])
def test_gain_phase_assembly(f_tec):
    """tess_gain_phases = tec * (tec_to_phase / nu) + phi0 at the nearest TEC
    frequency.  torch divides a scalar by a tensor as scalar * (1 / tensor), so
    the scale may differ from numpy's quotient by one rounding and the product
    by one more: 4 ulp of the larger term bounds both and the sum."""
    from ska_sdp_screen_fitting_amd.kl_tec_screen import TEC_TO_PHASE
    from ska_sdp_screen_fitting_amd.screen import nearest_index
    from ska_sdp_screen_fitting_amd.voronoi_tec_screen import tess_gain_phases
    rng = np.random.default_rng(f_tec)
    tec = rng.uniform(-0.5, 0.5, (3, f_tec, 4, 7))
    tec[1, 0, 2, 3] = np.nan
    phi0 = rng.uniform(-0.3, 0.3, tec.shape)
    freqs_tec = np.array([1.2e8, 1.6e8])[:f_tec]
    nu = np.array([1.1e8, 1.39e8, 1.41e8, 1.9e8])
    fidx = np.zeros(4, int) if f_tec == 1 else nearest_index(freqs_tec, nu)
    if f_tec == 2:
        assert fidx.tolist() == [0, 0, 1, 1]
    for k in (TEC_TO_PHASE, 1.0e9):
        scale = (k / nu)[None, :, None, None]
        got = tess_gain_phases(torch.from_numpy(tec), freqs_tec, nu, k)
        assert got.shape == (3, 4, 4, 7)
        term = tec[:, fidx] * scale
        tol = 4 * np.finfo(np.float64).eps * np.nanmax(np.abs(term))
        np.testing.assert_allclose(got.numpy(), term, rtol=0, atol=tol)
        assert np.array_equal(np.isnan(got.numpy()), np.isnan(term))
        got = tess_gain_phases(torch.from_numpy(tec), freqs_tec, nu, k,
                               torch.from_numpy(phi0))
        np.testing.assert_allclose(got.numpy(), term + phi0[:, fidx], rtol=0, atol=tol)


def test_memory_usage(tec_h5):
    path, _ = tec_h5
    scr = screen_of(path)
    scr.fit()
    per_plane = 8 * N_A * 16 * 16 / 1024 ** 3 * 10   # int(3.33 / 0.2) = 16
    assert scr.get_memory_usage(0.2) == pytest.approx(N_F * per_plane, rel=1e-12)
    assert scr.get_memory_usage(0.2, "tec", 5) == pytest.approx(5 * per_plane, rel=1e-12)
    assert scr.get_memory_usage(0.2, "gain", 3) == pytest.approx(12 * per_plane, rel=1e-12)


def test_unknown_screen_type_raises_first():
    """Before the file is opened or a device touched."""
    from ska_sdp_screen_fitting_amd import make_tec_aterm_image
    with pytest.raises(ValueError, match="unknown screen_type 'bogus'"):
        make_tec_aterm_image("/nonexistent/file.h5", screen_type="bogus")


def test_make_tec_aterm_image_keeps_its_arguments():
    """The new keywords are appended with defaults: earlier calls are unchanged."""
    import inspect
    from ska_sdp_screen_fitting_amd.kl_tec_screen import make_tec_aterm_image
    p = list(inspect.signature(make_tec_aterm_image).parameters.values())
    assert [q.name for q in p[-3:]] == ["phase_soltab_name", "screen_type", "smooth_deg"]
    assert p[-2].default == "kl" and p[-1].default == 0
