"""The fit with 61..128 directions (SF_MAX_FIT_DIR = 128, sf_set_basis_wide):
what the header and the binding declare, and the oracle against the
reference's own fits at D = 80 / 128 (tests/golden/make_golden_wide_fit.py and
the fit of wide80.npz).  CPU only; the kernels are checked in
tests/test_wide_fit.py.

Tolerance of the oracle checks: that of tests/test_oracle_golden.py's fit
cases (coefficients 1e-9 x max(1, |coef|max), residuals 1e-9); orders and
flagged weights bit-equal.
"""

import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from oracle import kl as okl

HEADER = os.path.join(REPO, "include", "screenfit.h")


def test_header_declares_the_wide_fit():
    text = open(HEADER).read()
    assert re.search(r"^#define\s+SF_MAX_FIT_DIR\s+128\b", text, flags=re.M)
    assert re.search(r"^#define\s+SF_MAX_DIR\s+60\b", text, flags=re.M)
    assert re.search(r"^int\s+sf_set_basis_wide\s*\(\s*sf_ctx\s*\*", text, flags=re.M)


def test_binding_declares_the_wide_fit():
    from ska_sdp_screen_fitting_amd import _lib
    assert _lib.SF_MAX_FIT_DIR == 128
    assert _lib.SF_MAX_DIR == 60
    assert callable(_lib.Context.set_basis_wide)
    assert "sf_set_basis_wide" in _lib.EXPORTED


def test_set_basis_wide_rejects_null():
    from ska_sdp_screen_fitting_amd._lib import load_library
    lib = load_library()
    assert lib.sf_set_basis_wide(None, None, 80, 100.0, 5 / 3) == -22
    assert lib.sf_set_basis_wide(None, None, 20, 100.0, 5 / 3) == -22


def test_device_fit_names_the_limit():
    """stationscreen._device_fit refuses D > 128 before it touches a device,
    naming SF_MAX_FIT_DIR."""
    from ska_sdp_screen_fitting_amd import stationscreen
    from ska_sdp_screen_fitting_amd._lib import ScreenFitError
    z = np.zeros((1, 1, 2, 129))
    with pytest.raises(ScreenFitError, match="SF_MAX_FIT_DIR"):
        stationscreen._device_fit(z, z.astype(np.float32), np.zeros((129, 3)),
                                  [5, 5], 0, 2, 5.0, True, -1, 5.0 / 3.0, 100.0)


def _check(r, coef, resid, w_out, orders):
    np.testing.assert_array_equal(r["orders"], orders)
    np.testing.assert_array_equal(r["w_out"], w_out)
    scale = max(1.0, np.abs(coef).max())
    cerr = np.abs(r["coef"] - coef).max()
    rerr = np.abs(r["resid"] - resid).max()
    print("coef err", cerr, "resid err", rerr, "scale", scale)
    assert cerr <= 1e-9 * scale
    assert rerr <= 1e-9


@pytest.mark.parametrize("name", ["wide80", "wide_fit80", "wide_fit128"])
def test_oracle_phase_fit_vs_reference(name):
    g = load_golden(name)
    assert g["val"].shape[-1] in (80, 128)
    r = okl.run_phase(g["val"], g["weight"], g["ant_pos"], g["piercepoints"],
                      int(g["ref_ant"]), int(g["order"]))
    _check(r, g["coef"], g["resid"], g["w_out"], g["orders"])
    # the second pass flagged something beyond the input flags
    assert (g["w_out"] == 0).sum() > (g["weight"] == 0).sum()


@pytest.mark.parametrize("case", ["noref", "ref"])
def test_oracle_tec_fit_vs_reference(case):
    g = load_golden("wide_fit80tec")
    r = okl.run_soltab(g["val"], g["weight"], g["ant_pos"], g["piercepoints"],
                       int(g[f"{case}_ref_ant"]), int(g["order"]), "tec",
                       niter=int(g["niter"]))
    _check(r, g[f"{case}_coef"], g[f"{case}_resid"], g[f"{case}_w_out"],
           g[f"{case}_orders"])
    assert (g[f"{case}_w_out"] == 0).sum() > (g["weight"] == 0).sum()


def test_oracle_amplitude_fit_vs_reference():
    g = load_golden("wide_fit80amp")
    r = okl.run_amplitude(g["amp_val"], g["amp_weight"], g["piercepoints"],
                          int(g["amp_order"]), niter=int(g["niter"]))
    _check(r, g["amp_coef"], g["amp_resid"], g["amp_w_out"], g["amp_orders"])
    assert (g["amp_w_out"] == 0).sum() > (g["amp_weight"] == 0).sum()
