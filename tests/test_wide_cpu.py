"""The pixel-side direction limit (SF_MAX_EVAL_DIR = 128, sf_set_piercepoints)
in the header and the binding, and the oracle pinned to the reference's own
D = 80 planes (tests/golden/make_golden_wide.py).  CPU only."""

import os
import re

import numpy as np

from conftest import REPO, load_golden
from oracle import geometry as og
from oracle import kl as okl

HEADER = os.path.join(REPO, "include", "screenfit.h")


def test_header_declares_the_eval_limit_and_entry_point():
    text = open(HEADER).read()
    assert re.search(r"^#define\s+SF_MAX_EVAL_DIR\s+128\b", text, flags=re.M)
    assert re.search(r"^#define\s+SF_MAX_DIR\s+60\b", text, flags=re.M)
    assert re.search(r"^#define\s+SF_EVAL_KERNEL_WIDE\s+9\b", text, flags=re.M)
    assert re.search(r"^int\s+sf_set_piercepoints\s*\(\s*sf_ctx\s*\*", text, flags=re.M)


def test_binding_constants_and_symbol():
    from ska_sdp_screen_fitting_amd import _lib
    assert _lib.SF_MAX_EVAL_DIR == 128
    assert _lib.SF_MAX_DIR == 60
    assert _lib.SF_EVAL_KERNEL_WIDE == 9
    assert _lib.EVAL_KERNEL_NAMES[_lib.SF_EVAL_KERNEL_WIDE] == "kl_eval_wide_kernel"
    assert "sf_set_piercepoints" in _lib.EXPORTED
    assert hasattr(_lib.Context, "set_piercepoints")
    lib = _lib.load_library()
    # NULL context: refused before any device call
    assert lib.sf_set_piercepoints(None, None, 80, 100.0, 5 / 3) == -22


def test_wide_golden_shape():
    g = load_golden("wide80")
    T, F, A, D = g["val"].shape
    assert D == 80 and g["coef"].shape == (T, F, A, D)
    assert g["kl17"].shape == (len(g["pairs17"]), T, 2, 17, 17)
    assert (g["weight"] == 0).any() and np.isfinite(g["coef"]).all()
    pp, mra, mdec = og.piercepoints(g["dir_radec"])
    assert mra == g["mid_ra"] and mdec == g["mid_dec"]
    np.testing.assert_allclose(pp, g["piercepoints"], rtol=0, atol=1e-8)


def test_oracle_eval_matches_reference_at_80_directions():
    g = load_golden("wide80")
    cpix = okl.cpix_matrix(g["piercepoints"], g["x17"], g["y17"])
    assert cpix.shape == (17 * 17, 80)
    for k, (f, s) in enumerate(g["pairs17"]):
        ph = okl.eval_phase_screens(g["coef"][:, f, s, :], cpix)
        planes = okl.eval_planes(ph)[:, 0:2]
        ref = g["kl17"][k].reshape(planes.shape)
        np.testing.assert_allclose(planes, ref, rtol=0, atol=1e-12)
