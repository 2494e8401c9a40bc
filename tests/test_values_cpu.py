"""Screen value cubes and the dTEC a-term file: the host side (no GPU).

The library exports ``sf_kl_eval_values`` and rejects a NULL context;
``fits.tec_header`` gives the cards of the reference's own
``make_template_image(aterm_type="tec")`` (tests/golden/tec_header.json, made
by tests/golden/make_golden_tec_header.py with astropy under the reference's
interpreter); a 5-axis cube written through ``CubeWriter`` with that header
reads back through ``fits.read_cube``; and the tec -> phase coefficient scaling
of the "gain" rendering is k / nu x coef.
"""

import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


def test_library_exports_sf_kl_eval_values():
    from ska_sdp_screen_fitting_amd._lib import EXPORTED, LIB_PATH
    lib = ctypes.CDLL(LIB_PATH)
    assert hasattr(lib, "sf_kl_eval_values")
    assert "sf_kl_eval_values" in EXPORTED


def test_null_context_rejected():
    from ska_sdp_screen_fitting_amd._lib import load_library
    lib = load_library()
    assert lib.sf_kl_eval_values(None, None, 1, None, 1, 0) == -22
    assert b"sf_kl_eval_values" in lib.sf_last_error()


@pytest.fixture(scope="module")
def tec_headers():
    with open(os.path.join(GOLDEN, "tec_header.json"), encoding="utf8") as fh:
        return json.load(fh)


@pytest.mark.parametrize("case,shape", [("t3f1a2_5x5", (3, 1, 2, 5, 5)),
                                        ("t1f2a3_4x6", (1, 2, 3, 4, 6))])
def test_tec_header_matches_reference(tec_headers, case, shape, tmp_path):
    from ska_sdp_screen_fitting_amd import fits as sffits
    c = tec_headers[case]
    assert tuple(c["shape"]) == shape
    cards = sffits.tec_header(c["rad"], c["dec"], c["nx"], c["ny"], c["cellsize_deg"],
                              c["freqs"], c["times"], c["n_ant"])
    want = c["cards"]
    assert [k for k, _ in cards] == [k for k, _ in want]
    for (k, v), (_, v2) in zip(cards, want):
        if isinstance(v2, float):
            # the value as written in the card text (16 significant digits)
            assert float(sffits.card(k, v)[10:30]) == v2, k
        elif k in ("SIMPLE", "EXTEND"):
            assert v is True and v2 == 1
        else:
            assert v == v2 and type(v) is type(v2), k
    # NAXISn are the reversed numpy shape [T][F][A][ny][nx]
    hdr = dict(cards)
    assert hdr["NAXIS"] == 5
    assert tuple(hdr[f"NAXIS{5 - i}"] for i in range(5)) == shape
    if len(c["freqs"]) == 1:
        assert hdr["CDELT4"] == 1e8

    # a [T][F][A][ny][nx] block written with that header round-trips
    data = np.random.default_rng(3).normal(size=shape).astype(np.float32)
    path = str(tmp_path / f"{case}.fits")
    w = sffits.CubeWriter(path, cards, shape)
    w.write(data[:1])
    if shape[0] > 1:
        w.write_raw(np.ascontiguousarray(data[1:], ">f4").tobytes())
    w.close()
    assert os.path.getsize(path) % 2880 == 0
    back_hdr, back = sffits.read_cube(path)
    assert back.shape == shape
    np.testing.assert_array_equal(back, data)
    for k, v in want:
        if k in ("SIMPLE", "EXTEND"):
            assert back_hdr[k] is True
        else:
            assert back_hdr[k] == v, k


def test_tec_to_phase_coefficients():
    """out[t, f, a, d] = k / nu_f x coef[t, f_tec, a, d]: one tec frequency
    broadcasts over F = 3 output frequencies; with several, each output takes
    the tec frequency the index names."""
    torch = pytest.importorskip("torch")
    from ska_sdp_screen_fitting_amd.kl_tec_screen import TEC_TO_PHASE, tec_to_phase_coef
    rng = np.random.default_rng(11)
    nu = np.array([1.2e8, 1.44e8, 1.68e8])
    coef = rng.normal(size=(4, 1, 3, 5))
    coef[1, 0, 2, 3] = np.nan
    got = tec_to_phase_coef(torch.from_numpy(coef), nu).numpy()
    assert TEC_TO_PHASE == -8.4479745e9
    assert got.shape == (4, 3, 3, 5) and got.dtype == np.float64
    want = coef * (TEC_TO_PHASE / nu)[None, :, None, None]
    # one fp64 multiply per element, k / nu rounded once on either side
    np.testing.assert_allclose(got, want, rtol=4e-16, atol=0)
    assert np.isnan(got[1, :, 2, 3]).all() and np.isnan(got).sum() == 3
    # another constant, several tec frequencies
    coef2 = rng.normal(size=(2, 2, 3, 5))
    got2 = tec_to_phase_coef(torch.from_numpy(coef2), nu, 2.5e9, [0, 1, 1]).numpy()
    want2 = coef2[:, [0, 1, 1]] * (2.5e9 / nu)[None, :, None, None]
    np.testing.assert_allclose(got2, want2, rtol=4e-16, atol=0)
    with pytest.raises(ValueError):
        tec_to_phase_coef(torch.from_numpy(coef2), nu)


def test_reexported():
    import ska_sdp_screen_fitting_amd as pkg
    from ska_sdp_screen_fitting_amd.kl_tec_screen import KLTecScreen
    from ska_sdp_screen_fitting_amd.screen import Screen
    assert callable(pkg.make_tec_aterm_image)
    assert issubclass(KLTecScreen, Screen)
