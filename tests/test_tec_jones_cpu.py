"""TEC screens to Jones cubes (sf_set_tec_freqs / sf_kl_eval_tec): what can be
checked without a GPU -- the exported symbols, the header, the NULL-context
errors, and the host logic in plain numpy: the per-TEC-frequency channel
grouping (one launch per frequency that has channels) and the axis checks of
``KLTecScreen``'s phase soltab.  The kernel itself: tests/test_tec_jones.py.
"""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "screenfit.h")
SYMBOLS = ("sf_set_tec_freqs", "sf_kl_eval_tec")


def test_library_exports_the_symbols():
    from ska_sdp_screen_fitting_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTED
    assert _lib.SF_MAX_TEC_FREQ == 4096
    assert callable(_lib.Context.set_tec_freqs) and callable(_lib.Context.eval_tec)


def test_header_declares_them():
    with open(HEADER, encoding="utf8") as fh:
        text = fh.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        # ... and the list at the top of the header names them
        assert s in text[:text.index("#ifndef SCREENFIT_H")]
    assert re.search(r"#define\s+SF_MAX_TEC_FREQ\s+4096\b", code)


def test_null_context_is_einval_and_names_the_function():
    from ska_sdp_screen_fitting_amd._lib import load_library
    lib = load_library()
    k = np.ones(2)
    assert lib.sf_set_tec_freqs(None, k.ctypes.data, None, 2, 1) == -22
    assert b"sf_set_tec_freqs" in lib.sf_last_error()
    assert lib.sf_kl_eval_tec(None, None, None, 1, 1, None, 0) == -22
    assert b"sf_kl_eval_tec" in lib.sf_last_error()


# ------------------------------------------------------------ channel grouping

def brute_groups(tec_index, n_tec_freq):
    out = []
    for i in range(n_tec_freq):
        ch = [f for f in range(len(tec_index)) if tec_index[f] == i]
        if ch:
            out.append((i, ch))
    return out


@pytest.mark.parametrize("idx,n", [
    ([0, 1, 1], 2),                 # the GPU tests' binding
    ([2, 0], 3),                    # an unused frequency in the middle
    ([1, 1, 1, 1], 4),              # repeated indices, frequencies 0, 2, 3 unused
    ([3, 0, 3, 1, 0, 3, 3], 5),     # unsorted, repeated, one unused, last unused
    ([0], 1),
    (list(np.random.default_rng(5).integers(0, 9, 64)), 11),
])
def test_channel_grouping_against_a_brute_force_loop(idx, n):
    from ska_sdp_screen_fitting_amd.kl_screen import tec_channel_groups
    got = tec_channel_groups(idx, n)
    want = brute_groups(idx, n)
    assert [(i, list(map(int, ch))) for i, ch in got] == want
    # every channel exactly once; no entry for a frequency without channels
    assert sorted(int(f) for _, ch in got for f in ch) == list(range(len(idx)))
    assert all(len(ch) for _, ch in got)
    assert [i for i, _ in got] == sorted(set(int(i) for i in idx))


def test_channel_grouping_rejects_bad_indices():
    from ska_sdp_screen_fitting_amd.kl_screen import tec_channel_groups
    for idx, n in (([0, 2], 2), ([-1, 0], 2), ([0], 0)):
        with pytest.raises(ValueError):
            tec_channel_groups(idx, n)


# ------------------------------------------------- the phase soltab's axis checks

def soltabs(**phase_changes):
    from ska_sdp_screen_fitting_amd.h5parm import Soltab
    axes = dict(time=np.arange(5) * 8.0 + 4.9e9, freq=np.array([1.3e8, 1.5e8]),
                ant=np.array(["CS001", "CS002", "RS106"]), dir=np.array(["[a]", "[b]", "[c]", "[d]"]))
    names = ["time", "freq", "ant", "dir"]

    def make(name, soltype, ax, order):
        shape = tuple(len(ax[a]) for a in order)
        return Soltab(name, soltype, order, [ax[a] for a in order], np.zeros(shape),
                      np.ones(shape, np.float32))
    tec = make("tec000", "tec", axes, names)
    pax = dict(axes)
    order = phase_changes.pop("order", names)
    pax.update(phase_changes)
    return tec, make("phase000", "phase", pax, order)


def test_phase_soltab_on_the_tec_grid_is_accepted():
    from ska_sdp_screen_fitting_amd.kl_tec_screen import check_phase_soltab_axes
    assert check_phase_soltab_axes(*soltabs()) is False
    # the axis ORDER of the arrays is free (stationscreen.run transposes)
    assert check_phase_soltab_axes(*soltabs(order=["time", "ant", "freq", "dir"])) is False


def test_phase_soltab_with_one_frequency_is_broadcast():
    from ska_sdp_screen_fitting_amd.kl_tec_screen import check_phase_soltab_axes
    assert check_phase_soltab_axes(*soltabs(freq=np.array([1.4e8]))) is True


@pytest.mark.parametrize("axis,value", [
    ("time", np.arange(4) * 8.0 + 4.9e9),                 # another length
    ("time", np.arange(5) * 8.0 + 4.9e9 + 4.0),           # same length, shifted
    ("ant", np.array(["CS001", "CS002"])),
    ("ant", np.array(["CS001", "RS106", "CS002"])),       # another order
    ("dir", np.array(["[a]", "[b]", "[c]", "[e]"])),
    ("freq", np.array([1.3e8, 1.5e8, 1.7e8])),
    ("freq", np.array([1.3e8, 1.6e8])),
])
def test_phase_soltab_off_the_tec_grid_raises(axis, value):
    from ska_sdp_screen_fitting_amd.kl_tec_screen import check_phase_soltab_axes
    with pytest.raises(ValueError, match=rf"\b{axis}\b axis differs"):
        check_phase_soltab_axes(*soltabs(**{axis: value}))


def test_phase_soltab_with_a_pol_axis_raises():
    from ska_sdp_screen_fitting_amd.h5parm import Soltab
    from ska_sdp_screen_fitting_amd.kl_tec_screen import check_phase_soltab_axes
    tec, ph = soltabs()
    names = ["time", "freq", "ant", "dir", "pol"]
    vals = [ph.time, ph.freq, ph.ant, ph.dir, np.array(["XX", "YY"])]
    shape = tuple(len(v) for v in vals)
    pol = Soltab("phase000", "phase", names, vals, np.zeros(shape), np.ones(shape, np.float32))
    with pytest.raises(ValueError, match="pol"):
        check_phase_soltab_axes(tec, pol)


def test_the_keywords_exist_and_default_to_auto():
    import inspect
    from ska_sdp_screen_fitting_amd import kl_tec_screen as m
    for fn in (m.KLTecScreen.write, m.KLTecScreen.write_chunk_gain, m.make_tec_aterm_image):
        assert inspect.signature(fn).parameters["fused"].default == "auto"
    assert inspect.signature(m.KLTecScreen.__init__).parameters["phase_soltab_name"].default is None
    assert inspect.signature(m.make_tec_aterm_image).parameters["phase_soltab_name"].default is None
    assert callable(m.tec_to_phase_coef)
    # the auto rule is a table lookup over the measured shapes
    assert len(m.FUSED_AUTO_WINS) == len(m.FUSED_AUTO_D)
    assert all(len(r) == len(m.FUSED_AUTO_F) for r in m.FUSED_AUTO_WINS)
    for i, D in enumerate(m.FUSED_AUTO_D):
        for j, F in enumerate(m.FUSED_AUTO_F):
            assert m.fused_auto(D, F) == m.FUSED_AUTO_WINS[i][j]
    assert m.fused_auto(m.FUSED_AUTO_D[0] - 1, 10 ** 6) is False
