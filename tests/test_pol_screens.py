"""Polarized phase tables end to end: ``stationscreen.run`` on a phase soltab
with a pol axis, ``make_aterm_image`` (KL and tessellated, phase000 and
gain000, ``.npz`` and ``.h5``) and the KLScreen methods, each against the same
work on the XX-only and YY-only scalar tables: planes 0 / 1 of the polarized
cube are the XX table's, planes 2 / 3 the YY table's.  Bit for bit where the
two run the same kernels (the fit, the tessellated fill, the KL evaluation
above 60 directions, the point kernel); elsewhere at the evaluation tolerance
2e-6 max(1, A) (tests/test_wide_eval.py).  Needs an MI355X: every test is
marked ``gpu``.
"""

import numpy as np
import pytest

from conftest import FIELD, load_golden
from pol_cases import (add_amplitudes, golden_table, smooth_table, table, write_h5,
                       write_npz, write_skymodel)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOUNDS = dict(bounds_deg=[124.565, 66.165, 127.895, 62.835],
              bounds_mid_deg=[FIELD["rad"], FIELD["dec"]], padding_fraction=0,
              cellsize_deg=0.2, ncpu=0)


@pytest.fixture(scope="module", autouse=True)
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def soltab_of(g, pol=None):
    from ska_sdp_screen_fitting_amd.h5parm import Solset, Soltab
    ants, dirs = [str(n) for n in g["ant_names"]], [str(n) for n in g["dir_names"]]
    ss = Solset("sol000", ants, g["ant_pos"], dirs, g["dir_radec"])
    axes = ["time", "freq", "ant", "dir"]
    vals = [g["times"], g["freqs"], np.array(ants), np.array(dirs)]
    val, weight = g["val"], g["weight"]
    if pol is None:
        axes, vals = axes + ["pol"], vals + [np.array(["XX", "YY"])]
    else:
        val, weight = val[..., pol], weight[..., pol]
    st = Soltab("phase000", "phase", axes, vals, val, weight, solset=ss)
    ss.soltabs["phase000"] = st
    return st


def run_fit(st, ref, order):
    from ska_sdp_screen_fitting_amd import stationscreen
    rc = stationscreen.run(st, "phase_screen000", order=order, ref_ant=ref,
                           scale_order=True, adjust_order=True)
    assert rc == 0
    ss = st.get_solset()
    scr, res = ss.get_soltab("phase_screen000"), ss.get_soltab("phase_screen000resid")
    return scr.val, res.val, scr.weight, res.weight


def test_run_on_pol_soltab_equals_per_pol_and_reference():
    """stationscreen.run loops the pols, as the reference's does: the result is
    each pol's scalar run bit for bit, and the reference's own coefficients,
    flags and orders at tests/test_gpu_parity.py's fit tolerance."""
    g = load_golden("pol12")
    ref, order = int(g["ref_ant"]), int(g["order"])
    coef, resid, w_out, orders = run_fit(soltab_of(g), ref, order)
    assert coef.shape == (4, 2, 4, 12, 2)
    for p in (0, 1):
        c, r, w, o = run_fit(soltab_of(g, p), ref, order)
        assert np.array_equal(c.view(np.int64), coef[..., p].copy().view(np.int64))
        assert np.array_equal(r.view(np.int64), resid[..., p].copy().view(np.int64))
        assert np.array_equal(w, w_out[..., p]) and np.array_equal(o, orders[..., p])
    np.testing.assert_array_equal(orders[:, :, :, 0, :], g["orders"])
    np.testing.assert_array_equal(w_out, g["w_out"])
    scale = max(1.0, np.abs(g["coef"]).max())
    assert np.abs(coef - g["coef"]).max() <= 1e-8 * scale
    assert np.abs(resid - g["resid"]).max() <= 1e-8


def same_reference_station(g):
    from ska_sdp_screen_fitting_amd.h5parm import get_reference_station
    refs = {get_reference_station(soltab_of(g, p), 10) for p in (None, 0, 1)}
    assert len(refs) == 1, refs


def aterm_cube(path, outroot, screen_type, soltab, skymodel, smooth_deg=0.0):
    from ska_sdp_screen_fitting_amd import fits as sffits
    from ska_sdp_screen_fitting_amd.make_aterm_images import make_aterm_image
    make_aterm_image(path, soltabname=soltab, screen_type=screen_type, outroot=str(outroot),
                     skymodel=skymodel, smooth_deg=smooth_deg, **BOUNDS)
    return sffits.read_cube(str(outroot) + "_0.fits")[1]


@pytest.mark.parametrize("soltab", ["phase000", "gain000"])
@pytest.mark.parametrize("screen_type", ["kl", "tessellated"])
def test_make_aterm_image_polarized(tmp_path, screen_type, soltab):
    g = golden_table(load_golden("pol12"))
    same_reference_station(g)
    if soltab == "gain000":
        g = add_amplitudes(g)
    sky = write_skymodel(tmp_path / "sky.txt", g["dir_names"], g["dir_radec"])
    smooth = 0.1 if screen_type == "tessellated" else 0.0
    xx = aterm_cube(write_npz(tmp_path / "xx.npz", g, pols=0), tmp_path / "xx",
                    screen_type, soltab, sky, smooth)
    yy = aterm_cube(write_npz(tmp_path / "yy.npz", g, pols=1), tmp_path / "yy",
                    screen_type, soltab, sky, smooth)
    assert xx.shape == (4, 2, 4, 4, 17, 17)
    assert np.abs(xx - yy).max() > 0.1  # the pols differ
    amax = max(1.0, np.abs(xx).max(), np.abs(yy).max())
    for name, path in (("npz", write_npz(tmp_path / "pol.npz", g)),
                       ("h5", write_h5(tmp_path / "pol.h5", g))):
        cube = aterm_cube(path, tmp_path / f"pol_{name}", screen_type, soltab, sky, smooth)
        assert cube.shape == xx.shape
        assert np.isfinite(cube).all()
        if screen_type == "tessellated":
            assert np.array_equal(bits(cube[:, :, :, 0:2]), bits(xx[:, :, :, 0:2])), name
            assert np.array_equal(bits(cube[:, :, :, 2:4]), bits(yy[:, :, :, 2:4])), name
        else:
            ex = np.abs(cube[:, :, :, 0:2] - xx[:, :, :, 0:2]).max()
            ey = np.abs(cube[:, :, :, 2:4] - yy[:, :, :, 2:4]).max()
            print(f"{soltab} {name}: max|d| XX {ex:.3g} YY {ey:.3g} A {amax:.3g}")
            assert max(ex, ey) <= 2e-6 * amax


def test_make_aterm_image_polarized_kl_above_60_directions(tmp_path):
    """D = 64: the scalar tables run kl_eval_wide_kernel, which shares the
    contraction order and the epilogue with kl_eval_pol_kernel: the same bits."""
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    s = make_solutions(n_ant=3, n_time=3, n_freq=1, n_dir=64, seed=64, flag_frac=0.01)
    g = table(s, s.val[::-1], s.weight[::-1])
    same_reference_station(g)
    xx = aterm_cube(write_npz(tmp_path / "xx.npz", g, pols=0), tmp_path / "xx", "kl",
                    "phase000", None)
    yy = aterm_cube(write_npz(tmp_path / "yy.npz", g, pols=1), tmp_path / "yy", "kl",
                    "phase000", None)
    cube = aterm_cube(write_npz(tmp_path / "pol.npz", g), tmp_path / "pol", "kl",
                      "phase000", None)
    assert cube.shape == (3, 1, 3, 4, 17, 17)
    assert np.abs(xx - yy).max() > 0.1
    assert np.array_equal(bits(cube[:, :, :, 0:2]), bits(xx[:, :, :, 0:2]))
    assert np.array_equal(bits(cube[:, :, :, 2:4]), bits(yy[:, :, :, 2:4]))


@pytest.mark.parametrize("gain", [False, True])
def test_kl_screen_methods_on_polarized_table(tmp_path, gain):
    """make_matrix, sample (planes and values) and patch_errors of a KLScreen
    with polarized phases against the XX-only and YY-only screens; patch_errors
    below the reference's 0.1 (test_pol_cpu.py checks with the oracle that
    these inputs allow it)."""
    from ska_sdp_screen_fitting_amd.kl_screen import KLScreen
    g = smooth_table()
    same_reference_station(g)
    if gain:
        g = add_amplitudes(g)
    amp = "amplitude000" if gain else None
    paths = [write_npz(tmp_path / "pol.npz", g), write_npz(tmp_path / "xx.npz", g, pols=0),
             write_npz(tmp_path / "yy.npz", g, pols=1)]
    scr = []
    for k, p in enumerate(paths):
        s = KLScreen(f"s{k}", p, None, FIELD["rad"], FIELD["dec"], FIELD["width"],
                     FIELD["width"], amplitude_soltab_name=amp)
        s.process()
        scr.append(s)
    pol, xx, yy = scr
    assert pol.pol_phases and not xx.pol_phases and not yy.pol_phases
    T, F, A, D = g["val"].shape[:4]
    assert np.shape(pol.vals_ph) == (T, F, A, D, 2)
    assert np.array_equal(pol.vals_ph[..., 0], xx.vals_ph)
    assert np.array_equal(pol.vals_ph[..., 1], yy.vals_ph)
    assert pol.get_memory_usage(0.2) == xx.get_memory_usage(0.2)
    # make_matrix: the pixel kernels differ (D <= 60), the evaluation tolerance
    for f, a in ((0, 1), (1, 4)):
        m = [s.make_matrix(0, T, f, a, 0.2, None, 0) for s in scr]
        assert m[0].shape == (T, 4, 17, 17)
        amax = max(1.0, np.abs(m[1]).max(), np.abs(m[2]).max())
        assert np.abs(m[0][:, 0:2] - m[1][:, 0:2]).max() <= 2e-6 * amax
        assert np.abs(m[0][:, 2:4] - m[2][:, 2:4]).max() <= 2e-6 * amax
        assert np.abs(m[1] - m[2]).max() > 0.05
    # sample: two sf_kl_eval_points calls, one per pol -- the scalar screens' bits
    src = np.asarray(pol.source_positions, np.float32)
    ra, de = np.rad2deg(src[:, 0]), np.rad2deg(src[:, 1])
    for cell in (None, 0.2):
        got = [s.sample(ra, de, cell) for s in scr]
        assert got[0].shape == (T, F, A, 4, D)
        assert np.array_equal(got[0][..., 0:2, :], got[1][..., 0:2, :], equal_nan=True)
        assert np.array_equal(got[0][..., 2:4, :], got[2][..., 2:4, :], equal_nan=True)
        vals = [s.sample(ra, de, cell, values=True) for s in scr]
        assert vals[0].shape == (T, F, A, D, 2)
        assert np.array_equal(vals[0][..., 0], vals[1], equal_nan=True)
        assert np.array_equal(vals[0][..., 1], vals[2], equal_nan=True)
        # a time range and small batches take the same values
        part = pol.sample(ra, de, cell, 1, 4, max_batch_bytes=1)
        assert np.array_equal(part, got[0][1:4], equal_nan=True)
        # patch_errors: planes 0 / 1 against the XX phases, 2 / 3 against YY's
        err = [s.patch_errors(cell) for s in scr]
        assert err[0].shape == (D,) and np.isfinite(err[0]).all()
        print("cellsize", cell, "patch errors", err[0])
        if not gain:
            assert np.array_equal(err[0], np.maximum(err[1], err[2]))
            assert err[0].max() < 0.1
            assert err[0].max() > 1e-4  # a fit, not a copy
        else:
            # with amplitudes a scalar screen's planes 2 / 3 carry a_yy with
            # ITS phase: only the pol's own pair compares
            assert np.all(err[0] <= np.maximum(err[1], err[2]))
