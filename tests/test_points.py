"""Screens sampled at positions (sf_set_points, sf_kl_eval_points,
sf_kl_eval_point_values; csrc/kl_points.hip) and their public interface
(KLEvaluator.set_points / sample_*, KLScreen.sample / patch_errors).

Checked against
  * the reference's own cube planes (``kl17`` / ``gain17`` of the goldens)
    with all 289 grid positions bound as points: 1e-6, the project's cos / sin
    tolerance; gain 1e-6 / 2e-6 max(1, |ref|) as
    tests/test_gain.py;
  * ``sf_kl_eval`` of the same grid in the same context (1e-6), whose bytes
    ``sf_set_points`` must not change;
  * the piercepoint identity: the screen at the piercepoints IS the fit's
    model, C coef = (val - val[ref]) - resid, which holds to <= 2e-12 in fp64
    numpy on the goldens; a GPU contraction in another summation order adds
    rounding of that size, and 1e-9 is the three decades of room the project
    gives its fits (1e-11 measured, 1e-8 allowed);
  * fp64 numpy (``c = -((d2 / r0**2) ** (beta/2)) / 2``) on seeded random
    coefficients at every shape where the kernel takes another path: point
    counts round the 16-point tile and the 32-point pass, slot counts round
    the 16-slot group and the 64-slot workgroup, direction counts round the
    k-step pairs, the basis in LDS and read through L2, NaN slots, outputs
    offset by one element.
Every output is pre-filled with a sentinel and carries a guard row after [S]
that must stay untouched.  Needs an MI355X: every test is marked ``gpu``.
"""

import os

import numpy as np
import pytest

from conftest import FIELD, GOLDEN, load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FAST = 1 << 8   # SF_EVAL_FAST_SINCOS
SCRUB = 1       # SF_EVAL_NAN_SCRUB
BE = 1 << 10    # SF_EVAL_BIG_ENDIAN
SENT = -7.0


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


def up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)


def planes_at(ctx, dev, coef, flags, xx=None, yy=None, offset=0):
    """sf_kl_eval_points into a sentinel-filled buffer with a guard row after
    [S] (and ``offset`` elements in front): host [S][4][P] float32."""
    S, P = coef.shape[0], ctx.points
    n = S * 4 * P
    buf = torch.full((offset + n + 4 * P,), SENT, dtype=torch.float32, device=dev)
    out = buf[offset:offset + n]
    ctx.eval_points(up(dev, coef), S, out, None if xx is None else up(dev, xx),
                    None if yy is None else up(dev, yy), flags)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(h[:offset] == SENT) and np.all(h[offset + n:] == SENT), "guard"
    got = h[offset:offset + n].reshape(S, 4, P)
    assert not np.any(got == SENT), "an output element was not written"
    return got


def values_at(ctx, dev, coef, offset=0):
    """sf_kl_eval_point_values likewise: host [S][P] float64."""
    S, P = coef.shape[0], ctx.points
    n = S * P
    buf = torch.full((offset + n + P,), SENT, dtype=torch.float64, device=dev)
    ctx.eval_point_values(up(dev, coef), S, buf[offset:offset + n])
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(h[:offset] == SENT) and np.all(h[offset + n:] == SENT), "guard"
    got = h[offset:offset + n].reshape(S, P)
    assert not np.any(got == SENT), "an output element was not written"
    return got


def grid_points(x, y):
    """All grid positions, pixel (j, i) -> point j * nx + i at (x[i], y[j])."""
    X, Y = np.meshgrid(x, y)  # [ny][nx]
    return np.stack([X.ravel(), Y.ravel()], axis=1)


def cpix_np(pp, xy, r0=100.0, beta=5.0 / 3.0):
    d2 = ((pp[None, :, 0] - xy[:, None, 0]) ** 2 + (pp[None, :, 1] - xy[:, None, 1]) ** 2
          + pp[None, :, 2] ** 2)
    return -((d2 / r0 ** 2) ** (beta / 2)) / 2   # [P][D]


def bind(ctx, g):
    ctx.set_piercepoints(g["piercepoints"], float(g["r_0"]) if "r_0" in g else 100.0,
                         float(g["beta"]) if "beta" in g else 5.0 / 3.0)


# ------------------------------------------------- 1. / 3. the reference's cube

@pytest.mark.parametrize("name", ["fixture_kl", "synth12tiny", "synth20", "synth50",
                                  "wide80"])
def test_points_vs_reference_cube_and_grid_eval(ctx, dev, name):
    g = load_golden(name)
    bind(ctx, g)
    ctx.set_grid(g["x17"], g["y17"])
    f0, a0 = (int(v) for v in g["pairs17"][0])
    c0 = up(dev, g["coef"][:, f0, a0, :])
    S = c0.shape[0]
    before = torch.full((S, 4, 17, 17), SENT, dtype=torch.float32, device=dev)
    ctx.eval(c0, S, before, flags=FAST)
    ctx.set_points(grid_points(g["x17"], g["y17"]))
    assert ctx.points == 289
    after = torch.full((S, 4, 17, 17), SENT, dtype=torch.float32, device=dev)
    ctx.eval(c0, S, after, flags=FAST)
    torch.cuda.synchronize()
    # sf_kl_eval writes the same bytes before and after sf_set_points
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    for flags in (0, FAST):
        for k, (f, a) in enumerate(g["pairs17"]):
            coef = g["coef"][:, int(f), int(a), :]
            got = planes_at(ctx, dev, coef, flags).reshape(S, 4, 17, 17)
            ref = g["kl17"][k]  # [T][2][17][17]
            err = np.abs(got[:, 0:2] - ref).max()
            cube = torch.full((S, 4, 17, 17), SENT, dtype=torch.float32, device=dev)
            ctx.eval(up(dev, coef), S, cube, flags=flags)
            torch.cuda.synchronize()
            dcube = np.abs(got - cube.cpu().numpy()).max()
            print(f"{name} pair {k} flags={flags:#x}: vs reference {err:.3g}, "
                  f"vs sf_kl_eval {dcube:.3g}")
            assert err <= 1e-6
            assert dcube <= 1e-6
            np.testing.assert_array_equal(got[:, 2:4], got[:, 0:2])


# ----------------------------------------------------------------- 2. gain

@pytest.mark.parametrize("fast", [False, True])
def test_gain_points_vs_reference_cube(ctx, dev, fast):
    g = load_golden("gain12")
    bind(ctx, g)
    ctx.set_points(grid_points(g["x17"], g["y17"]))
    tol = 2e-6 if fast else 1e-6
    for k, (f, a) in enumerate(g["pairs"]):
        got = planes_at(ctx, dev, g["coef"][:, f, a, :], FAST if fast else 0,
                        g["amp_interp"][:, f, a, :, 0], g["amp_interp"][:, f, a, :, 1])
        ref = g["gain17"][k]  # [T][4][17][17]
        err = (np.abs(got.reshape(ref.shape) - ref) / np.maximum(1.0, np.abs(ref))).max()
        print(f"gain12 pair {k} fast={fast}: {err:.3g}")
        assert err <= tol


# -------------------------------------------- 4. / 5. the piercepoint identity

def identity_slots(coef, ref):
    use = np.any(coef != 0, axis=-1)
    use[:, :, ref] = False
    return use


@pytest.mark.parametrize("name", ["fixture_kl", "synth20", "synth50", "wide_fit80",
                                  "wide_fit128"])
def test_values_at_piercepoints_are_the_fit_model(ctx, dev, name):
    g = load_golden(name)
    bind(ctx, g)
    ctx.set_points(g["piercepoints"][:, :2])
    D = g["coef"].shape[-1]
    got = values_at(ctx, dev, g["coef"].reshape(-1, D)).reshape(g["coef"].shape)
    ref = int(g["ref_ant"])
    want = (g["val"] - g["val"][:, :, ref:ref + 1, :]) - g["resid"]
    use = identity_slots(g["coef"], ref)
    assert use.sum() >= 6
    err = np.abs(got - want)[use].max()
    print(f"{name}: {use.sum()} slots, max |C coef - model| = {err:.3g}")
    assert err <= 1e-9


@pytest.mark.parametrize("name", ["synth20", "wide_fit80"])
def test_fit_then_sample(ctx, dev, name):
    from ska_sdp_screen_fitting_amd.stationscreen import station_orders
    g = load_golden(name)
    ref = int(g["ref_ant"])
    st = station_orders(g["ant_pos"], ref, int(g["order"]))
    pp = g["piercepoints"]
    if name == "wide_fit80":
        ctx.set_basis_wide(pp, float(g["r_0"]), float(g["beta"]))
    else:
        ctx.set_basis(pp, float(g["r_0"]), float(g["beta"]))
    T, F, A, D = g["val"].shape
    ph = up(dev, g["val"])
    wt = torch.from_numpy(np.ascontiguousarray(g["weight"], np.float32)).to(dev)
    coef = torch.full_like(ph, SENT)
    resid = torch.full_like(ph, SENT)
    ctx.fit(ph, wt, T, F, A, st, ref_ant=ref, coef=coef, resid=resid)
    ctx.set_points(pp[:, :2])
    vals = torch.full((T * F * A + 1, D), SENT, dtype=torch.float64, device=dev)
    ctx.eval_point_values(coef, T * F * A, vals)
    torch.cuda.synchronize()
    assert torch.all(vals[-1] == SENT)
    got = vals[:-1].cpu().numpy().reshape(T, F, A, D)
    c = coef.cpu().numpy()
    want = (g["val"] - g["val"][:, :, ref:ref + 1, :]) - resid.cpu().numpy()
    use = identity_slots(c, ref)
    assert use.sum() >= 6
    err = np.abs(got - want)[use].max()
    print(f"{name}: {use.sum()} fitted slots, max |C coef - model| = {err:.3g}")
    assert err <= 1e-9


# ------------------------------------------------------------------ 6. edges

def synth_geometry(D, P, seed):
    """D piercepoints over a field of +-3000 piercepoint pixels (1.5 deg; the
    goldens span ~4000) and P positions over the same field plus a margin."""
    rng = np.random.default_rng(seed)
    pp = np.zeros((D, 3))
    pp[:, :2] = rng.uniform(-3000.0, 3000.0, (D, 2))
    xy = rng.uniform(-3500.0, 3500.0, (P, 2))
    return pp, xy, rng


def check_against_numpy(ctx, dev, D, P, S, seed):
    pp, xy, rng = synth_geometry(D, P, seed)
    ctx.set_piercepoints(pp)
    ctx.set_points(xy)
    c = cpix_np(pp, xy)
    coef = rng.normal(0, 0.01, (S, D))
    coef[S // 2:] *= 30.0      # phases over many turns: the exact reduction
    v = coef @ c.T
    got_v = values_at(ctx, dev, coef)
    ev = (np.abs(got_v - v) / np.maximum(1.0, np.abs(v))).max()
    want = np.stack([np.cos(v), np.sin(v), np.cos(v), np.sin(v)], axis=1)
    errs = [ev]
    for flags in (0, FAST):
        got = planes_at(ctx, dev, coef, flags)
        errs.append(np.abs(got - want).max())
    # gain: log10 amplitudes within +-1
    ax = rng.normal(0, 1.0, (S, D))
    ay = rng.normal(0, 1.0, (S, D))
    ax /= max(1.0, np.abs(ax @ c.T).max())
    ay /= max(1.0, np.abs(ay @ c.T).max())
    a_x, a_y = 10 ** (ax @ c.T), 10 ** (ay @ c.T)
    wantg = np.stack([a_x * np.cos(v), a_x * np.sin(v), a_y * np.cos(v), a_y * np.sin(v)],
                     axis=1)
    for flags, tol in ((0, 1e-6), (FAST, 2e-6)):
        got = planes_at(ctx, dev, coef, flags, ax, ay)
        eg = (np.abs(got - wantg) / np.maximum(1.0, np.abs(wantg))).max()
        errs.append(eg)
        assert eg <= tol, (flags, eg)   # tests/test_gain.py's tolerances
    print(f"D={D} P={P} S={S}: values {errs[0]:.3g} planes {errs[1]:.3g} / "
          f"{errs[2]:.3g} (fast) gain {errs[3]:.3g} / {errs[4]:.3g} (fast)")
    assert errs[0] <= 1e-9
    assert errs[1] <= 1e-6 and errs[2] <= 1e-6


# 1: one live column; 15 | 16 | 17: the 16-point tile; 289: 19 tiles (a half
# pass at the end), the basis read through L2 at D = 20
@pytest.mark.parametrize("P", [1, 15, 16, 17, 289])
def test_point_counts(ctx, dev, P):
    check_against_numpy(ctx, dev, 20, P, 33, 100 + P)


def test_most_points(ctx, dev):
    check_against_numpy(ctx, dev, 20, 4096, 16, 4096)


# 15 | 16 | 17: the 16-slot group; 1000: 16 workgroup items, the last ragged
@pytest.mark.parametrize("S", [1, 15, 16, 17, 1000])
def test_slot_counts(ctx, dev, S):
    check_against_numpy(ctx, dev, 20, 20, S, 200 + S)


# 1 | 7: one and two k-steps (a padded one); 60 | 61 | 64 | 65: the k-step and
# k-step-pair boundaries round the lane-per-direction limit; 128: the most,
# its basis read through L2
@pytest.mark.parametrize("D", [1, 7, 60, 61, 64, 65, 128])
def test_direction_counts(ctx, dev, D):
    check_against_numpy(ctx, dev, D, 33, 33, 300 + D)


def test_nan_slot(ctx, dev):
    pp, xy, rng = synth_geometry(20, 20, 77)
    ctx.set_piercepoints(pp)
    ctx.set_points(xy)
    S, bad = 40, 21
    coef = rng.normal(0, 0.01, (S, 20))
    clean = coef.copy()
    coef[bad, 7] = np.nan
    keep = np.arange(S) != bad
    for flags in (0, FAST):
        ref = planes_at(ctx, dev, clean, flags)
        raw = planes_at(ctx, dev, coef, flags)
        assert np.all(np.isnan(raw[bad]))
        np.testing.assert_array_equal(raw[keep].view(np.uint32), ref[keep].view(np.uint32))
        scr = planes_at(ctx, dev, coef, flags | SCRUB)
        assert np.all(scr[bad, 0::2] == 1.0) and np.all(scr[bad, 1::2] == 0.0)
        np.testing.assert_array_equal(scr[keep].view(np.uint32), ref[keep].view(np.uint32))
    ref = values_at(ctx, dev, clean)
    got = values_at(ctx, dev, coef)
    assert np.all(np.isnan(got[bad]))
    np.testing.assert_array_equal(got[keep].view(np.uint64), ref[keep].view(np.uint64))


@pytest.mark.parametrize("P", [17, 20])
def test_output_offset_by_one_element(ctx, dev, P):
    """A planes pointer that is only 4-byte aligned, a values pointer that is
    only 8-byte aligned: the same numbers."""
    pp, xy, rng = synth_geometry(20, P, 55 + P)
    ctx.set_piercepoints(pp)
    ctx.set_points(xy)
    coef = rng.normal(0, 0.01, (35, 20))
    ax, ay = rng.normal(0, 1e-3, (35, 20)), rng.normal(0, 1e-3, (35, 20))
    for flags in (0, FAST):
        a = planes_at(ctx, dev, coef, flags)
        for off in (1, 2, 3):
            b = planes_at(ctx, dev, coef, flags, offset=off)
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        ga = planes_at(ctx, dev, coef, flags, ax, ay)
        gb = planes_at(ctx, dev, coef, flags, ax, ay, offset=1)
        np.testing.assert_array_equal(ga.view(np.uint32), gb.view(np.uint32))
    va = values_at(ctx, dev, coef)
    vb = values_at(ctx, dev, coef, offset=1)
    np.testing.assert_array_equal(va.view(np.uint64), vb.view(np.uint64))


# --------------------------------------------------------------- 7. contract

def test_contract(dev):
    from ska_sdp_screen_fitting_amd._lib import Context, ScreenFitError
    c = Context(0)
    try:
        c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        xy = np.zeros((3, 2))
        with pytest.raises(ScreenFitError, match=r"\(-22\)"):
            c.set_points(xy)                      # no geometry yet
        g = load_golden("synth12tiny")
        c.set_basis(g["piercepoints"])
        coef = up(dev, g["coef"].reshape(-1, 12)[:4])
        planes = torch.full((4, 4, 3), SENT, dtype=torch.float32, device=dev)
        values = torch.full((4, 3), SENT, dtype=torch.float64, device=dev)
        c.points = 3  # the binding's operand check; the library has no points
        with pytest.raises(ScreenFitError, match=r"\(-22\)"):
            c.eval_points(coef, 4, planes)
        with pytest.raises(ScreenFitError, match=r"\(-22\)"):
            c.eval_point_values(coef, 4, values)
        for bad in (np.zeros((0, 2)), np.zeros((4097, 2))):
            with pytest.raises(ScreenFitError, match=r"\(-22\)"):
                c.set_points(bad)
        with pytest.raises(ScreenFitError, match=r"\(-22\)"):
            c.set_points(np.array([[0.0, np.nan]]))
        c.set_points(xy)
        c.eval_points(coef, 4, planes, flags=FAST)
        with pytest.raises(ScreenFitError, match=r"\(-22\)"):
            c.eval_points(coef, 4, planes, flags=FAST | BE)
        with pytest.raises(ScreenFitError, match=r"\(-22\)"):
            c.eval_points(coef, 4, planes, coef_xx=coef)   # one amplitude set
        # a new geometry drops the points, as it drops the grid
        c.set_basis(g["piercepoints"])
        assert c.points == 0
        c.points = 3
        with pytest.raises(ScreenFitError, match=r"\(-22\)"):
            c.eval_points(coef, 4, planes)
        torch.cuda.synchronize()
    finally:
        c.close()


# ------------------------------------------------------- 8. public interface

@pytest.fixture(scope="module")
def fitted(dev):
    """KLScreen on the reference's fixture, fitted (as
    tests/test_gpu_parity.py::test_make_aterm_image_fixture_kl builds it)."""
    from ska_sdp_screen_fitting_amd.kl_screen import KLScreen
    scr = KLScreen("kl", os.path.join(GOLDEN, "fixture_kl.npz"),
                   os.path.join(GOLDEN, "skymodel.txt"), FIELD["rad"], FIELD["dec"],
                   FIELD["width"], FIELD["width"], solset_name="sol000",
                   phase_soltab_name="phase000")
    scr.process(ncpu=0)
    src = np.asarray(scr.source_positions, np.float32)
    return scr, np.rad2deg(src[:, 0]), np.rad2deg(src[:, 1])


def test_sample_is_the_cube_entry(fitted):
    from ska_sdp_screen_fitting_amd import geometry
    scr, ra, de = fitted
    ix, iy, inside = geometry.patch_pixels(ra, de, scr.rad, scr.dec, scr.width_ra, 0.2)
    assert inside.all()
    s = scr.sample(ra, de, cellsize_deg=0.2)
    T, F, A, D = np.shape(scr.vals_ph)
    assert s.shape == (T, F, A, 4, D) and s.dtype == np.float64
    for f, a in ((0, 1), (5, 30), (11, 61)):
        m = scr.make_matrix(0, T, f, a, 0.2, None, 1)      # [T][4][17][17]
        err = np.abs(s[:, f, a] - m[:, :, iy, ix]).max()
        print(f"freq {f} station {a}: |sample - cube| = {err:.3g}")
        assert err <= 1e-6
    # a sub-range of times, one position off the field
    s2 = scr.sample(np.append(ra, scr.rad), np.append(de, scr.dec + 3.0),
                    cellsize_deg=0.2, t_start=3, t_stop=9)
    assert s2.shape == (6, F, A, 4, D + 1)
    np.testing.assert_array_equal(s2[..., :D], s[3:9])
    assert np.all(np.isnan(s2[..., D]))
    # a 1 MiB batch budget: many batches, the same arrays
    s3 = scr.sample(ra, de, cellsize_deg=0.2, max_batch_bytes=1 << 20)
    np.testing.assert_array_equal(s3, s)


def test_patch_errors_meet_the_reference_criterion(fitted):
    from ska_sdp_screen_fitting_amd import geometry
    scr, ra, de = fitted
    err = scr.patch_errors(0.2)
    T, F, A, D = np.shape(scr.vals_ph)
    assert err.shape == (D,) and err.dtype == np.float64
    # restated from make_matrix: the cube entry at each direction's pixel
    ix, iy, _ = geometry.patch_pixels(ra, de, scr.rad, scr.dec, scr.width_ra, 0.2)
    st = scr.solset.get_soltab("phase000")
    val, wgt = np.asarray(st.val), np.asarray(st.weight)
    phi = val - val[:, :, scr.ref_ind:scr.ref_ind + 1, :]
    use = (wgt != 0) & np.isfinite(val)
    # every slot's cube in one launch: eval_host is what make_matrix calls per
    # (freq, station), with make_matrix's flags (raw planes, fast sincos)
    cube = scr.evaluator(0.2).eval_host(np.asarray(scr.vals_ph), flags=FAST)
    m = cube[..., iy, ix].astype(np.float64)                # [T][F][A][4][D]
    one = scr.make_matrix(0, T, 3, 17, 0.2, None, 1)[:, :, iy, ix]
    np.testing.assert_array_equal(m[:, 3, 17], one)
    want = np.zeros(D)
    for q, fn in enumerate((np.cos, np.sin, np.cos, np.sin)):
        d = np.where(use, np.abs(m[:, :, :, q] - fn(phi)), 0.0)
        want = np.maximum(want, d.reshape(-1, D).max(axis=0))
    print("patch_errors(0.2):", np.round(err, 4), "restated:", np.round(want, 4))
    np.testing.assert_allclose(err, want, rtol=0, atol=1e-6)
    assert np.all(err < 0.1)   # the reference's test_fit_kl_screens threshold
    np.testing.assert_array_equal(scr.patch_errors(0.2, max_batch_bytes=1 << 20), err)
    # at the exact positions the screen is the fit's model: errors of the size
    # of the fit residuals, every direction finite
    exact = scr.patch_errors()
    assert exact.shape == (D,) and np.all(np.isfinite(exact))


def test_sample_values_are_the_fit_model(fitted):
    scr, ra, de = fitted
    v = scr.sample(ra, de, values=True)
    T, F, A, D = np.shape(scr.vals_ph)
    assert v.shape == (T, F, A, D) and v.dtype == np.float64
    st = scr.solset.get_soltab("phase000")
    resid = np.asarray(scr.solset.get_soltab("phase_screen000resid").val)
    val = np.asarray(st.val)
    want = (val - val[:, :, scr.ref_ind:scr.ref_ind + 1, :]) - resid
    use = identity_slots(np.asarray(scr.vals_ph), scr.ref_ind)
    err = np.abs(v - want)[use].max()
    print(f"{use.sum()} slots: max |sample(values) - (input - ref - resid)| = {err:.3g}")
    assert err <= 1e-9
    np.testing.assert_array_equal(
        scr.sample(ra, de, values=True, max_batch_bytes=1 << 20), v)


def test_gain_screen_sample_and_patch_errors(dev):
    """Gain screens (phase + XX / YY amplitudes) through the public
    interface: ``sample`` is the gain cube's entry (tests/test_gain.py's
    2e-6 max(1, |ref|) on the fast epilogue), ``patch_errors`` its numpy
    restatement with the input amplitudes gathered onto the phase grid
    (oracle ``interpolate_nearest``)."""
    from oracle import kl as okl
    from ska_sdp_screen_fitting_amd import geometry
    from ska_sdp_screen_fitting_amd.kl_screen import KLScreen
    g = load_golden("gain12")
    scr = KLScreen("gain", os.path.join(GOLDEN, "gain12.npz"), None, FIELD["rad"],
                   FIELD["dec"], FIELD["width"], FIELD["width"], solset_name="sol000",
                   phase_soltab_name="phase000", amplitude_soltab_name="amplitude000")
    scr.process(ncpu=0)
    src = np.asarray(scr.source_positions, np.float32)
    ra, de = np.rad2deg(src[:, 0]), np.rad2deg(src[:, 1])
    ix, iy, inside = geometry.patch_pixels(ra, de, scr.rad, scr.dec, scr.width_ra, 0.2)
    T, F, A, D = np.shape(scr.vals_ph)
    s = scr.sample(ra, de, cellsize_deg=0.2)
    assert s.shape == (T, F, A, 4, D)
    cube = np.stack([np.stack([scr.make_matrix(0, T, f, a, 0.2, None, 1)
                               for a in range(A)], axis=1) for f in range(F)], axis=1)
    m = cube[..., iy, ix]                                   # [T][F][A][4][D]
    ok = inside & np.ones_like(m, bool)
    both = ok & ~np.isnan(m)
    np.testing.assert_array_equal(np.isnan(s)[ok], np.isnan(m)[ok])
    err = (np.abs(s - m)[both] / np.maximum(1.0, np.abs(m[both]))).max()
    print(f"gain sample vs cube: {err:.3g}; inside {inside.sum()} of {D}")
    assert err <= 2e-6
    assert np.all(np.isnan(s[..., ~inside]))
    # patch_errors restated
    val, wgt = np.asarray(g["val"]), np.asarray(g["weight"])
    grid = (g["amp_times"], g["amp_freqs"], g["times"], g["freqs"])
    aval = okl.interpolate_nearest(g["amp_val"], *grid)
    awgt = okl.interpolate_nearest(g["amp_weight"], *grid)
    phi = val - val[:, :, scr.ref_ind:scr.ref_ind + 1, :]
    use = ((wgt != 0) & np.isfinite(val) & (awgt[..., 0] != 0) & (awgt[..., 1] != 0)
           & np.isfinite(aval[..., 0]) & np.isfinite(aval[..., 1]))
    want = np.full(D, -np.inf)
    for q, (amp, fn) in enumerate(((aval[..., 0], np.cos), (aval[..., 0], np.sin),
                                   (aval[..., 1], np.cos), (aval[..., 1], np.sin))):
        d = np.where(use, np.abs(m[:, :, :, q] - amp * fn(phi)), -np.inf)
        want = np.maximum(want, d.reshape(-1, D).max(axis=0))
    want[~inside | ~np.isfinite(want)] = np.nan
    got = scr.patch_errors(0.2)
    print("gain patch_errors(0.2):", np.round(got, 4))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    assert fin.any()
    np.testing.assert_allclose(got[fin], want[fin], rtol=0,
                               atol=2e-6 * max(1.0, float(np.nanmax(np.abs(m)))))
