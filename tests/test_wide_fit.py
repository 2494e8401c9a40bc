"""The KL fit with 61..128 directions: sf_set_basis_wide (SF_MAX_FIT_DIR = 128)
and sf_kl_fit on a wide-basis context (csrc/kl_fit_wide.hip: one workgroup
per slot, workgroup Jacobi; stationscreen.py:390-430, 433-594, 597-782).

Checked against the reference's own fits at D = 80 / 128
(tests/golden/make_golden_wide_fit.py, wide80.npz) and against the oracle,
at the project's tolerances (tests/test_gpu_parity.py): coefficients
|d| <= 1e-8 x max(1, |coef|max), residuals 1e-8, orders and flagged weights
bit-equal; basis as test_basis_vs_oracle; evaluated planes 2e-6.
Needs an MI355X: every test is marked ``gpu``.
"""

import numpy as np
import pytest

from conftest import FIELD, load_golden
from oracle import geometry as og
from oracle import kl as okl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PHASE, TEC, AMPLITUDE = 0, 1, 2
WIDE_D = [61, 64, 65, 96, 127, 128]


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


def synth(D, **kw):
    from ska_sdp_screen_fitting_amd import geometry
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    args = dict(n_ant=3, n_time=4, n_freq=1, n_dir=D, seed=1000 + D,
                flag_frac=0.02, outlier_frac=0.005)
    args.update(kw)
    s = make_solutions(**args)
    pp, _, _ = geometry.piercepoints(s.dir_radec)
    return s, pp


def wide_fit(ctx, dev, val, weight, pp, st, ref, screen_type=PHASE, niter=2,
             bind=True, outputs=True, **kw):
    """sf_set_basis_wide + sf_kl_fit -> host (coef, resid, w_out, orders)."""
    if bind:
        ctx.set_basis_wide(pp)
    T, F, A, D = val.shape
    ph = torch.from_numpy(np.ascontiguousarray(val, np.float64)).to(dev)
    wt = torch.from_numpy(np.ascontiguousarray(weight, np.float32)).to(dev)
    coef = torch.full_like(ph, -7.0)
    if not outputs:
        ctx.fit(ph, wt, T, F, A, st, screen_type=screen_type, niter=niter,
                ref_ant=ref, coef=coef, **kw)
        torch.cuda.synchronize()
        return coef.cpu().numpy()
    resid = torch.full_like(ph, -7.0)
    w_out = torch.full_like(wt, -7.0)
    order = torch.full((T, F, A), -7, dtype=torch.int32, device=dev)
    ctx.fit(ph, wt, T, F, A, st, screen_type=screen_type, niter=niter,
            ref_ant=ref, coef=coef, resid=resid, w_out=w_out, order_out=order,
            **kw)
    torch.cuda.synchronize()
    return (coef.cpu().numpy(), resid.cpu().numpy(), w_out.cpu().numpy(),
            order.cpu().numpy())


def check(got, coef, resid, w_out, orders, what=""):
    g_coef, g_resid, g_w, g_ord = got
    cerr = np.abs(g_coef - coef).max()
    rerr = np.abs(g_resid - resid).max()
    scale = max(1.0, np.abs(coef).max())
    print(f"{what}: coef err {cerr:.3g} resid err {rerr:.3g} scale {scale:.3g} "
          f"orders {np.unique(orders).tolist()}")
    np.testing.assert_array_equal(g_ord, orders)
    np.testing.assert_array_equal(g_w, w_out)
    assert cerr <= 1e-8 * scale
    assert rerr <= 1e-8


def phase_orders(s, ref, order=20):
    from ska_sdp_screen_fitting_amd.stationscreen import station_orders
    return station_orders(s.ant_pos if hasattr(s, "ant_pos") else s["ant_pos"],
                          ref, order)


# ------------------------------------------------------------------ 1. basis

@pytest.mark.parametrize("D", WIDE_D)
def test_wide_basis_vs_oracle(ctx, D):
    _, pp = synth(D)
    c0, pinv0, u0 = okl.calculate_svd(pp, 100.0, 5.0 / 3.0)
    ctx.set_basis_wide(pp)
    c, pinv, u, eig = ctx.get_basis()
    sv = np.linalg.svd(c0, compute_uv=False)
    cond = sv.max() / sv[sv > 1e-3].min()
    print(f"D={D} |pinv err| {np.abs(pinv - pinv0).max():.3g} allowed "
          f"{1e-13 * cond * np.abs(pinv0).max():.3g} |eig err| "
          f"{np.abs(np.abs(eig) - sv).max():.3g} |uTU-I| "
          f"{np.abs(np.abs(u.T @ u0) - np.eye(D)).max():.3g}")
    np.testing.assert_allclose(c, c0, rtol=1e-13, atol=0)
    np.testing.assert_allclose(pinv, pinv0, rtol=0,
                               atol=1e-13 * cond * np.abs(pinv0).max())
    np.testing.assert_allclose(np.abs(eig), sv, rtol=1e-12, atol=1e-12 * sv.max())
    np.testing.assert_allclose(np.abs(u.T @ u0), np.eye(D), atol=1e-9)


def test_wide_basis_below_limit_is_set_basis(ctx):
    _, pp = synth(20)
    ctx.set_basis(pp)
    a = ctx.get_basis()
    ctx.set_basis_wide(pp)
    b = ctx.get_basis()
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


# --------------------------------------------------- 2. the reference's fits

@pytest.mark.parametrize("name", ["wide80", "wide_fit80", "wide_fit128"])
def test_wide_fit_vs_reference_golden(ctx, dev, name):
    g = load_golden(name)
    ref = int(g["ref_ant"])
    st = phase_orders(g, ref, int(g["order"]))
    got = wide_fit(ctx, dev, g["val"], g["weight"], g["piercepoints"], st, ref)
    check(got, g["coef"], g["resid"], g["w_out"], g["orders"], name)


@pytest.mark.parametrize("case", ["noref", "ref"])
def test_wide_tec_fit_vs_reference_golden(ctx, dev, case):
    g = load_golden("wide_fit80tec")
    ref = int(g[f"{case}_ref_ant"])
    st = phase_orders(g, ref, int(g["order"]))
    got = wide_fit(ctx, dev, g["val"], g["weight"], g["piercepoints"], st, ref,
                   screen_type=TEC, niter=int(g["niter"]))
    check(got, g[f"{case}_coef"], g[f"{case}_resid"], g[f"{case}_w_out"],
          g[f"{case}_orders"], "tec " + case)


def stack_pols(a):
    """[T, F, A, D, P] -> [T, F, P * A, D], as stationscreen.run stacks the
    pols of an amplitude soltab into one fit."""
    return np.concatenate([a[..., p] for p in range(a.shape[-1])], axis=2)


def unstack_pols(a, P):
    A = a.shape[2] // P
    return np.stack([a[:, :, p * A:(p + 1) * A] for p in range(P)], axis=-1)


def test_wide_amplitude_fit_vs_reference_golden(ctx, dev):
    g = load_golden("wide_fit80amp")
    P = g["amp_val"].shape[-1]
    A = g["amp_val"].shape[2]
    got = wide_fit(ctx, dev, stack_pols(g["amp_val"]), stack_pols(g["amp_weight"]),
                   g["piercepoints"], [int(g["amp_order"])] * (A * P), -1,
                   screen_type=AMPLITUDE, niter=int(g["niter"]))
    got = tuple(unstack_pols(x, P) for x in got)
    check(got, g["amp_coef"], g["amp_resid"], g["amp_w_out"], g["amp_orders"],
          "amplitude")


# ------------------------------------------------------- 3. phase vs oracle

def phase_vs_oracle(ctx, dev, s, pp, what):
    ref = okl.reference_station(s.weight)
    r = okl.run_phase(s.val, s.weight, s.ant_pos, pp, ref, 20)
    got = wide_fit(ctx, dev, s.val, s.weight, pp, phase_orders(s, ref), ref)
    check(got, r["coef"], r["resid"], r["w_out"], r["orders"], what)
    return r


@pytest.mark.parametrize("D", WIDE_D)
def test_wide_phase_fit_vs_oracle(ctx, dev, D):
    """61 / 64 / 65: across the wave boundary; odd and even n; 127 / 128: the
    workgroup full."""
    s, pp = synth(D)
    phase_vs_oracle(ctx, dev, s, pp, f"D={D}")


def test_wide_phase_fit_heavy_flags(ctx, dev):
    """40 % flags: subsets of 40..55 directions, adapted orders."""
    s, pp = synth(80, flag_frac=0.4, outlier_frac=0.02, seed=4080, n_freq=2)
    r = phase_vs_oracle(ctx, dev, s, pp, "D=80 40% flags")
    n = (r["w_out"] > 0).sum(-1)
    assert n[n > 0].min() >= 40 and n.max() <= 55
    assert len(np.unique(r["orders"])) >= 3
    st = ctx.fit_stats()
    assert st["n_general"] == 0 and st["n_masks"] > 0


def test_wide_phase_fit_tiny_weights(ctx, dev):
    """Weights of 5e-4, below the pinv cutoff: the truncated eigen-solve of
    U_k^T W U_k."""
    s, pp = synth(96, flag_frac=0.05, tiny_weight_frac=0.1, seed=4096)
    assert (s.weight == np.float32(5e-4)).sum() > 50
    phase_vs_oracle(ctx, dev, s, pp, "D=96 tiny weights")


# ------------------------------------------------------------ 4. crafted slots

def test_wide_fit_crafted_subsets(ctx, dev):
    """Two, one and no unflagged direction, a skipped (all-NaN) station and
    the reference station, at D = 65."""
    s, pp = synth(65, seed=4065, n_ant=4, n_time=3, outlier_frac=0.0)
    val, w = s.val.copy(), s.weight.copy()

    def only(t, a, keep):
        w[t, 0, a, :] = 0.0
        w[t, 0, a, np.array(keep, dtype=int)] = 1.0
    only(0, 1, [3, 40])
    only(0, 2, [63, 64])
    only(1, 1, [64])
    only(2, 1, [])
    val[:, :, 3, :] = np.nan
    # the oracle's U of a two-direction subset is an exact signed permutation
    # (no LAPACK rounding residue enters its order-1 fit)
    for pair in ([3, 40], [63, 64]):
        c2, _, u2 = okl.calculate_svd(pp[pair], 100.0, 5.0 / 3.0)
        assert c2[0, 0] == 0.0 and c2[1, 1] == 0.0
        assert np.array_equal(np.abs(u2), np.array([[0.0, 1.0], [1.0, 0.0]]))
    r = okl.run_phase(val, w, s.ant_pos, pp, 0, 20)
    assert r["orders"][0, 0, 1] == 1 and r["orders"][0, 0, 2] == 1
    assert r["orders"][1, 0, 1] == 0 and not r["coef"][1, 0, 1].any()
    got = wide_fit(ctx, dev, val, w, pp, phase_orders(s, 0), 0)
    check(got, r["coef"], r["resid"], r["w_out"], r["orders"], "crafted D=65")
    coef, resid, _, orders = got
    # the empty slot keeps its station's order (no fit ran: the oracle too);
    # skipped blocks and the reference station are all zeros
    assert not coef[2, 0, 1].any()
    for t, a in ((0, 3), (1, 3), (2, 3), (0, 0)):
        assert not coef[t, 0, a].any() and orders[t, 0, a] == 0, (t, a)
    assert not resid[:, 0, 3].any() and not resid[:, 0, 0].any()


# ------------------------------------------------- 5. tec, amplitude vs oracle

@pytest.mark.parametrize("D", [80, 128])
def test_wide_tec_fit_vs_oracle(ctx, dev, D):
    s, pp = synth(D, n_freq=2)
    ref = okl.reference_station(s.weight)
    r = okl.run_soltab(s.val, s.weight, s.ant_pos, pp, ref, 20, "tec", niter=2)
    got = wide_fit(ctx, dev, s.val, s.weight, pp, phase_orders(s, ref), ref,
                   screen_type=TEC, niter=2)
    check(got, r["coef"], r["resid"], r["w_out"], r["orders"], f"tec D={D}")


@pytest.mark.parametrize("D", [80, 128])
def test_wide_amplitude_fit_vs_oracle(ctx, dev, D):
    """Both pols stacked along the station axis in one call, as
    stationscreen.run fits an amplitude soltab; niter 3, order 12."""
    from ska_sdp_screen_fitting_amd.synthetic import make_amplitudes
    s, pp = synth(D, n_freq=2)
    make_amplitudes(s, seed=2000 + D, flag_frac=0.02, outlier_frac=0.005)
    amp, wt = s.amp_val, s.meta["amp_weight"]
    r = okl.run_amplitude(amp, wt, pp, 12)
    P, A = amp.shape[-1], amp.shape[2]
    got = wide_fit(ctx, dev, stack_pols(amp), stack_pols(wt), pp, [12] * (A * P),
                   -1, screen_type=AMPLITUDE, niter=3)
    got = tuple(unstack_pols(x, P) for x in got)
    check(got, r["coef"], r["resid"], r["w_out"], r["orders"], f"amplitude D={D}")
    assert (r["w_out"] == 0).sum() > (wt == 0).sum()  # the block sigma flagged


# ------------------------------------------------------------------ 6. the ABI

def test_wide_fit_abi(ctx, dev):
    from ska_sdp_screen_fitting_amd._lib import SF_MAX_FIT_DIR, ScreenFitError
    s, pp = synth(80, n_ant=4)
    ref = okl.reference_station(s.weight)
    st = phase_orders(s, ref)
    full = wide_fit(ctx, dev, s.val, s.weight, pp, st, ref)
    # two calls give identical bytes
    again = wide_fit(ctx, dev, s.val, s.weight, pp, st, ref)
    for a, b in zip(full, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # NULL resid / w_out / order_out: the same coefficients
    lone = wide_fit(ctx, dev, s.val, s.weight, pp, st, ref, outputs=False)
    assert np.array_equal(lone.view(np.uint8), full[0].view(np.uint8))
    # two antenna shards with the reference phases passed in
    refph = torch.from_numpy(np.ascontiguousarray(s.val[:, :, ref, :])).to(dev)
    for a0, a1 in ((0, 2), (2, 4)):
        part = wide_fit(ctx, dev, s.val[:, :, a0:a1], s.weight[:, :, a0:a1], pp,
                        st[a0:a1], ref, bind=False, ant_offset=a0,
                        ref_phase=refph)
        for a, b in zip(part, full):
            assert np.array_equal(a.view(np.uint8),
                                  np.ascontiguousarray(b[:, :, a0:a1]).view(np.uint8))
    # no mask pool above 60 directions
    with pytest.raises(ScreenFitError):
        ctx.fit_pool()
    assert ctx.fit_stats()["n_general"] == 0
    # 129 directions are refused and the context stays usable
    big = np.random.default_rng(0).normal(0, 50.0, (SF_MAX_FIT_DIR + 1, 3))
    with pytest.raises(ScreenFitError):
        ctx.set_basis_wide(big)
    once_more = wide_fit(ctx, dev, s.val, s.weight, pp, st, ref)
    for a, b in zip(full, once_more):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_wide_basis_binds_the_evaluation_geometry(ctx, dev):
    """After set_basis_wide, set_grid + eval write the bytes they write after
    set_piercepoints (the wide evaluation kernel)."""
    from ska_sdp_screen_fitting_amd import geometry
    s, pp = synth(80)
    _, mra, mdec = geometry.piercepoints(s.dir_radec)
    x, y = geometry.grid_coords(FIELD["rad"], FIELD["dec"], FIELD["width"], 0.2,
                                mra, mdec)
    coef = np.random.default_rng(80).normal(0, 0.01, (19, 80))
    cd = torch.from_numpy(coef).to(dev)
    outs = []
    for setter in (ctx.set_piercepoints, ctx.set_basis_wide):
        setter(pp)
        ctx.set_grid(x, y)
        assert ctx.eval_kernel(1 | 1 << 8) == "kl_eval_wide_kernel"
        out = torch.full((19, 4, len(y), len(x)), -7.0, dtype=torch.float32,
                         device=dev)
        ctx.eval(cd, 19, out, flags=1 | 1 << 8)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32))


# ------------------------------------------------------------- 7. end to end

def test_make_aterm_image_80_directions_kl(tmp_path, dev):
    """stationscreen.run + KLScreen.fit + make_aterm_image(screen_type="kl")
    on a synthetic H5parm with 80 directions, vs the oracle's fit and
    evaluation."""
    from ska_sdp_screen_fitting_amd import fits as sffits
    from ska_sdp_screen_fitting_amd.h5parm import Solset, Soltab, write_h5parm
    from ska_sdp_screen_fitting_amd.make_aterm_images import make_aterm_image
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    s = make_solutions(n_ant=3, n_time=4, n_freq=2, n_dir=80, seed=81)
    ss = Solset("sol000", s.ant_names, s.ant_pos, s.dir_names, s.dir_radec)
    axes = ["time", "freq", "ant", "dir"]
    st = Soltab("phase000", "phase", axes,
                [s.times, s.freqs, np.array(s.ant_names), np.array(s.dir_names)],
                s.val, s.weight, solset=ss)
    ss.soltabs["phase000"] = st
    h5 = str(tmp_path / "wide.h5")
    write_h5parm(h5, [ss])
    outroot = str(tmp_path / "widekl")
    make_aterm_image(h5, soltabname="phase000", screen_type="kl",
                     outroot=outroot, bounds_deg=[124.565, 66.165, 127.895, 62.835],
                     bounds_mid_deg=[FIELD["rad"], FIELD["dec"]], skymodel=None,
                     solsetname="sol000", padding_fraction=0, cellsize_deg=0.2,
                     ncpu=0)
    _, cube = sffits.read_cube(outroot + "_0.fits")
    assert cube.shape == (4, 2, 3, 4, 17, 17)
    pp, mra, mdec = og.piercepoints(s.dir_radec)
    ref = okl.reference_station(s.weight)
    r = okl.run_phase(s.val, s.weight, s.ant_pos, pp, ref, 20)
    x, y = og.grid_coords(FIELD["rad"], FIELD["dec"], FIELD["width"], 0.2, mra, mdec)
    cpix = okl.cpix_matrix(pp, x, y)
    want = okl.eval_planes(okl.eval_phase_screens(r["coef"].reshape(-1, 80), cpix))
    err = np.abs(cube.reshape(want.shape) - want).max()
    print("80-direction KL cube vs oracle:", err)
    assert err <= 2e-6


def test_klscreen_planes_of_the_reference_fit_80_directions(dev):
    """The reference's fitted coefficients at D = 80 through KLScreen
    .make_matrix against its own planes (wide80.npz kl17)."""
    from ska_sdp_screen_fitting_amd.kl_screen import KLScreen
    g = load_golden("wide80")
    scr = KLScreen("wide80", None, None, FIELD["rad"], FIELD["dec"],
                   FIELD["width"], FIELD["width"])
    scr.vals_ph = g["coef"]
    scr.piercepoints = g["piercepoints"]
    scr.r_0, scr.beta_val = float(g["r_0"]), float(g["beta"])
    scr.mid_ra, scr.mid_dec = float(g["mid_ra"]), float(g["mid_dec"])
    T = g["coef"].shape[0]
    for k, (f, a) in enumerate(g["pairs17"]):
        got = scr.make_matrix(0, T, int(f), int(a), 0.2, None, 1)
        ref = g["kl17"][k]                    # [T][2][17][17]
        for p in range(4):
            assert np.abs(got[:, p] - ref[:, p % 2]).max() <= 2e-6
