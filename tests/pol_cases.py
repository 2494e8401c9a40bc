"""Inputs shared by the polarized-phase tests (test_pol_cpu.py,
test_pol_screens.py): tables with a ``pol`` axis, written as ``.npz`` and
``.h5``, their XX-only / YY-only scalar tables, and a sky model."""

import numpy as np

from oracle import kl as okl

NPZ_KEYS = ("val", "weight", "times", "freqs", "dir_names", "ant_names",
            "dir_radec", "ant_pos")
AMP_KEYS = ("amp_val", "amp_weight", "amp_times", "amp_freqs", "amp_pol")


def write_npz(path, g, pols=None, **extra):
    """The table ``g`` as an ``.npz`` solution file; ``pols``: an index or a
    list into the pol axis (an index gives the scalar table of that pol)."""
    d = {k: g[k] for k in NPZ_KEYS + AMP_KEYS if k in g}
    if pols is not None:
        d["val"], d["weight"] = g["val"][..., pols], g["weight"][..., pols]
    d.update(extra)
    np.savez(path, **d)
    return str(path)


def write_h5(path, g, pols=None):
    """The same table as an H5parm file (phase000 with its pol axis, and
    amplitude000 when the table has amplitudes)."""
    from ska_sdp_screen_fitting_amd.h5parm import Solset, Soltab, write_h5parm
    names = [str(n) for n in g["ant_names"]], [str(n) for n in g["dir_names"]]
    ss = Solset("sol000", names[0], g["ant_pos"], names[1], g["dir_radec"])
    val, weight = g["val"], g["weight"]
    if pols is not None:
        val, weight = val[..., pols], weight[..., pols]
    axes = ["time", "freq", "ant", "dir"]
    avals = [g["times"], g["freqs"], np.array(names[0]), np.array(names[1])]
    pol = np.array(["XX", "YY"])
    ss.soltabs["phase000"] = Soltab(
        "phase000", "phase", axes + (["pol"] if val.ndim == 5 else []),
        avals + ([pol] if val.ndim == 5 else []), val, weight, solset=ss)
    if "amp_val" in g:
        ss.soltabs["amplitude000"] = Soltab(
            "amplitude000", "amplitude", axes + ["pol"],
            [g["amp_times"], g["amp_freqs"], avals[2], avals[3], pol],
            g["amp_val"], g["amp_weight"], solset=ss)
    write_h5parm(str(path), [ss])
    return str(path)


def write_skymodel(path, dir_names, dir_radec):
    """makesourcedb patch lines for the directions (RA hh:mm:ss, Dec dd.mm.ss)."""
    def sexa(v, sep):
        d = int(v)
        m = int((v - d) * 60)
        sec = ((v - d) * 60 - m) * 60
        return f"{d}{sep}{m:02d}{sep}{sec:09.6f}"

    with open(path, "w", encoding="utf8") as fh:
        fh.write("FORMAT = Name, Type, Patch, Ra, Dec, I\n\n")
        for name, (ra, dec) in zip(dir_names, np.rad2deg(np.asarray(dir_radec, np.float64))):
            fh.write(f" , , {str(name).strip('[]')}, {sexa(ra / 15.0, ':')}, {sexa(dec, '.')}\n")
    return str(path)


def add_amplitudes(g, seed=5):
    """XX / YY amplitudes on a coarser grid (synthetic.make_amplitudes)."""
    from ska_sdp_screen_fitting_amd.synthetic import SolutionSet, make_amplitudes
    s = SolutionSet(val=g["val"][..., 0], weight=g["weight"][..., 0], times=g["times"],
                    freqs=g["freqs"], ant_names=list(g["ant_names"]), ant_pos=g["ant_pos"],
                    dir_names=list(g["dir_names"]), dir_radec=g["dir_radec"])
    make_amplitudes(s, n_time=2, n_freq=1, seed=seed, flag_frac=0.02, outlier_frac=0.0)
    g = dict(g)
    g.update(amp_val=s.amp_val, amp_weight=s.meta["amp_weight"],
             amp_times=s.meta["amp_times"], amp_freqs=s.meta["amp_freqs"],
             amp_pol=np.array(["XX", "YY"]))
    return g


def table(sol_xx, val_yy, weight_yy):
    """A polarized table on the geometry of ``sol_xx`` (a SolutionSet).  Station
    0 carries no flags, so it is the reference station of the polarized table
    and of either pol's scalar table alike (get_reference_station: the first
    station with the largest summed weight)."""
    val = np.stack([sol_xx.val, val_yy], axis=-1)
    weight = np.stack([sol_xx.weight, weight_yy], axis=-1).astype(np.float32)
    weight[:, :, 0] = 1.0
    return dict(val=val, weight=weight, times=sol_xx.times, freqs=sol_xx.freqs,
                dir_names=np.array(sol_xx.dir_names), ant_names=np.array(sol_xx.ant_names),
                dir_radec=sol_xx.dir_radec, ant_pos=sol_xx.ant_pos)


def golden_table(g):
    """The pol12 inputs (tests/golden/pol12.npz), station 0 unflagged."""
    t = {k: g[k] for k in NPZ_KEYS}
    t["weight"] = t["weight"].copy()
    t["weight"][:, :, 0] = 1.0
    return t


def smooth_table(n_dir=7, seed=77):
    """A fixture-shaped polarized table (7 directions) whose phases a KL screen
    of the fit's order can follow: per slot and pol a random combination of
    the first three KL modes of the geometry (0.25 rad rms each) plus 0.003 rad
    of noise, 3 % of the entries flagged, differently per pol."""
    from ska_sdp_screen_fitting_amd import geometry
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    s = make_solutions(n_ant=5, n_time=6, n_freq=2, n_dir=n_dir, seed=seed,
                       flag_frac=0.03, outlier_frac=0.0)
    pp = geometry.piercepoints(s.dir_radec)[0]
    u = okl.Basis(pp).u[:, :3]
    rng = np.random.default_rng(seed + 1)
    shape = s.val.shape
    vals = [rng.normal(0, 0.25, shape[:3] + (3,)) @ u.T + rng.normal(0, 0.003, shape)
            for _ in range(2)]
    s.val = vals[0]
    return table(s, vals[1], s.weight[::-1])


def oracle_patch_errors(g, cellsize_deg, rad, dec, width):
    """KLScreen.patch_errors of the table from the oracle's fit: per pol the
    largest |cos / sin of the fitted screen at a direction's position (or, with
    ``cellsize_deg``, at its pixel) - cos / sin of the referenced input phase|
    over the unflagged entries."""
    from ska_sdp_screen_fitting_amd import geometry
    pp, mra, mdec = geometry.piercepoints(g["dir_radec"])
    D = len(pp)
    ref = okl.reference_station(g["weight"].sum(-1))
    src = np.asarray(g["dir_radec"], np.float32)
    ra, de = np.rad2deg(src[:, 0]), np.rad2deg(src[:, 1])
    if cellsize_deg is None:
        x, y = geometry.screen_xy(ra, de, mra, mdec)
    else:
        ix, iy, inside = geometry.patch_pixels(ra, de, rad, dec, width, cellsize_deg)
        assert inside.all()
        gx, gy = geometry.grid_coords(rad, dec, width, cellsize_deg, mra, mdec)
        x, y = gx[ix], gy[iy]
    cp = np.stack([okl.cpix_matrix(pp, [x[k]], [y[k]])[0] for k in range(D)])
    worst = []
    for p in (0, 1):
        val, wt = g["val"][..., p], g["weight"][..., p]
        r = okl.run_soltab(val, wt, g["ant_pos"], pp, ref, min(20, D - 1), "phase")
        scr = r["coef"] @ cp.T
        phi = val - val[:, :, ref:ref + 1]
        e = np.maximum(np.abs(np.cos(scr) - np.cos(phi)), np.abs(np.sin(scr) - np.sin(phi)))
        worst.append(float(np.where(wt != 0, e, 0.0).max()))
    return worst
