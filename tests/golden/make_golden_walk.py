#!/opt/conda/bin/python3.9
"""Golden vectors for the order walk of ``adjust_order`` and for fit
parameters off their defaults, produced by running the reference's own
``stationscreen.run`` (the interpreter, shims and duck-typed soltabs of
make_golden.py) -- data only.

With the weights of ``make_solutions`` (0, 5e-4, 1) and its 0.05 rad noise
the reduced chi^2 of a fit is ~ 0.003: the first step of the walk
(stationscreen.py:700-782) lands on the order it started from and no slot is
ever re-fitted.  Weights like an H5parm's 1 / sigma^2 (x 400 for sigma =
0.05) put the reduced chi^2 near 1, and the walk moves the order of about
half of the slots: re-fits, sign flips and the double-bound stop.

Every case is ``make_solutions(seed=7, flag_frac=0.02, outlier_frac=0.02)``;
the weights are scaled here.  A file holds the inputs (``val``, ``weight``,
``ant_pos``, ``dir_radec``, ``piercepoints``, ``order``, ``beta``, ``r_0``),
the names of its groups (``groups``; a group is one soltab: its
``<group>_type``, ``<group>_ref_ant`` and, where they differ from the file's,
``<group>_val`` / ``<group>_weight``) and per group and parameter set k
``<group>_s<k>_niter / _nsigma / _adjust_order / _coef / _resid / _w_out /
_orders`` (``<group>_nsets`` sets).

* walk20       phase, 5 x 8 x 2, D = 20, order 12, weights x 400
* walk20mixed  the same with x {100, 400, 1600} per entry and 1 % of the
               entries at 5e-4 (below the pinv cutoff: the general path)
* walk20beta   walk20 at beta = 1.0 (r_0 is fixed at 100 in the reference,
               stationscreen.py:1046)
* cascade12    phase, 5 x 8 x 2, D = 12, order 11, weights 1, nsigma 1.5 and
               8 passes: outlier flags of later passes take slots down to 3,
               2, 1 and 0 unflagged directions
* walk50       phase, 4 x 6 x 1, D = 50, order 20, x 400
* walk14tec    tec, 4 x 6 x 2, D = 14, order 10, x 400, ref_ant 2 and -1
               (quirk Q15) as tec14; the values are the phase values
               themselves (noise 0.05, so that x 400 is 1 / sigma^2)
* walk14amp    amplitude, 4 x 6 x 2, D = 14, pols 10^(0.1 val) and
               10^(0.07 val), order 6, as KLScreen.fit calls it, x 4e4
               (1 / sigma^2 of the 0.005 log10 noise)
* walk80       phase and tec, 3 x 4 x 1, D = 80, order 20, x 400

Usage:  timeout 1200 /opt/conda/bin/python3.9 tests/golden/make_golden_walk.py [name ...]
(under ``timeout``: a slot that the flags leave with one unflagged direction
kills the reference's worker, and the run then hangs)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (applies the shims)

import numpy as np  # noqa: E402

from make_golden_gain import AmpSoltab  # noqa: E402
from make_golden_tec import TecSoltab  # noqa: E402
from ska_sdp_screen_fitting import stationscreen  # noqa: E402
from ska_sdp_screen_fitting_amd.synthetic import make_solutions  # noqa: E402

SEED = 7
T, F = True, False


def solutions(n_ant, n_time, n_freq, n_dir, scale=1.0):
    s = make_solutions(n_ant=n_ant, n_time=n_time, n_freq=n_freq, n_dir=n_dir,
                       seed=SEED, flag_frac=0.02, outlier_frac=0.02)
    s.weight = (s.weight * np.float32(scale)).astype(np.float32)
    return s


def as_sol(s, val=None, weight=None):
    return dict(val=s.val if val is None else val,
                weight=s.weight if weight is None else weight,
                times=s.times, freqs=s.freqs, dir_names=s.dir_names,
                ant_names=s.ant_names, dir_radec=s.dir_radec, ant_pos=s.ant_pos)


def run_group(out, group, make_soltab, screen_type, order, ref, scale_order,
              sets, beta=5.0 / 3.0):
    """stationscreen.run once per parameter set (niter, nsigma,
    adjust_order) on a fresh soltab; the results go into ``out``."""
    name = f"{screen_type}_screen000"
    out[f"{group}_type"] = screen_type
    out[f"{group}_ref_ant"] = ref
    out[f"{group}_nsets"] = len(sets)
    for k, (niter, nsigma, adjust) in enumerate(sets):
        st = make_soltab()
        rc = stationscreen.run(st, name, order=order, beta=beta, niter=niter,
                               nsigma=nsigma, ref_ant=ref,
                               scale_order=scale_order, adjust_order=adjust,
                               ncpu=1)
        assert rc == 0
        ss = st.get_solset()
        scr, res = ss.made[name], ss.made[name + "resid"]
        p = f"{group}_s{k}_"
        out[p + "niter"] = niter
        out[p + "nsigma"] = float(nsigma)
        out[p + "adjust_order"] = int(adjust)
        out[p + "coef"] = scr.vals
        out[p + "resid"] = res.vals
        out[p + "w_out"] = scr.weights.astype(np.float32)
        out[p + "orders"] = res.weights[:, :, :, 0].astype(np.int32)
        out["piercepoints"] = ss.obj._v_file.arrays[f"/sol000/{name}/piercepoint"]
        assert float(scr.obj._v_attrs["beta"]) == beta
        out["beta"] = beta
        out["r_0"] = float(scr.obj._v_attrs["r_0"])
        n = (out[p + "w_out"] > 0).sum(axis=3)
        print(f"  {group} {niter, nsigma, adjust}: orders",
              dict(zip(*np.unique(out[p + "orders"], return_counts=True))),
              "unflagged", dict(zip(*np.unique(n, return_counts=True))))


def save(name, s, out, order):
    np.savez_compressed(
        os.path.join(HERE, name + ".npz"), val=s.val, weight=s.weight,
        ant_pos=s.ant_pos, dir_radec=s.dir_radec, order=order, **out)
    print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


def phase_case(name, shape, order, sets, scale=1.0, beta=5.0 / 3.0,
               mixed=False, tec=False):
    s = solutions(*shape, scale=scale)
    if mixed:
        rng = np.random.default_rng(20)
        fac = rng.choice(np.array([100.0, 400.0, 1600.0], np.float32),
                         size=s.weight.shape)
        tiny = (rng.random(s.weight.shape) < 0.01) & (s.weight > 0)
        s.weight = (s.weight * fac).astype(np.float32)
        s.weight[tiny] = np.float32(5e-4)
    ref = mg.reference_station(np.asarray(s.weight), 10)
    out = dict(groups=np.array(["phase", "tec"] if tec else ["phase"]))
    run_group(out, "phase", lambda: mg.DuckSoltab(as_sol(s)), "phase", order,
              ref, True, sets, beta)
    if tec:
        run_group(out, "tec", lambda: TecSoltab(as_sol(s)), "tec", order, ref,
                  True, sets, beta)
    save(name, s, out, order)


def tec_case():
    s = solutions(4, 6, 2, 14, scale=400.0)
    out = dict(groups=np.array(["ref", "noref"]))
    sets = [(3, 5.0, T), (4, 3.0, T), (4, 3.0, F)]
    for group, ref in (("ref", 2), ("noref", -1)):
        run_group(out, group, lambda: TecSoltab(as_sol(s)), "tec", 10, ref,
                  True, sets)
    save("walk14tec", s, out, 10)


def amp_case():
    s = solutions(4, 6, 2, 14, scale=4.0e4)
    amp = np.stack([10.0 ** (0.1 * s.val), 10.0 ** (0.07 * s.val)], axis=-1)
    wt = np.stack([s.weight, s.weight], axis=-1)
    out = dict(groups=np.array(["amp"]), amp_val=amp, amp_weight=wt)
    sets = [(3, 5.0, T), (4, 3.0, T), (4, 3.0, F)]

    def soltab():
        return AmpSoltab(as_sol(s), amp, wt, s.times, s.freqs)

    name = "amplitude_screen000"
    out["amp_type"], out["amp_ref_ant"], out["amp_nsets"] = "amplitude", -1, 3
    for k, (niter, nsigma, adjust) in enumerate(sets):
        st = soltab()
        rc = stationscreen.run(st, name, order=6, niter=niter, nsigma=nsigma,
                               scale_order=False, adjust_order=adjust, ncpu=1)
        assert rc == 0
        ss = st.get_solset()
        scr, res = ss.made[name], ss.made[name + "resid"]
        p = f"amp_s{k}_"
        out[p + "niter"], out[p + "nsigma"] = niter, float(nsigma)
        out[p + "adjust_order"] = int(adjust)
        out[p + "coef"], out[p + "resid"] = scr.vals, res.vals
        out[p + "w_out"] = scr.weights.astype(np.float32)
        out[p + "orders"] = res.weights[:, :, :, 0, :].astype(np.int32)
        out["piercepoints"] = ss.obj._v_file.arrays[f"/sol000/{name}/piercepoint"]
        out["beta"] = float(scr.obj._v_attrs["beta"])
        out["r_0"] = float(scr.obj._v_attrs["r_0"])
        print(f"  amp {niter, nsigma, adjust}: orders",
              dict(zip(*np.unique(out[p + "orders"], return_counts=True))),
              "flags in", int((wt == 0).sum()), "out",
              int((out[p + "w_out"] == 0).sum()))
    save("walk14amp", s, out, 6)


CASES = {
    "walk20": lambda: phase_case(
        "walk20", (5, 8, 2, 20), 12,
        [(2, 5.0, T), (4, 3.0, T), (4, 3.0, F), (1, 5.0, F), (4, 1e9, T)],
        scale=400.0),
    "walk20mixed": lambda: phase_case(
        "walk20mixed", (5, 8, 2, 20), 12, [(2, 5.0, T), (4, 3.0, T)],
        mixed=True),
    "walk20beta": lambda: phase_case(
        "walk20beta", (5, 8, 2, 20), 12, [(3, 3.0, T)], scale=400.0, beta=1.0),
    "walk50": lambda: phase_case(
        "walk50", (4, 6, 1, 50), 20, [(2, 5.0, T), (4, 3.0, T)], scale=400.0),
    "walk80": lambda: phase_case(
        "walk80", (3, 4, 1, 80), 20, [(3, 5.0, T), (4, 3.0, T)], scale=400.0,
        tec=True),
    "walk14tec": tec_case,
    "walk14amp": amp_case,
    "cascade12": lambda: phase_case(
        "cascade12", (5, 8, 2, 12), 11, [(8, 1.5, T), (8, 1.5, F)]),
}


def main():
    for name in sys.argv[1:] or CASES:
        print(name)
        CASES[name]()
    print("done")


if __name__ == "__main__":
    main()
