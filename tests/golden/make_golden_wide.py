#!/opt/conda/bin/python3.9
"""Golden vectors past SF_MAX_DIR: D = 80 directions, produced by running the
reference itself (same interpreter, shims and duck-typed soltabs as
make_golden.py; the reference places no bound on D):

* stationscreen.run on 3 stations x 2 times x 1 frequency of synthetic phases
  (2 % flags, 0.5 % outliers), exactly as KLScreen.fit calls it;
* KLScreen.make_matrix (kl_screen.py:192-380) at 17 x 17 pixels for every
  (frequency, station) pair: the planes the evaluation above 60 directions
  (sf_set_piercepoints + sf_kl_eval, kl_eval_wide.hip) is pinned to.

Usage:  /opt/conda/bin/python3.9 tests/golden/make_golden_wide.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (applies the shims)

import numpy as np  # noqa: E402

from ska_sdp_screen_fitting_amd.synthetic import make_solutions  # noqa: E402


def main():
    kw = dict(n_ant=3, n_time=2, n_freq=1, n_dir=80, seed=8080,
              flag_frac=0.02, outlier_frac=0.005)
    s = make_solutions(**kw)
    sol = dict(val=s.val, weight=s.weight, times=s.times, freqs=s.freqs,
               dir_names=s.dir_names, ant_names=s.ant_names,
               dir_radec=s.dir_radec, ant_pos=s.ant_pos)
    fit = mg.run_fit(sol)
    print("wide80 fit", fit["fit_seconds"], "s ref", fit["ref_ant"], "orders",
          np.unique(fit["orders"], return_counts=True))
    rad, dec, width = 126.23, 64.50, 3.3300000000000054
    scr = mg.make_kl(sol, fit, 0.2, rad, dec, width)
    pairs = [(0, a) for a in range(kw["n_ant"])]
    kl, xs, ys = mg.eval_slots(scr, pairs, 0, kw["n_time"], 0.2)
    np.savez_compressed(
        os.path.join(HERE, "wide80.npz"),
        val=sol["val"], weight=sol["weight"], times=sol["times"],
        freqs=sol["freqs"], dir_names=np.array(sol["dir_names"]),
        ant_names=np.array(sol["ant_names"]), dir_radec=sol["dir_radec"],
        ant_pos=sol["ant_pos"], ref_ant=fit["ref_ant"], order=fit["order"],
        coef=fit["coef"], w_out=fit["w_out"], resid=fit["resid"],
        orders=fit["orders"], piercepoints=fit["piercepoints"],
        mid_ra=fit["mid_ra"], mid_dec=fit["mid_dec"], beta=fit["beta"],
        r_0=fit["r_0"], pairs17=np.array(pairs), kl17=kl, x17=xs, y17=ys)
    print("done")


if __name__ == "__main__":
    main()
