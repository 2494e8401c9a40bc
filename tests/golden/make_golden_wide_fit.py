#!/opt/conda/bin/python3.9
"""Golden vectors for the fit past SF_MAX_DIR (61..128 directions,
sf_set_basis_wide + sf_kl_fit, csrc/kl_fit_wide.hip), produced by running the
reference's stationscreen.run itself (same interpreter, shims and duck-typed
soltabs as make_golden.py / make_golden_wide.py; the reference places no bound
on the number of directions):

* wide_fit80.npz     phase, D = 80, 3 stations x 8 times x 2 freqs,
                     2 % flags, 0.5 % outliers, as KLScreen.fit calls it;
* wide_fit128.npz    phase, D = 128, 3 x 4 x 1;
* wide_fit80tec.npz  tec, D = 80, 3 x 4 x 1, niter = 3: case "noref"
                     (ref_ant = -1, quirk Q15) and case "ref" (ref_ant = 1);
* wide_fit80amp.npz  amplitude, D = 80, 3 x 4 x 2, both pols, as KLScreen.fit
                     calls it (order 12, niter 3, no order scaling,
                     ref_ant = -1).

Usage:  /opt/conda/bin/python3.9 tests/golden/make_golden_wide_fit.py
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
from ska_sdp_screen_fitting_amd.synthetic import (make_amplitudes,  # noqa: E402
                                                  make_solutions)


def as_sol(s, val=None):
    return dict(val=s.val if val is None else val, weight=s.weight,
                times=s.times, freqs=s.freqs, dir_names=s.dir_names,
                ant_names=s.ant_names, dir_radec=s.dir_radec, ant_pos=s.ant_pos)


def common(sol):
    return dict(val=sol["val"], weight=sol["weight"], times=sol["times"],
                freqs=sol["freqs"], dir_names=np.array(sol["dir_names"]),
                ant_names=np.array(sol["ant_names"]),
                dir_radec=sol["dir_radec"], ant_pos=sol["ant_pos"])


def phase_case(name, **kw):
    sol = as_sol(make_solutions(**kw))
    fit = mg.run_fit(sol)
    print(name, fit["fit_seconds"], "s ref", fit["ref_ant"], "orders",
          np.unique(fit["orders"], return_counts=True), "flags in",
          int((sol["weight"] == 0).sum()), "out", int((fit["w_out"] == 0).sum()))
    np.savez_compressed(
        os.path.join(HERE, name + ".npz"), ref_ant=fit["ref_ant"],
        order=fit["order"], coef=fit["coef"], w_out=fit["w_out"],
        resid=fit["resid"], orders=fit["orders"],
        piercepoints=fit["piercepoints"], beta=fit["beta"], r_0=fit["r_0"],
        **common(sol))


def tec_case():
    s = make_solutions(n_ant=3, n_time=4, n_freq=1, n_dir=80, seed=8082,
                       flag_frac=0.02, outlier_frac=0.005)
    sol = as_sol(s, s.val * 0.05)  # TECU-sized values
    out = dict(order=20, niter=3, **common(sol))
    for case, ref in (("noref", -1), ("ref", 1)):
        st = TecSoltab(sol)
        rc = stationscreen.run(st, "tec_screen000", order=20, niter=3,
                               ref_ant=ref, scale_order=True,
                               adjust_order=True, ncpu=1)
        assert rc == 0
        ss = st.get_solset()
        scr = ss.made["tec_screen000"]
        res = ss.made["tec_screen000resid"]
        out[f"{case}_ref_ant"] = ref
        out[f"{case}_coef"] = scr.vals
        out[f"{case}_w_out"] = scr.weights.astype(np.float32)
        out[f"{case}_resid"] = res.vals
        out[f"{case}_orders"] = res.weights[..., 0].astype(np.int32)
        out["piercepoints"] = ss.obj._v_file.arrays[
            "/sol000/tec_screen000/piercepoint"]
        print("tec", case, "orders",
              np.unique(out[f"{case}_orders"], return_counts=True), "flags in",
              int((s.weight == 0).sum()), "out",
              int((out[f"{case}_w_out"] == 0).sum()))
    np.savez_compressed(os.path.join(HERE, "wide_fit80tec.npz"), **out)


def amp_case():
    s = make_solutions(n_ant=3, n_time=4, n_freq=2, n_dir=80, seed=8083,
                       flag_frac=0.02, outlier_frac=0.005)
    make_amplitudes(s, seed=8084, flag_frac=0.02, outlier_frac=0.005)
    sol = as_sol(s)
    st = AmpSoltab(sol, s.amp_val, s.meta["amp_weight"], s.meta["amp_times"],
                   s.meta["amp_freqs"])
    rc = stationscreen.run(st, "amplitude_screen000", order=12, niter=3,
                           scale_order=False, adjust_order=True, ncpu=1)
    assert rc == 0
    ss = st.get_solset()
    ascr = ss.made["amplitude_screen000"]
    ares = ss.made["amplitude_screen000resid"]
    print("amp orders", np.unique(ares.weights, return_counts=True),
          "flags in", int((s.meta["amp_weight"] == 0).sum()), "out",
          int((ascr.weights == 0).sum()))
    np.savez_compressed(
        os.path.join(HERE, "wide_fit80amp.npz"),
        dir_radec=s.dir_radec, ant_pos=s.ant_pos,
        piercepoints=ss.obj._v_file.arrays[
            "/sol000/amplitude_screen000/piercepoint"],
        amp_val=s.amp_val, amp_weight=s.meta["amp_weight"], amp_order=12,
        niter=3, amp_coef=ascr.vals, amp_w_out=ascr.weights.astype(np.float32),
        amp_resid=ares.vals,
        amp_orders=ares.weights[:, :, :, 0, :].astype(np.int32))


def main():
    phase_case("wide_fit80", n_ant=3, n_time=8, n_freq=2, n_dir=80, seed=8081,
               flag_frac=0.02, outlier_frac=0.005)
    phase_case("wide_fit128", n_ant=3, n_time=4, n_freq=1, n_dir=128,
               seed=8128, flag_frac=0.02, outlier_frac=0.005)
    tec_case()
    amp_case()
    print("done")


if __name__ == "__main__":
    main()
