#!/opt/conda/bin/python3.9
"""Golden vectors below the pinv cutoff: the reference's own
``stationscreen.run`` (the interpreter, shims and duck-typed soltabs of
make_golden.py) on the two cases of tests/cutoff_cases.py that reach the
cutoff at the reference's fixed r_0 = 100 -- data only.

* twins20    D = 20, two pairs of directions 1 and 2 piercepoint units apart:
             C has two singular values below 1e-3 (rank 18 of 20); slots
             with one twin of each pair flagged (a full-rank subset), one
             twin, and both twins of a pair.  Phase and tec in
             near_twins20.npz, amplitude (two frequencies) in
             near_twins20amp.npz.
* tie_small  D = 4 (near_tie4.npz), one pass: slots whose only two unflagged
             directions are a twin pair -- C_sub = [[0, b], [b, 0]] with
             |b| = 2.3e-4, so pinv(C_sub) = 0 -- beside slots whose only two
             are an ordinary pair (the e_2 rule of make_golden_ties.py).

The inputs come from ``cutoff_cases.inputs``; a file holds ``dir_radec``,
``ant_pos``, the reference's ``piercepoints``, ``r_0``, ``beta`` and per group
(phase / tec / amp) ``<group>_val / _weight / _ref_ant / _order / _niter /
_nsigma / _adjust`` (the inputs, for the test that they are the ones
cutoff_cases makes) and ``<group>_coef / _resid / _w_out / _orders``.

Usage:  timeout 1200 /opt/conda/bin/python3.9 tests/golden/make_golden_near.py
(under ``timeout``, for make_golden_walk.py's reason)

The run that made the committed files (numpy 1.26.4, scipy 1.7.1), and the
reference against the oracle (tests/test_fit_cutoff_cpu.py):

  near_twins20     90151 bytes   phase: final orders 14..19, 11..20
                   unflagged; tec: orders 10..19
  near_twins20amp  66850 bytes   orders 6..19
  near_tie4        41078 bytes   54 (108 for the two pols) two-direction
                   slots; 160 zero coefficients = the reference station's 84
                   + 60 of the 15 twin-pair slots + 16 of the 4 ordinary
                   pairs whose second weight is 5e-4
  No two-direction subset left rounding residue in the reference's U.

The reference and the oracle agree: orders and flagged weights identical,
coefficients within 6e-12 (twins20, |coef|max 12.7) and 5e-17 (tie_small),
residuals within 4e-15 (tie_small) and 3e-12.  In particular the doubtful
spot -- the screen of a twin-pair slot, or of a pair whose second weight is
below the cutoff, is ``atan2`` of an all-zero projection, where the sign of
a BLAS zero could turn 0 into +-pi -- comes out +0 in both, also at the slot
(time 2, freq 1, station 2) whose second phase is 2.47 rad, cos < 0: the
reference's coefficients there are exactly 0 and its residuals exactly the
referenced values (value - 1 for an amplitude).  oracle/kl.py needed no
change.  (The kernels' two-direction shortcut did: it formed 0 x W cos(phi),
a zero with the sign of the cosine, and atan2(+0, -0) is pi.)

The values of ``make_solutions`` differ in the last bit between numpy builds
(its ``coeff @ basis`` is a BLAS product), so the files' ``<group>_val`` are
the inputs of record; cutoff_cases takes them from here.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (applies the shims)

import numpy as np  # noqa: E402

from make_golden_gain import AmpSoltab  # noqa: E402
from make_golden_tec import TecSoltab  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, mg.REPO)
import cutoff_cases as cc  # noqa: E402

SCREEN = {"phase": "phase", "tec": "tec", "amp": "amplitude"}


def run_group(inp, group, out):
    d = inp["groups"][group]
    amp = group == "amp"
    nf = d["val"].shape[1]
    sol = dict(val=d["val"], weight=d["weight"], times=inp["times"],
               freqs=inp["freqs"][:nf], dir_names=inp["dir_names"],
               ant_names=inp["ant_names"], dir_radec=inp["dir_radec"],
               ant_pos=inp["ant_pos"])
    if amp:
        phase = dict(sol, val=d["val"][..., 0], weight=d["weight"][..., 0])
        st = AmpSoltab(phase, d["val"], d["weight"], sol["times"], sol["freqs"])
    else:
        st = (TecSoltab if group == "tec" else mg.DuckSoltab)(sol)
    name = SCREEN[group] + "_screen000"
    rc = mg.stationscreen.run(st, name, order=d["order"], niter=d["niter"],
                              nsigma=d["nsigma"], ref_ant=d["ref_ant"],
                              scale_order=not amp, adjust_order=d["adjust"],
                              ncpu=1)
    assert rc == 0
    ss = st.get_solset()
    scr, res = ss.made[name], ss.made[name + "resid"]
    for k in ("val", "weight", "ref_ant", "order", "niter", "nsigma"):
        out[f"{group}_{k}"] = d[k]
    out[f"{group}_adjust"] = int(d["adjust"])
    out[f"{group}_coef"] = scr.vals
    out[f"{group}_resid"] = res.vals
    out[f"{group}_w_out"] = scr.weights.astype(np.float32)
    ow = res.weights
    out[f"{group}_orders"] = (ow[:, :, :, 0, :] if amp else
                              ow[:, :, :, 0]).astype(np.int32)
    out["piercepoints"] = ss.obj._v_file.arrays[f"/sol000/{name}/piercepoint"]
    out["beta"] = float(scr.obj._v_attrs["beta"])
    out["r_0"] = float(scr.obj._v_attrs["r_0"])
    n = (out[f"{group}_w_out"] > 0).sum(axis=3)
    # no two-direction slot whose subset SVD (the reference's own LAPACK) is
    # not an exact permutation: make_golden_ties.py's ``tie_residue``, where
    # the screen is atan2 of rounding residue, must not occur here
    from scipy.linalg import svd
    w_out = out[f"{group}_w_out"]
    if amp:
        w_out = np.moveaxis(w_out, -1, -2)
    for idx in np.argwhere((w_out > 0).sum(axis=-1) == 2):
        unfl = np.where(w_out[tuple(idx)] > 0)[0]
        c, _, _ = mg.stationscreen._calculate_svd(
            out["piercepoints"][unfl], out["r_0"], out["beta"], 2)
        u = svd(c)[0]
        assert np.all((u == 0.0) | (np.abs(u) == 1.0)), (group, idx, u)
    print(f"  {group}: orders",
          dict(zip(*np.unique(out[f"{group}_orders"], return_counts=True))),
          "unflagged", dict(zip(*np.unique(n, return_counts=True))),
          "coef: zeros", int((scr.vals == 0).sum()), "of", scr.vals.size,
          "|coef|max", float(np.abs(scr.vals).max()))


def main():
    files = {"near_twins20": ("twins20", ("phase", "tec")),
             "near_twins20amp": ("twins20", ("amp",)),
             "near_tie4": ("tie_small", ("phase", "tec", "amp"))}
    for fname, (case, groups) in files.items():
        print(fname)
        inp = cc.inputs(case)
        out = dict(dir_radec=inp["dir_radec"], ant_pos=inp["ant_pos"])
        for g in groups:
            run_group(inp, g, out)
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **out)
        print(fname, os.path.getsize(path), "bytes")
    print("done")


if __name__ == "__main__":
    main()
