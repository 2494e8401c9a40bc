"""The cases of the pinv-cutoff tests (tests/test_fit_cutoff_cpu.py on the
oracle, tests/test_fit_cutoff.py on the kernels): KL covariances C with
eigenvalues at or below the 1e-3 cutoff of ``pinv(C, rcond=1e-3)``
(kPinvAtol, csrc/kl_fit_steps.h), which no other input of the suite has.

Two ways into the regime:

* a large r_0 (C scales with r_0^-beta): ``r0_*`` at D = 20 (rank 17, 4 and
  0 of 20), the ends of the lane kernel's range (D = 7, 23), the subset pool
  at one slot per wavefront (D = 50), the wide fit (D = 80, 128), a tec and
  an amplitude soltab (D = 14), and weights of 5e-4 beside a truncated C
  (``mixed20``);
* nearly coincident directions at the reference's r_0 = 100: ``twins20``
  (two pairs 1 and 2 piercepoint units apart: rank 18 of 20), ``dup12`` (one
  direction twice: an eigenvalue that is exactly 0) and ``tie_small`` (D = 4;
  slots whose only two unflagged directions are a twin pair, |b| = 2.3e-4,
  beside slots whose only two are an ordinary pair; ``tie_wide``: the same
  at D = 64, for the wide fit).

``twins20`` and ``tie_small`` are also run by the reference itself
(tests/golden/make_golden_near.py -> near_*.npz); their Runs then carry the
reference's piercepoints, and ``reference(r)`` gives its outputs.

The Runs are those of tests/walk_cases.py, so its ``run_oracle`` / ``oracle``
and the ``fit`` / ``check`` / ``same_bytes`` of tests/test_fit_walk.py serve
unchanged.  ``RANK[case]`` is the number of singular values of the full C
above the cutoff.
"""

import functools
import os
from types import SimpleNamespace

import numpy as np

import walk_cases as wc
from conftest import GOLDEN
from oracle import geometry as og
from oracle import kl as okl

# one piercepoint unit (a pixel of the 0.0005 deg TAN plane of
# stationscreen.py:275-300), in radians of declination
PP_UNIT = np.deg2rad(0.0005)

# case -> (n_dir, (n_ant, n_time, n_freq), r_0, rank of the full C)
R0_CASES = {
    "r0_1e4": (20, (5, 7, 3), 1e4, 17),
    "r0_1e5": (20, (5, 7, 3), 1e5, 4),
    "r0_1e6": (20, (5, 7, 3), 1e6, 0),
    "d7_r0_1e5": (7, (5, 7, 3), 1e5, 3),
    "d23_r0_1e5": (23, (5, 7, 3), 1e5, 4),
    "d50_r0_1e4": (50, (3, 4, 1), 1e4, 34),
    "d80_r0_1e4": (80, (3, 4, 1), 1e4, 41),
    "d128_r0_1e4": (128, (3, 4, 1), 1e4, 53),
    "mixed20_r0_1e4": (20, (5, 7, 3), 1e4, 17),
}
RANK = {k: v[3] for k, v in R0_CASES.items()}
RANK.update(tec14_r0_1e4=12, amp14_r0_1e4=12, twins20=18, dup12=11,
            tie_small=3, tie_wide=63)
# the twin pairs (twin, partner, distance in piercepoint units)
TWINS20 = ((5, 2, 1.0), (13, 9, 2.0))
TIE_TWIN = (2, 0, 1.0)
DUP12 = (7, 3)
NEAR_FILES = {"twins20": ("near_twins20", "near_twins20amp"),
              "tie_small": ("near_tie4",)}


def _solutions(n_dir, shape, **kw):
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    n_ant, n_time, n_freq = shape
    prm = dict(seed=11, flag_frac=0.02, outlier_frac=0.02)
    prm.update(kw)
    return make_solutions(n_ant=n_ant, n_time=n_time, n_freq=n_freq,
                          n_dir=n_dir, **prm)


def _twin(s, twin, partner, dist, rng):
    """Direction ``twin`` moves to ``dist`` units north of ``partner`` and
    takes its phases plus 0.05 rad of noise."""
    s.dir_radec[twin] = s.dir_radec[partner]
    s.dir_radec[twin, 1] += np.float32(dist * PP_UNIT)
    s.val[..., twin] = s.val[..., partner] + rng.normal(
        0.0, 0.05, size=s.val.shape[:3])


def _amplitudes(val, weight):
    """The two pols of walk14amp (make_golden_walk.py) from phase values."""
    amp = np.stack([10.0 ** (0.1 * val), 10.0 ** (0.07 * val)], axis=-1)
    return amp, np.stack([weight, weight], axis=-1)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """What a case is made of, before any fit: a dict of dir_radec, ant_pos
    and per group (phase / tec / amp) val, weight, ref_ant, order, niter,
    nsigma, adjust.  make_golden_near.py feeds the reference from it."""
    P = dict(niter=3, nsigma=3.0, adjust=True)
    if name in R0_CASES:
        n_dir, shape, _, _ = R0_CASES[name]
        s = _solutions(n_dir, shape)
        w = (s.weight * np.float32(400.0)).astype(np.float32)
        if name.startswith("mixed"):
            # a few weights of 5e-4, as in walk20mixed: the slow class
            rng = np.random.default_rng(20)
            w[(rng.random(w.shape) < 0.01) & (w > 0)] = np.float32(5e-4)
        groups = dict(phase=dict(val=s.val, weight=w, order=min(20, n_dir - 1),
                                 **P))
    elif name in ("tec14_r0_1e4", "amp14_r0_1e4"):
        s = _solutions(14, (4, 6, 2))
        if name.startswith("tec"):
            w = (s.weight * np.float32(400.0)).astype(np.float32)
            groups = dict(tec=dict(val=s.val, weight=w, order=10, **P))
        else:
            w = (s.weight * np.float32(4.0e4)).astype(np.float32)
            amp, wt = _amplitudes(s.val, w)
            groups = dict(amp=dict(val=amp, weight=wt, order=6, **P))
    elif name == "twins20":
        s = _solutions(20, (5, 7, 3))
        rng = np.random.default_rng(2020)
        for twin, partner, dist in TWINS20:
            _twin(s, twin, partner, dist, rng)
        w = (s.weight * np.float32(400.0)).astype(np.float32)
        (t1, p1, _), (t2, _, _) = TWINS20
        T, F, A, _ = w.shape
        for t in range(T):
            for f in range(F):
                for a in range(A):
                    k = (t + f + a) % 7
                    if k == 0:      # one twin of each pair: a full-rank subset
                        w[t, f, a, [t1, t2]] = 0.0
                    elif k == 1:    # one twin: the other pair still truncates
                        w[t, f, a, t1] = 0.0
                    elif k == 2:    # both twins of a pair
                        w[t, f, a, [t1, p1]] = 0.0
        amp, wt = _amplitudes(s.val[:, :2], w[:, :2] * np.float32(100.0))
        groups = dict(phase=dict(val=s.val, weight=w, order=19, **P),
                      tec=dict(val=s.val, weight=w, order=19, **P),
                      amp=dict(val=amp, weight=wt, order=6, **P))
    elif name == "dup12":
        s = _solutions(12, (5, 7, 3))
        rng = np.random.default_rng(1212)
        _twin(s, DUP12[0], DUP12[1], 0.0, rng)
        w = (s.weight * np.float32(400.0)).astype(np.float32)
        groups = dict(phase=dict(val=s.val, weight=w, order=11, **P))
    elif name == "tie_small":
        s = _solutions(4, (5, 7, 3), flag_frac=0.0, outlier_frac=0.0)
        rng = np.random.default_rng(44)
        _twin(s, *TIE_TWIN, rng)
        w = np.zeros(s.weight.shape, np.float32)
        # which directions a slot keeps, by its running number
        keep = ([0, 2], [0, 1], [2, 3], [0, 1, 2, 3], [0, 2, 3], [0, 1, 3])
        T, F, A, _ = w.shape
        for t in range(T):
            for f in range(F):
                for a in range(A):
                    k = ((t * F + f) * A + a) % 6
                    w[t, f, a, keep[k]] = 400.0
                    if k == 2:      # an ordinary pair with unequal weights
                        w[t, f, a, 3] = 100.0
                    if k == 0 and t == 0:   # a twin pair in the slow class
                        w[t, f, a, 2] = 5e-4
                    if k == 1 and t in (1, 2):
                        # an ordinary pair whose second weight is below the
                        # cutoff: inv_u = pinv([w_2]) = 0, the fit is 0; at
                        # station 2 with cos(phi_2) < 0, where a zero of the
                        # wrong sign would turn atan2(0, 0) into pi
                        w[t, f, a, 1] = 5e-4
                        if a == 2:
                            s.val[t, f, a, 1] += 2.5
        one = dict(niter=1, nsigma=5.0, adjust=True)
        amp, wt = _amplitudes(s.val, w)
        groups = dict(phase=dict(val=s.val, weight=w, order=3, **one),
                      tec=dict(val=s.val, weight=w, order=3, **one),
                      amp=dict(val=amp, weight=wt, order=3, **one))
    elif name == "tie_wide":
        # the same pairs among 64 directions: the workgroup-per-slot fit
        s = _solutions(64, (3, 4, 1), flag_frac=0.0, outlier_frac=0.0)
        rng = np.random.default_rng(64)
        _twin(s, *TIE_TWIN, rng)
        w = np.zeros(s.weight.shape, np.float32)
        T, F, A, _ = w.shape
        for t in range(T):
            for f in range(F):
                for a in range(A):
                    k = ((t * F + f) * A + a) % 4
                    w[t, f, a, ([0, 2], [0, 1], slice(None), [2, 3])[k]] = 400.0
        one = dict(niter=1, nsigma=5.0, adjust=True)
        amp, wt = _amplitudes(s.val, w)
        groups = dict(phase=dict(val=s.val, weight=w, order=20, **one),
                      tec=dict(val=s.val, weight=w, order=20, **one),
                      amp=dict(val=amp, weight=wt, order=12, **one))
    else:
        raise KeyError(name)
    for g, d in groups.items():
        d["ref_ant"] = -1 if g == "amp" else okl.reference_station(d["weight"])
    return dict(dir_radec=s.dir_radec, ant_pos=s.ant_pos, times=s.times,
                freqs=s.freqs, dir_names=s.dir_names, ant_names=s.ant_names,
                groups=groups)


@functools.lru_cache(maxsize=None)
def near_golden(name):
    """The reference's own run of a case (make_golden_near.py), its files
    merged into one dict."""
    g = {}
    for f in NEAR_FILES[name]:
        g.update(np.load(os.path.join(GOLDEN, f + ".npz"), allow_pickle=False))
    return g


@functools.lru_cache(maxsize=None)
def runs(name):
    """The Runs (walk_cases) of a case, one per group."""
    inp = inputs(name)
    if name in NEAR_FILES:
        # the file's inputs: what the reference was given (make_solutions'
        # matrix products differ in the last bit between numpy builds)
        g = near_golden(name)
        pp = g["piercepoints"]
        inp = dict(inp, groups={
            grp: dict(d, val=g[f"{grp}_val"], weight=g[f"{grp}_weight"])
            for grp, d in inp["groups"].items()})
    else:
        pp, _, _ = og.piercepoints(inp["dir_radec"])
    r_0 = R0_CASES[name][2] if name in R0_CASES else (
        1e4 if name.endswith("r0_1e4") else 100.0)
    out = []
    for group, d in inp["groups"].items():
        amp = group == "amp"
        cv = wc.stack_pols if amp else np.asarray
        n_pol = 2 if amp else 1
        out.append(SimpleNamespace(
            case=name, group=group, k=0,
            type="amplitude" if amp else group, ref=d["ref_ant"], scaled=True,
            n_pol=n_pol, val=cv(d["val"]), weight=cv(d["weight"]),
            ant_pos=inp["ant_pos"], pp=pp, order=d["order"],
            st=wc._st_orders(inp["ant_pos"], d["ref_ant"], d["order"], n_pol,
                             not amp),
            beta=5.0 / 3.0, r_0=r_0, niter=d["niter"], nsigma=d["nsigma"],
            adjust=d["adjust"], coef=None, resid=None, w_out=None,
            orders=None))
    return tuple(out)


CASES = list(R0_CASES) + ["tec14_r0_1e4", "amp14_r0_1e4", "twins20", "dup12",
                          "tie_small", "tie_wide"]


def all_runs(names=None):
    return [r for n in (names or CASES) for r in runs(n)]


def reference(r):
    """(coef, resid, w_out, orders) of the reference's own run of a
    ``twins20`` / ``tie_small`` Run, in the Run's layout."""
    g = near_golden(r.case)
    cv = wc.stack_pols if r.type == "amplitude" else np.asarray
    return tuple(cv(g[f"{r.group}_{k}"])
                 for k in ("coef", "resid", "w_out", "orders"))


def referenced(r):
    """The values a pass fits: minus the reference station's (walk_cases.
    run_oracle does the same; amplitudes are not referenced)."""
    if r.type == "amplitude" or r.ref < 0:
        return r.val
    return r.val - r.val[:, :, r.ref:r.ref + 1, :]


def singular_values(r, idx=None):
    """Singular values of C (of the rows and columns ``idx``) at the Run's
    r_0 and beta, descending."""
    pp = r.pp if idx is None else r.pp[idx]
    c, _, _ = okl.calculate_svd(pp, r.r_0, r.beta)
    return np.linalg.svd(c, compute_uv=False)


def pair_slots(r):
    """([T, F, A] bool, [T, F, A] bool): the fitted slots with exactly two
    unflagged directions whose fit is zero -- the twin pair (pinv(C_sub) = 0)
    or a second weight at or below the cutoff (inv_u = pinv([w_2]) = 0) --
    and those the e_2 rule fits."""
    un = r.weight > 0
    two = wc.fitted(r) & (un.sum(axis=-1) == 2)
    twin, partner, _ = TIE_TWIN
    zero = two & un[..., twin] & un[..., partner]
    for idx in map(tuple, np.argwhere(two)):
        second = np.where(un[idx])[0][1]
        if r.weight[idx][second] <= okl.PINV_ATOL:
            zero[idx] = True
    return zero, two & ~zero


def check_pairs(r, coef, resid, orders):
    """What the reference gives on two-direction slots (near_tie4.npz), held
    against any (coef, resid, orders): a zero fit leaves every coefficient 0
    and the residual the value bit for bit (value - 1 of an amplitude: the
    screen is atan2(+0, +0) = 0, never +-pi); the e_2 rule leaves a residual
    of 0, to rounding, at the second direction."""
    zero, kept = pair_slots(r)
    un = r.weight > 0
    assert np.all(orders[zero | kept] == 1)
    assert np.all(coef[zero] == 0.0)
    val = referenced(r)
    want = val[zero] - 1.0 if r.type == "amplitude" else val[zero]
    assert np.array_equal(np.ascontiguousarray(resid[zero]).view(np.uint8),
                          np.ascontiguousarray(want).view(np.uint8))
    for idx in map(tuple, np.argwhere(kept)):
        second = np.where(un[idx])[0][1]
        # the values are O(1); the reference's own residuals there <= 1.2e-16
        assert abs(resid[idx][second]) <= 1e-12
        assert np.abs(coef[idx]).max() > 0
