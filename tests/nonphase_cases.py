"""The cases of the tec / amplitude fit tests (tests/test_fit_nonphase_cpu.py
on the oracle, tests/test_fit_nonphase.py on the kernels), as the ``Run``s of
tests/walk_cases.py:

* the reference's own unsharded runs: tec14, walk14tec, walk14amp, ties4tec,
  wide_fit80tec and wide_fit80amp (tests/golden/);
* oracle-only runs at D = 8, 33, 60, 61 and 128 -- a tec fit with
  ref_ant = 1, one with ref_ant = -1 (quirk Q15: referenced to the LAST
  station of the soltab) and an amplitude fit at each D, with weights near
  1 / sigma^2 (the order walk moves), niter 4, nsigma 3 and T x D > 256 (the
  block sigma's 256-thread loop over the block wraps).  Each oracle-only tec
  run has one (frequency, station) block that is all NaN and one whose
  weights are all zero.

``shards(A)`` is the uneven station split both test files use.
"""

import functools
from types import SimpleNamespace

import numpy as np

import walk_cases as wc
from conftest import load_golden
from oracle import geometry as og
from oracle import kl as okl

# D -> T of the oracle-only runs (4 stations, 2 frequencies): T x D > 256
ORACLE_T = {8: 33, 33: 8, 60: 5, 61: 5, 128: 3}
N_ANT, N_FREQ = 4, 2
# the order of the oracle-only runs is min(20, D - 1), except at D = 8: the
# walk moves a slot's order only up from its station's order, to at most
# n_unflagged - 1, so from D - 1 = 7 no slot could move, and from 4 less than
# a quarter of the amplitude slots do (validity (a))
ORACLE_ORDER = {8: 3}
# the skipped blocks of the oracle-only tec runs, (frequency, station): not
# the last station (every block of its frequency would be NaN after the
# referencing of ref_ant = -1) and not station 1 (the reference of "ref")
NAN_BLOCK = (0, 0)
ZERO_BLOCK = (1, 2)


def _run(case, group, stype, ref, val, weight, ant_pos, pp, order, niter,
         nsigma, adjust, n_pol=1, scaled=False, skipped=(), k=0, coef=None,
         resid=None, w_out=None, orders=None):
    amp = stype == "amplitude"
    return SimpleNamespace(
        case=case, group=group, k=k, type=stype, ref=ref, scaled=scaled,
        n_pol=n_pol, val=val, weight=weight, ant_pos=ant_pos, pp=pp,
        order=order, st=wc._st_orders(ant_pos, ref, order, n_pol, not amp),
        beta=5.0 / 3.0, r_0=100.0, niter=niter, nsigma=nsigma, adjust=adjust,
        skipped=tuple(skipped), coef=coef, resid=resid, w_out=w_out,
        orders=orders)


def _golden_tec(name, groups):
    g = load_golden(name)
    out = []
    for group in groups:
        p = f"{group}_" if group else ""
        out.append(_run(
            name, group or "ref", "tec", int(g[p + "ref_ant"]), g["val"],
            g["weight"], g["ant_pos"], g["piercepoints"], int(g["order"]),
            int(g["niter"]), 5.0, True, coef=g[p + "coef"],
            resid=g[p + "resid"], w_out=g[p + "w_out"], orders=g[p + "orders"]))
    return out


def _golden_amp(name):
    g = load_golden(name)
    sp = wc.stack_pols
    return [_run(name, "amp", "amplitude", -1, sp(g["amp_val"]),
                 sp(g["amp_weight"]), g["ant_pos"], g["piercepoints"],
                 int(g["amp_order"]), int(g["niter"]), 5.0, True,
                 n_pol=g["amp_val"].shape[-1], coef=sp(g["amp_coef"]),
                 resid=sp(g["amp_resid"]), w_out=sp(g["amp_w_out"]),
                 orders=sp(g["amp_orders"]))]


def _walk(name):
    return [SimpleNamespace(**vars(r), skipped=()) for r in wc.runs(name)]


@functools.lru_cache(maxsize=None)
def golden_runs():
    return tuple(_golden_tec("tec14", ("ref", "noref")) + _walk("walk14tec")
                 + _walk("walk14amp") + _golden_tec("ties4tec", ("",))
                 + _golden_tec("wide_fit80tec", ("ref", "noref"))
                 + _golden_amp("wide_fit80amp"))


@functools.lru_cache(maxsize=None)
def oracle_runs(D):
    """(tec ref_ant = 1, tec ref_ant = -1, amplitude) at D directions."""
    from ska_sdp_screen_fitting_amd.synthetic import (make_amplitudes,
                                                      make_solutions)
    s = make_solutions(n_ant=N_ANT, n_time=ORACLE_T[D], n_freq=N_FREQ, n_dir=D,
                       seed=7 + D, flag_frac=0.03, outlier_frac=0.02)
    pp, _, _ = og.piercepoints(s.dir_radec)
    order = ORACLE_ORDER.get(D, min(20, D - 1))
    val = s.val * 0.05
    weight = (s.weight * np.float32(1.6e5)).astype(np.float32)
    val[:, NAN_BLOCK[0], NAN_BLOCK[1], :] = np.nan
    weight[:, ZERO_BLOCK[0], ZERO_BLOCK[1], :] = 0.0
    prm = dict(niter=4, nsigma=3.0, adjust=True, scaled=True)
    out = [_run(f"oracle{D}tec", group, "tec", ref, val, weight, s.ant_pos, pp,
                order, skipped=(NAN_BLOCK, ZERO_BLOCK), **prm)
           for group, ref in (("ref", 1), ("noref", -1))]
    make_amplitudes(s, seed=100 + D, flag_frac=0.03, outlier_frac=0.02)
    aw = (s.meta["amp_weight"] * np.float32(1e4)).astype(np.float32)
    out.append(_run(f"oracle{D}amp", "amp", "amplitude", -1,
                    wc.stack_pols(s.amp_val), wc.stack_pols(aw), s.ant_pos, pp,
                    order, n_pol=s.amp_val.shape[-1], **prm))
    return tuple(out)


def all_oracle_runs():
    return [r for D in ORACLE_T for r in oracle_runs(D)]


def all_runs():
    return list(golden_runs()) + all_oracle_runs()


def n_dir(r):
    return r.val.shape[-1]


def fit_mask(r):
    """[T, F, A] bool: the slots a pass fits -- wc.fitted(r) without the
    skipped blocks of the Run."""
    keep = wc.fitted(r).copy()
    for f, a in r.skipped:
        keep[:, f, a] = False
    return keep


def shards(A):
    """Uneven contiguous station ranges covering 0..A: a one-station shard,
    the middle and the shard that holds the last station (A = 3: two)."""
    cuts = sorted({0, 1, max(1, A - 2), A})
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]


def sub_run(r, a0, a1, extra=None):
    """The Run of stations a0..a1 alone (``extra``: one more station appended)
    as an unsharded tec soltab with ref_ant = -1: what a shard fitted with
    ref_phase = NULL computes."""
    assert r.type == "tec" and r.ref == -1
    idx = list(range(a0, a1)) + ([] if extra is None else [extra])
    sub = SimpleNamespace(**vars(r))
    sub.val, sub.weight = r.val[:, :, idx], r.weight[:, :, idx]
    sub.ant_pos = r.ant_pos[idx]
    sub.st = [r.st[a] for a in idx]
    sub.coef = sub.resid = sub.w_out = sub.orders = None
    return sub


_alone_cache = {}


def oracle_alone(r, a0, a1):
    """The oracle on stations a0..a1 alone, computed once (do not modify)."""
    key = (r.case, r.group, r.k, a0, a1)
    if key not in _alone_cache:
        _alone_cache[key] = wc.run_oracle(sub_run(r, a0, a1))
    return _alone_cache[key]
