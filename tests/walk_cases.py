"""The cases of the order-walk tests (tests/test_fit_walk_cpu.py on the
oracle, tests/test_fit_walk.py on the kernels): the reference's own runs in
tests/golden/walk*.npz / cascade12.npz (make_golden_walk.py) and two
oracle-only shapes, D = 60 and D = 128.

A ``Run`` is one soltab fitted with one parameter set, in the layout of
sf_kl_fit: ``val`` / ``weight`` [T, F, A, D] (an amplitude soltab's pols
stacked along the station axis, as stationscreen.run fits them), the
per-station orders ``st`` and the expected ``coef``, ``resid``, ``w_out``
[T, F, A, D] and ``orders`` [T, F, A] (``None`` for an oracle-only run).
"""

import functools
from types import SimpleNamespace

import numpy as np

from conftest import load_golden
from oracle import geometry as og
from oracle import kl as okl

SCREEN_TYPES = {"phase": 0, "tec": 1, "amplitude": 2}

# golden file -> the weights were scaled to ~ 1 / sigma^2 (the walk moves)
GOLDEN_FILES = {"walk20": True, "walk20mixed": True, "walk20beta": True,
                "walk50": True, "walk80": True, "walk14tec": True,
                "walk14amp": True, "cascade12": False}
# oracle-only: (n_ant, n_time, n_freq, n_dir), the ABI's limits of the two
# fit pipelines
ORACLE_SHAPES = {"oracle60": (3, 4, 1, 60), "oracle128": (3, 2, 1, 128)}


def stack_pols(a):
    """[T, F, A, D, P] -> [T, F, P * A, D] (or [T, F, A, P] -> [T, F, P * A])."""
    return np.concatenate([a[..., p] for p in range(a.shape[-1])], axis=2)


def _st_orders(ant_pos, ref, order, n_pol=1, scale_order=True):
    st = okl.station_orders(ant_pos, ref, order, scale_order=scale_order)
    return [int(o) for o in st] * n_pol


@functools.lru_cache(maxsize=None)
def runs(name):
    """Every (group, parameter set) of a case, as a tuple of Runs."""
    if name in ORACLE_SHAPES:
        return (_oracle_only(name),)
    g = load_golden(name)
    out = []
    for group in g["groups"]:
        group = str(group)
        stype = str(g[f"{group}_type"])
        ref = int(g[f"{group}_ref_ant"])
        amp = stype == "amplitude"
        val = g["amp_val"] if amp else g.get(f"{group}_val", g["val"])
        wt = g["amp_weight"] if amp else g.get(f"{group}_weight", g["weight"])
        n_pol = val.shape[-1] if amp else 1
        for k in range(int(g[f"{group}_nsets"])):
            p = f"{group}_s{k}_"
            cv = (stack_pols if amp else np.asarray)
            out.append(SimpleNamespace(
                case=name, group=group, k=k, type=stype, ref=ref,
                scaled=GOLDEN_FILES[name], n_pol=n_pol,
                val=cv(val), weight=cv(wt), ant_pos=g["ant_pos"],
                pp=g["piercepoints"], order=int(g["order"]),
                st=_st_orders(g["ant_pos"], ref, int(g["order"]), n_pol, not amp),
                beta=float(g["beta"]), r_0=float(g["r_0"]),
                niter=int(g[p + "niter"]), nsigma=float(g[p + "nsigma"]),
                adjust=bool(g[p + "adjust_order"]),
                coef=cv(g[p + "coef"]), resid=cv(g[p + "resid"]),
                w_out=cv(g[p + "w_out"]), orders=cv(g[p + "orders"])))
    return tuple(out)


def _oracle_only(name):
    from ska_sdp_screen_fitting_amd.synthetic import make_solutions
    n_ant, n_time, n_freq, n_dir = ORACLE_SHAPES[name]
    s = make_solutions(n_ant=n_ant, n_time=n_time, n_freq=n_freq, n_dir=n_dir,
                       seed=7, flag_frac=0.02, outlier_frac=0.02)
    weight = (s.weight * np.float32(400.0)).astype(np.float32)
    pp, _, _ = og.piercepoints(s.dir_radec)
    ref = okl.reference_station(weight)
    return SimpleNamespace(
        case=name, group="phase", k=0, type="phase", ref=ref, scaled=True,
        n_pol=1, val=s.val, weight=weight, ant_pos=s.ant_pos, pp=pp, order=20,
        st=_st_orders(s.ant_pos, ref, 20), beta=5.0 / 3.0, r_0=100.0, niter=4,
        nsigma=3.0, adjust=True, coef=None, resid=None, w_out=None, orders=None)


def all_runs(names=None):
    return [r for n in (names or list(GOLDEN_FILES) + list(ORACLE_SHAPES))
            for r in runs(n)]


def run_id(r):
    return (f"{r.case}-{r.group}-n{r.niter}-s{r.nsigma:g}-"
            f"{'adj' if r.adjust else 'fix'}")


def run_oracle(r, val=None, **kw):
    """The oracle on a Run (optionally on other values, or with other
    parameters: niter, nsigma, adjust_order, beta, r_0) ->
    (coef, resid, w_out, orders) in the Run's layout."""
    val = r.val if val is None else val
    prm = dict(niter=r.niter, nsigma=r.nsigma, adjust_order=r.adjust,
               beta=r.beta, r_0=r.r_0)
    prm.update(kw)
    if r.type == "amplitude":
        A = val.shape[2] // r.n_pol
        unstack = lambda a: np.stack(                          # noqa: E731
            [a[:, :, p * A:(p + 1) * A] for p in range(r.n_pol)], axis=-1)
        o = okl.run_amplitude(unstack(val), unstack(r.weight), r.pp, r.order,
                              **prm)
        return tuple(stack_pols(o[k]) for k in ("coef", "resid", "w_out", "orders"))
    if r.type == "tec":
        o = okl.run_soltab(val, r.weight, r.ant_pos, r.pp, r.ref, r.order,
                           "tec", **prm)
    else:
        o = okl.run_phase(val, r.weight, r.ant_pos, r.pp, r.ref, r.order, **prm)
    return o["coef"], o["resid"], o["w_out"], o["orders"]


_oracle_cache = {}


def oracle(r):
    """run_oracle(r), computed once per Run and shared (do not modify)."""
    key = (r.case, r.group, r.k)
    if key not in _oracle_cache:
        _oracle_cache[key] = run_oracle(r)
    return _oracle_cache[key]


def expected(r):
    """What a kernel must give on a Run: the reference's own outputs, or the
    oracle's where there is no golden."""
    if r.coef is None:
        return oracle(r)
    return r.coef, r.resid, r.w_out, r.orders


def fitted(r):
    """[T, F, A] bool: the slots a pass fits (not the reference station)."""
    keep = np.ones(r.val.shape[:3], bool)
    if r.type != "amplitude" and r.ref >= 0:
        keep[:, :, r.ref] = False
    return keep


def walked(r, w_out, orders):
    """[T, F, A] bool: fitted slots whose final order is not the one every
    pass without a walk ends at, min(station_order, n_unflagged - 1)."""
    n = (w_out > 0).sum(axis=-1)
    st = np.asarray(r.st)[None, None, :]
    return fitted(r) & (n > 0) & (orders != np.minimum(st, n - 1))
