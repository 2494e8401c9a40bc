"""Digest of the KL fit's outputs on every fit fixture under tests/golden/,
for the library named by SCREENFIT_LIB (default: the package's own): one line
per case, setting and output with the sha256 of the raw bytes of coef, resid,
w_out and order_out, and one with the sha256 of the pool of subset bases the
fit left (Context.fit_pool / fit_pool_wide: masks and entries, sorted by
mask).  Two builds compute the same fit bit for bit exactly when their outputs
of this tool are equal byte for byte.

    SCREENFIT_LIB=/path/to/libscreenfit.so python tools/fit_digest.py [--out FILE]

The cases are the fixtures with the inputs and parameters the GPU tests feed
them (gpu_fit of tests/test_gpu_parity.py, wide_fit of tests/test_wide_fit.py,
the fits of tests/test_tec.py and tests/test_gain.py): the smallest sets that
reach each branch of the fit -- tiny weights (the truncated eigen-solve),
two-direction ties, heavy flags, the block sigma of tec / amplitude, and 80,
96 and 128 directions (3, 2 and 1 matrices of the wide fit in LDS).
wide_tiny96 is no fixture file: it is the input of
test_wide_phase_fit_tiny_weights, the wide fit's truncated eigen-solve.

Settings, where they apply: the default; with <= 60 directions
SF_OPT_FIT_GENERAL = 1 (phase at the case's niter, tec at niter 1, which is
what the general kernel accepts; it builds no pool, so its pool line repeats
the previous fit's), SF_OPT_FIT_PACK = 0, SF_OPT_FIT_LEAN = 0,
SF_OPT_FIT_LANE = 0 (every slot through the pass kernel),
SF_OPT_FIT_SUBSET_DELETION = 0, 2 and 3 (subset bases by Jacobi, by deletions
from the global basis, by deletions from ancestors at every mask count) and
SF_OPT_FIT_EIG_WAVES = 1; above 60 directions SF_OPT_FIT_WIDE_CACHE = 0.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-screen-fitting_amd"))
from ska_sdp_screen_fitting_amd import geometry, get_context  # noqa: E402
from ska_sdp_screen_fitting_amd._lib import (  # noqa: E402
    SF_MAX_DIR, SF_OPT_FIT_EIG_WAVES, SF_OPT_FIT_GENERAL, SF_OPT_FIT_LANE, SF_OPT_FIT_LEAN,
    SF_OPT_FIT_PACK, SF_OPT_FIT_SUBSET_DELETION, SF_OPT_FIT_WIDE_CACHE,
    SF_SCREEN_AMPLITUDE, SF_SCREEN_PHASE, SF_SCREEN_TEC, library_identity)
from ska_sdp_screen_fitting_amd.stationscreen import station_orders  # noqa: E402
from ska_sdp_screen_fitting_amd.synthetic import make_solutions  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
# (tag, (option, value, value restored after the fit), for wide cases)
SETTINGS = (("default", None, None), ("general", (SF_OPT_FIT_GENERAL, 1, 0), False),
            ("pack0", (SF_OPT_FIT_PACK, 0, 1), False),
            ("lean0", (SF_OPT_FIT_LEAN, 0, 1), False),
            ("lane0", (SF_OPT_FIT_LANE, 0, 1), False),
            ("deletion0", (SF_OPT_FIT_SUBSET_DELETION, 0, 1), False),
            ("deletion2", (SF_OPT_FIT_SUBSET_DELETION, 2, 1), False),
            ("deletion3", (SF_OPT_FIT_SUBSET_DELETION, 3, 1), False),
            ("eigwaves1", (SF_OPT_FIT_EIG_WAVES, 1, 0), False),
            ("widecache0", (SF_OPT_FIT_WIDE_CACHE, 0, 1), True))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))


def stack_pols(a):
    """[T, F, A, D, P] -> [T, F, P * A, D], as stationscreen.run stacks the
    pols of an amplitude soltab into one fit."""
    return np.concatenate([a[..., p] for p in range(a.shape[-1])], axis=2)


def cases():
    """(name, val, weight, piercepoints, station orders, ref_ant, screen
    type, niter)"""
    for name in ("synth12tiny", "synth20", "synth50", "ties4", "ties6",
                 "wide_fit80", "wide_fit128"):
        g = load(name)
        ref = int(g["ref_ant"])
        yield (name, g["val"], g["weight"], g["piercepoints"],
               station_orders(g["ant_pos"], ref, int(g["order"])), ref,
               SF_SCREEN_PHASE, 2)
    g = load("ties4tec")
    ref = int(g["ref_ant"])
    yield ("ties4tec", g["val"], g["weight"], g["piercepoints"],
           station_orders(g["ant_pos"], ref, int(g["order"])), ref, SF_SCREEN_TEC,
           int(g["niter"]))
    for name in ("tec14", "wide_fit80tec"):
        g = load(name)
        for case in ("ref", "noref"):
            ref = int(g[f"{case}_ref_ant"])
            yield (f"{name}:{case}", g["val"], g["weight"], g["piercepoints"],
                   station_orders(g["ant_pos"], ref, int(g["order"])), ref,
                   SF_SCREEN_TEC, int(g["niter"]))
    for name in ("ties4amp", "gain12", "wide_fit80amp"):
        g = load(name)
        val, w = stack_pols(g["amp_val"]), stack_pols(g["amp_weight"])
        yield (name, val, w, g["piercepoints"],
               [int(g["amp_order"])] * val.shape[2], -1, SF_SCREEN_AMPLITUDE,
               int(g["niter"]) if "niter" in g else 3)
    s = make_solutions(n_ant=3, n_time=4, n_freq=1, n_dir=96, seed=4096,
                       flag_frac=0.05, outlier_frac=0.005, tiny_weight_frac=0.1)
    pp, _, _ = geometry.piercepoints(s.dir_radec)
    sys.path.insert(0, REPO)
    from oracle import kl as okl
    ref = okl.reference_station(s.weight)
    yield ("wide_tiny96", s.val, s.weight, pp, station_orders(s.ant_pos, ref, 20),
           ref, SF_SCREEN_PHASE, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_digest.py needs a GPU")
    dev = torch.device("cuda", 0)
    ctx = get_context(0)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    print(f"# library {library_identity()}", file=sys.stderr)
    lines = []
    for name, val, weight, pp, st, ref, screen_type, niter in cases():
        T, F, A, D = val.shape
        wide = D > SF_MAX_DIR
        (ctx.set_basis_wide if wide else ctx.set_basis)(pp)
        ph = torch.from_numpy(np.ascontiguousarray(val, np.float64)).to(dev)
        wt = torch.from_numpy(np.ascontiguousarray(weight, np.float32)).to(dev)
        for tag, opt, for_wide in SETTINGS:
            n = niter
            if opt and wide != for_wide:
                continue
            if tag == "general":
                if screen_type == SF_SCREEN_AMPLITUDE:
                    continue
                if screen_type == SF_SCREEN_TEC:
                    n = 1
            coef = torch.full_like(ph, -7.0)
            resid = torch.full_like(ph, -7.0)
            w_out = torch.full_like(wt, -7.0)
            order = torch.full((T, F, A), -7, dtype=torch.int32, device=dev)
            if opt:
                ctx.set_option(opt[0], opt[1])
            try:
                ctx.fit(ph, wt, T, F, A, st, screen_type=screen_type, niter=n,
                        ref_ant=ref, coef=coef, resid=resid, w_out=w_out,
                        order_out=order)
                torch.cuda.synchronize()
            finally:
                if opt:
                    ctx.set_option(opt[0], opt[2])
            for what, x in (("coef", coef), ("resid", resid), ("w_out", w_out),
                            ("order_out", order)):
                h = hashlib.sha256(np.ascontiguousarray(x.cpu().numpy()).tobytes())
                lines.append(f"{name} {tag} niter={n} {what} {h.hexdigest()}")
                print(lines[-1], flush=True)
            masks, entries = ctx.fit_pool_wide() if wide else ctx.fit_pool()
            h = hashlib.sha256(np.ascontiguousarray(masks).tobytes())
            h.update(np.ascontiguousarray(entries).tobytes())
            lines.append(f"{name} {tag} niter={n} pool[{len(masks)}] {h.hexdigest()}")
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf8") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
