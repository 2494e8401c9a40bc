"""Timing of the value-cube kernel (sf_kl_eval_values, kl_values.hip) on one
GPU, beside sf_kl_eval on its fp64 contraction and beside the only other route
to the same array (sf_kl_eval_point_values in batches of 4,096 positions).

    python tools/eval_values.py [--reps 7] [--out FILE]

Shapes: 256^2 at D = 20, 50, 80, 128 and 512^2 at D = 50.  Per shape the slot
count S is sized from a calibration launch so that a value launch takes
>= 50 ms; the output streams through an 8 GiB ring (the same buffer serves
sf_kl_eval with a quarter of the entries).  Per repetition every case runs
once, interleaved (drift hits all alike), after an untimed warm-up launch:
  values     sf_kl_eval_values, SF_EVAL_NAN_SCRUB, plain little-endian stores
  values-nt  the same with SF_EVAL_NT_STORES
  jones-f64  sf_kl_eval, SF_OPT_EVAL_INT = 0 (fp64 MFMA contraction), phase
             screens, SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS, plain stores
Reported per shape: median / min / max ms, ns per slot, algorithmic TB/s with
bytes = S (4 N^2 + 8 D) + 8 D N^2 and its fraction of 8 TB/s, achieved fp64
FLOP/s (2 D N^2 S) against the MFMA peak derived from profiles/mfma.json
(2048 flop per v_mfma_f64_16x16x4_f64 / cyc_per_mfma_f64 cycles x 1024 SIMDs x
2.4 GHz), and the fraction of the LOWER of the two rooflines (the larger of
the two bound times / measured time).
Condition 1: values ms <= jones-f64 ms + (max - min of the jones-f64 launches).
Condition 2 (256^2, D = 20, 16,384 slots, wall clock): the value kernel against
sf_set_points + sf_kl_eval_point_values per 4,096 positions + fp32 cast and
strided copy in torch; the two arrays are compared.
A ragged batch of every shape is first checked against fp64 numpy with the
tolerance of tests/test_values.py.  Exit status 1 when a condition fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-screen-fitting_amd"))
from ska_sdp_screen_fitting_amd import get_context  # noqa: E402
from ska_sdp_screen_fitting_amd._lib import (  # noqa: E402
    SF_EVAL_FAST_SINCOS, SF_EVAL_NAN_SCRUB, SF_EVAL_NT_STORES, SF_MAX_DIR,
    SF_MAX_POINTS, SF_OPT_EVAL_INT, library_identity)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--target-ms", type=float, default=60.0,
                help="value-launch time the slot count is sized for")
ap.add_argument("--out", default=None, help="also write the report here")
args = ap.parse_args()
if args.reps < 5:
    raise SystemExit("eval_values.py: at least 5 timed launches")

if not torch.cuda.is_available():
    raise SystemExit("eval_values.py needs a GPU: nothing is estimated")
dev = torch.device("cuda", 0)
ctx = get_context(0)
stream = torch.cuda.current_stream(dev)
ctx.set_stream(stream.cuda_stream)

with open(os.path.join(REPO, "profiles", "mfma.json"), encoding="utf8") as fh:
    cyc = [e["cyc_per_mfma_f64"] for e in json.load(fh)["entries"]
           if e.get("cyc_per_mfma_f64")]
PEAK = 2048.0 / min(cyc) * 1024 * 2.4e9   # flop/s
HBM = 8e12
C_SUM = 4e-15                              # tests/test_values.py

SHAPES = ((256, 20), (256, 50), (256, 80), (256, 128), (512, 50))
RING_BYTES = 8 * 2 ** 30
buf = torch.empty(RING_BYTES // 4, dtype=torch.float32, device=dev)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def geometry(N, D):
    rng = np.random.default_rng(D * 1000 + N)
    pp = np.stack([rng.uniform(-3000, 3000, D), rng.uniform(-3000, 3000, D),
                   np.zeros(D)], 1)
    return pp, np.linspace(-2000, 2000, N), rng


def select(N, D, pp, x):
    if D > SF_MAX_DIR:
        ctx.set_piercepoints(pp)
    else:
        ctx.set_basis(pp)
    ctx.set_grid(x, x)


def cpix_np(pp, x):
    gx, gy = np.meshgrid(x, x)
    d2 = ((pp[:, 0][None, :] - gx.reshape(-1, 1)) ** 2
          + (pp[:, 1][None, :] - gy.reshape(-1, 1)) ** 2 + pp[:, 2][None, :] ** 2)
    return -((d2 / 100.0 ** 2) ** (5.0 / 6.0)) / 2.0


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


V_FLAGS = SF_EVAL_NAN_SCRUB
J_FLAGS = SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS
ok = True
ctx.set_option(SF_OPT_EVAL_INT, 0)
try:
    say(f"library {library_identity()}  ring {RING_BYTES >> 30} GiB  reps {args.reps}  "
        f"fp64 MFMA peak {PEAK / 1e12:.1f} TFLOP/s ({min(cyc):.0f} cycles per MFMA, "
        f"profiles/mfma.json)  HBM {HBM / 1e12:.0f} TB/s")
    for N, D in SHAPES:
        pp, x, rng = geometry(N, D)
        select(N, D, pp, x)
        P = N * N
        # ---- check a ragged batch against fp64 numpy
        Sc = 37
        cc = rng.normal(0, 0.01, (Sc, D))
        o = torch.full((Sc, N, N), -7.0, dtype=torch.float32, device=dev)
        ctx.eval_values(torch.from_numpy(cc).to(dev), Sc, o, Sc, 0)
        torch.cuda.synchronize()
        cpix = cpix_np(pp, x)
        v = cc @ cpix.T
        err = np.abs(o.cpu().numpy().reshape(Sc, P).astype(np.float64) - v)
        tol = 2.0 ** -24 * np.abs(v) + C_SUM * (np.abs(cc) @ np.abs(cpix).T)
        say(f"check {N}^2 D={D}: max err / tol {float((err / tol).max()):.3f}")
        if not np.all(err <= tol):
            raise SystemExit("eval_values.py: output check failed")
        del o
        # ---- size S from a calibration launch
        ring_v = RING_BYTES // (4 * P)
        ring_j = RING_BYTES // (16 * P)
        out_v = buf[: ring_v * P].view(ring_v, N, N)
        out_j = buf[: ring_j * 4 * P].view(ring_j, 4, N, N)
        S0 = 8192
        c0 = torch.from_numpy(rng.normal(0, 0.01, (S0, D))).to(dev)
        ctx.eval_values(c0, S0, out_v, ring_v, V_FLAGS)
        t0 = min(timed(lambda: ctx.eval_values(c0, S0, out_v, ring_v, V_FLAGS))
                 for _ in range(3))
        S = max(int(np.ceil(args.target_ms / t0 * S0 / 1024.0)) * 1024, S0)
        coef = torch.from_numpy(rng.normal(0, 0.01, (S, D))).to(dev)
        # a short launch overstates the time per slot: size again at length
        t1 = min(timed(lambda: ctx.eval_values(coef, S, out_v, ring_v, V_FLAGS))
                 for _ in range(2))
        if t1 < args.target_ms:
            S = int(np.ceil(args.target_ms / t1 * S / 1024.0)) * 1024
            coef = torch.from_numpy(rng.normal(0, 0.01, (S, D))).to(dev)
        cases = {
            "values": lambda: ctx.eval_values(coef, S, out_v, ring_v, V_FLAGS),
            "values-nt": lambda: ctx.eval_values(coef, S, out_v, ring_v,
                                                 V_FLAGS | SF_EVAL_NT_STORES),
            "jones-f64": lambda: ctx.eval(coef, S, out_j, ring_j, J_FLAGS),
        }
        kern = f"{ctx.eval_kernel(J_FLAGS)} / {ctx.eval_contraction(J_FLAGS)}"
        res = {k: [] for k in cases}
        for rep in range(args.reps + 1):
            for name, fn in cases.items():
                fn()  # untimed warm-up
                t = timed(fn)
                if rep:
                    res[name].append(t)
        say(f"--- {N}^2 D={D}  S={S} slots/launch  rings {ring_v} / {ring_j} entries  "
            f"jones-f64 = {kern}")
        for name in cases:
            t = res[name]
            ms = float(np.median(t))
            per = 4 if name != "jones-f64" else 16
            nbytes = S * (per * P + 8 * D) + 8 * D * P
            flops = 2.0 * D * P * S
            t_store, t_mfma = nbytes / HBM, flops / PEAK
            bound = "stores" if t_store >= t_mfma else "MFMA"
            say(f"{name:10s} median {ms:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  "
                f"{ms * 1e6 / S:7.1f} ns/slot  {nbytes / (ms * 1e-3) / 1e12:6.3f} TB/s "
                f"({nbytes / (ms * 1e-3) / HBM:.3f} of 8 TB/s)  "
                f"{flops / (ms * 1e-3) / 1e12:6.2f} TFLOP/s ({flops / (ms * 1e-3) / PEAK:.3f} of peak)  "
                f"lower roofline: {bound}, fraction {max(t_store, t_mfma) / (ms * 1e-3):.3f}")
        tv, tj = float(np.median(res["values"])), float(np.median(res["jones-f64"]))
        spread = max(res["jones-f64"]) - min(res["jones-f64"])
        c1 = tv <= tj + spread
        ok &= c1
        say(f"condition 1 ({N}^2 D={D}): values {tv:.3f} ms vs jones-f64 {tj:.3f} ms "
            f"+ spread {spread:.3f} ms: {'PASS' if c1 else 'FAIL'}  (x{tj / tv:.2f})")
        del coef, c0

    # ---- condition 2: the parent's route to the same array, 256^2 D = 20
    N, D, S2 = 256, 20, 16384
    pp, x, rng = geometry(N, D)
    select(N, D, pp, x)
    P = N * N
    coef = torch.from_numpy(rng.normal(0, 0.01, (S2, D))).to(dev)
    gx, gy = np.meshgrid(x, x)
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1)
    out_k = buf[: S2 * P].view(S2, P)
    out_p = torch.empty((S2, P), dtype=torch.float32, device=dev)
    vals = torch.empty((S2, SF_MAX_POINTS), dtype=torch.float64, device=dev)

    def kernel_route():
        ctx.eval_values(coef, S2, out_k, S2, 0)
        torch.cuda.synchronize()

    def points_route():
        for p0 in range(0, P, SF_MAX_POINTS):
            ctx.set_points(xy[p0:p0 + SF_MAX_POINTS])
            ctx.eval_point_values(coef, S2, vals)
            out_p[:, p0:p0 + SF_MAX_POINTS] = vals.to(torch.float32)
        torch.cuda.synchronize()

    wall = {"values": [], "points": []}
    for rep in range(args.reps + 1):
        for name, fn in (("values", kernel_route), ("points", points_route)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            if rep:
                wall[name].append((time.perf_counter() - t) * 1e3)
    same = bool(torch.equal(out_k.view(torch.int32), out_p.view(torch.int32)))
    dmax = float((out_k - out_p).abs().max())
    tk, tp = float(np.median(wall["values"])), float(np.median(wall["points"]))
    c2 = tk < tp
    ok &= c2
    say(f"condition 2 (256^2 D=20, {S2} slots, wall clock incl. sync): values "
        f"{tk:.3f} ms (min {min(wall['values']):.3f} max {max(wall['values']):.3f}) vs "
        f"{P // SF_MAX_POINTS} x (sf_set_points + sf_kl_eval_point_values + cast / copy) "
        f"{tp:.3f} ms (min {min(wall['points']):.3f} max {max(wall['points']):.3f}): "
        f"{'PASS' if c2 else 'FAIL'}  (x{tp / tk:.1f}); arrays bit-equal: {same}, "
        f"max |d| {dmax:.3g}")
finally:
    ctx.set_option(SF_OPT_EVAL_INT, -1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf8") as fh:
            fh.write("\n".join(lines) + "\n")
sys.exit(0 if ok else 1)
