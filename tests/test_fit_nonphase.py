"""tec and amplitude fits on the kernels: every direction regime, the "same
bits" options, and station shards (ant_offset + ref_phase).

The inputs are the Runs of tests/nonphase_cases.py: the reference's own
unsharded tec / amplitude runs, and oracle-only runs at D = 8, 33, 60, 61 and
128 with T x D > 256 (the block pipeline of the non-phase screens --
kl_block_sigma_kernel -> kl_block_flag_kernel -> mask-table insert -> next
pass -- with its 256-thread loop over the block wrapping, the one-slot-per-
wave pass at D >= 33, both sides of SF_MAX_DIR, the wide fit full).
tests/test_fit_nonphase_cpu.py shows on the oracle that no slot of these
inputs is ill-conditioned or marginal, so no slot is excluded here.

A station shard must write the bytes of its slice of the unsharded fit.  For
tec with ref_ant = -1 (quirk Q15: referenced to the LAST station of the whole
soltab) that takes the global last station's values as ``ref_phase``; with
``ref_phase`` NULL the call's own last station is subtracted, which is the
unsharded result only for the shard that holds the global last station.

Tolerances: those at the top of tests/test_gpu_parity.py -- orders and
``w_out`` identical, |d coef| <= 1e-8 x max(1, |coef|max), |d resid| <= 1e-8;
byte equality among the options the ABI documents as "same bits" and between
a shard and its slice of the whole.
Needs an MI355X: every test is marked ``gpu``.
"""

from types import SimpleNamespace

import numpy as np
import pytest

import nonphase_cases as nc
import walk_cases as wc
from test_fit_walk import SAME_BITS, check, fit, options, same_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RUNS = nc.all_runs()
ORACLE_RUNS = nc.all_oracle_runs()
NARROW = [r for r in ORACLE_RUNS if nc.n_dir(r) <= 60]
WIDE = [r for r in ORACLE_RUNS if nc.n_dir(r) > 60]
TEC_REF = [r for r in RUNS if r.type == "tec" and r.ref >= 0]
TEC_NOREF = [r for r in RUNS if r.type == "tec" and r.ref == -1]
AMP = [r for r in RUNS if r.type == "amplitude"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx(dev):
    from ska_sdp_screen_fitting_amd import get_context
    c = get_context(0)
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    return c


def shard_fit(ctx, dev, r, a0, a1, **kw):
    """sf_kl_fit on stations a0..a1 of the Run with ant_offset = a0 (and the
    Run's ref_ant, unless given)."""
    part = SimpleNamespace(**vars(r))
    part.val, part.weight = r.val[:, :, a0:a1], r.weight[:, :, a0:a1]
    part.st = r.st[a0:a1]
    part.ref = kw.pop("ref_ant", r.ref)
    kw.setdefault("ant_offset", a0)
    return fit(ctx, dev, part, **kw)


def station_values(r, a, dev):
    """Device [T][F][D] values of station a: a ``ref_phase``."""
    return torch.from_numpy(np.ascontiguousarray(r.val[:, :, a, :])).to(dev)


def piece(full, a0, a1):
    return [x[:, :, a0:a1] for x in full]


# ------------------------------------------------- 1. the default pipeline

@pytest.mark.parametrize("r", RUNS, ids=wc.run_id)
def test_fit_vs_reference(ctx, dev, r):
    """Every run on the default pipeline (the wide fit above 60 directions)
    against the reference's own run (the oracle's for the oracle-only runs)."""
    got = fit(ctx, dev, r)
    check(got, wc.expected(r), wc.run_id(r))
    for f, a in r.skipped:
        assert not got[0][:, f, a].any() and not got[1][:, f, a].any()
        assert not got[3][:, f, a].any()
        same_bytes((got[2][:, f, a],), (r.weight[:, f, a],), "skipped block")


# ------------------------------------- 2. the options that keep every bit

@pytest.mark.parametrize("r", NARROW, ids=wc.run_id)
def test_fit_options_keep_every_bit(ctx, dev, r):
    """One slot per wavefront, the general layout, 1 and 4 waves per subset
    Jacobi and the deletion modes 2 and 3 write the bytes the defaults
    write; every subset basis by the Jacobi solve stays within tolerance."""
    base = fit(ctx, dev, r)
    check(base, wc.expected(r), wc.run_id(r))
    for o in SAME_BITS:
        with options(ctx, **o):
            same_bytes(fit(ctx, dev, r), base, (wc.run_id(r), o))
    with options(ctx, SUBSET_DELETION=0):
        check(fit(ctx, dev, r), wc.expected(r), wc.run_id(r) + " jacobi")


@pytest.mark.parametrize("r", WIDE, ids=wc.run_id)
def test_wide_fit_options_keep_every_bit(ctx, dev, r):
    """Above 60 directions: the mask cache off and a pool of one entry."""
    base = fit(ctx, dev, r)
    check(base, wc.expected(r), wc.run_id(r))
    for o in (dict(WIDE_CACHE=0), dict(WIDE_POOL_MAX=1)):
        with options(ctx, **o):
            same_bytes(fit(ctx, dev, r), base, (wc.run_id(r), o))


# --------------------------------------------- 3. shards equal the whole

@pytest.mark.parametrize("r", TEC_REF, ids=wc.run_id)
def test_tec_shards_with_a_reference_station(ctx, dev, r):
    """ref_ant >= 0: the reference read locally where the shard holds it,
    passed as ref_phase where it does not, and passed although the shard
    holds it."""
    full = fit(ctx, dev, r)
    check(full, wc.expected(r), wc.run_id(r))
    refph = station_values(r, r.ref, dev)
    for a0, a1 in nc.shards(r.val.shape[2]):
        want = piece(full, a0, a1)
        same_bytes(shard_fit(ctx, dev, r, a0, a1, ref_phase=refph), want,
                   (wc.run_id(r), a0, a1, "ref_phase"))
        if a0 <= r.ref < a1:
            same_bytes(shard_fit(ctx, dev, r, a0, a1), want,
                       (wc.run_id(r), a0, a1, "local"))
    # the reference is inside one shard and outside another
    inside = [a0 <= r.ref < a1 for a0, a1 in nc.shards(r.val.shape[2])]
    assert any(inside) and not all(inside)


@pytest.mark.parametrize("r", TEC_NOREF, ids=wc.run_id)
def test_tec_shards_without_a_reference_station(ctx, dev, r):
    """ref_ant = -1: ref_phase holds the values of the global last station,
    in every shard."""
    full = fit(ctx, dev, r)
    check(full, wc.expected(r), wc.run_id(r))
    A = r.val.shape[2]
    last = station_values(r, A - 1, dev)
    for a0, a1 in nc.shards(A):
        same_bytes(shard_fit(ctx, dev, r, a0, a1, ref_phase=last),
                   piece(full, a0, a1), (wc.run_id(r), a0, a1))
    # ... and in the unsharded call
    same_bytes(fit(ctx, dev, r, ref_phase=last), full, (wc.run_id(r), "whole"))


@pytest.mark.parametrize("r", AMP, ids=wc.run_id)
def test_amplitude_shards(ctx, dev, r):
    """Contiguous ranges of the pol-stacked station axis.  Amplitude is never
    referenced: ref_ant, ant_offset and ref_phase change no byte."""
    full = fit(ctx, dev, r)
    check(full, wc.expected(r), wc.run_id(r))
    junk = torch.from_numpy(np.ascontiguousarray(r.val[:, :, 0, :]) + 0.25).to(dev)
    for a0, a1 in nc.shards(r.val.shape[2]):
        want = piece(full, a0, a1)
        for kw in (dict(ant_offset=0), dict(), dict(ref_ant=a0),
                   dict(ref_ant=a1 - 1, ref_phase=junk),
                   dict(ref_ant=0, ref_phase=junk),
                   dict(ref_ant=-1, ref_phase=junk)):
            same_bytes(shard_fit(ctx, dev, r, a0, a1, **kw), want,
                       (wc.run_id(r), a0, a1, sorted(kw)))


@pytest.mark.parametrize("r", [x for x in nc.oracle_runs(33) if x.type == "tec"],
                         ids=wc.run_id)
def test_general_kernel_tec_shards(ctx, dev, r):
    """SF_OPT_FIT_GENERAL = 1 (kl_fit.hip; tec with a single pass)."""
    A = r.val.shape[2]
    refph = station_values(r, r.ref if r.ref >= 0 else A - 1, dev)
    with options(ctx, GENERAL=1):
        full = fit(ctx, dev, r, niter=1)
        check(full, wc.run_oracle(r, niter=1), wc.run_id(r) + " general niter 1")
        for a0, a1 in nc.shards(A):
            same_bytes(shard_fit(ctx, dev, r, a0, a1, niter=1, ref_phase=refph),
                       piece(full, a0, a1), (wc.run_id(r), a0, a1, "general"))


# ------------------------------------------ 4. NULL ref_phase stays pinned

@pytest.mark.parametrize("r", TEC_NOREF, ids=wc.run_id)
def test_null_ref_phase_is_the_calls_last_station(ctx, dev, r):
    """ref_ant = -1 and ref_phase = NULL: the call's own last station is
    subtracted -- the oracle on the shard alone -- which is not the unsharded
    result unless the shard holds the global last station."""
    full = fit(ctx, dev, r)
    A = r.val.shape[2]
    for a0, a1 in nc.shards(A):
        got = shard_fit(ctx, dev, r, a0, a1)
        check(got, nc.oracle_alone(r, a0, a1), f"{wc.run_id(r)} {a0}:{a1} alone")
        if a1 == A:
            same_bytes(got, piece(full, a0, a1), (wc.run_id(r), a0, a1))
        else:
            assert not np.array_equal(got[0], full[0][:, :, a0:a1])
            assert not np.array_equal(got[1], full[1][:, :, a0:a1])
