"""The pure host helpers of the cube writers, no GPU: ``streaming.batch_rows``
(the rows-per-batch rule of every ``write_chunk`` and of ``KLScreen.sample``)
and ``make_aterm_images.padded_bounds`` (the bounds arguments of
``make_aterm_image`` and ``make_tec_aterm_image``)."""

import pytest

from ska_sdp_screen_fitting_amd.make_aterm_images import padded_bounds
from ska_sdp_screen_fitting_amd.streaming import batch_rows


def test_batch_rows():
    assert batch_rows(5, 1000, 999) == 1        # a row larger than the budget
    assert batch_rows(5, 1000, 1) == 1          # a budget of one byte
    assert batch_rows(5, 1000, 1 << 30) == 5    # never more than n_rows
    assert batch_rows(5, 1000, 5000) == 5
    assert batch_rows(6, 1000, 3000) == 3       # an exact divisor
    assert batch_rows(5, 1000, 2000) == 2       # 2, 2, 1
    assert batch_rows(5, 1000, 2999) == 2       # whole rows only
    assert batch_rows(1, 1000, 1 << 30) == 1
    assert isinstance(batch_rows(5, 1000, 2500.0), int)


BOUNDS = [124.565, 66.165, 127.895, 62.835]
MID = [126.23, 64.50]


def test_padded_bounds_list_and_string():
    caller = list(BOUNDS)
    got, mid = padded_bounds(caller, MID, 1.4)
    assert caller == BOUNDS and got is not caller  # the caller's list is kept
    pad_ra = (BOUNDS[2] - BOUNDS[0]) * 0.4
    pad_dec = (BOUNDS[3] - BOUNDS[1]) * 0.4
    assert got == pytest.approx([BOUNDS[0] - pad_ra, BOUNDS[1] - pad_dec,
                                 BOUNDS[2] + pad_ra, BOUNDS[3] + pad_dec], abs=1e-12)
    assert mid == MID
    text = "[" + ";".join(f" {v!r} " for v in BOUNDS) + "]"
    got_s, mid_s = padded_bounds(text, "[126.23; 64.50]", "1.4")
    assert got_s == got and mid_s == MID
    assert padded_bounds(tuple(BOUNDS), tuple(MID), 1.4)[0] == got


def test_padded_bounds_without_padding():
    caller = list(BOUNDS)
    got, _ = padded_bounds(caller, MID, None)
    assert got == BOUNDS and got is not caller
    assert padded_bounds(caller, MID, 1.0)[0] == BOUNDS
    # a fraction of 0 shrinks by the whole extent (what the tests' BOUNDS pass)
    got0, _ = padded_bounds(caller, MID, 0)
    assert got0[3] - got0[1] == pytest.approx(-(BOUNDS[3] - BOUNDS[1]), abs=1e-12)
    assert caller == BOUNDS
