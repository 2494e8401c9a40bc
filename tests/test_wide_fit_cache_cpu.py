"""The mask cache of the wide fit: what the header and the binding declare
(SF_OPT_FIT_WIDE_CACHE / _POOL_MB / _POOL_MAX, sf_get_fit_pool_wide).  CPU
only; the kernels are checked in tests/test_wide_fit_cache.py."""

import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "screenfit.h")


@pytest.mark.parametrize("name, value", [("SF_OPT_FIT_WIDE_CACHE", 19),
                                         ("SF_OPT_FIT_WIDE_POOL_MB", 20),
                                         ("SF_OPT_FIT_WIDE_POOL_MAX", 21)])
def test_binding_constants_equal_the_header(name, value):
    from ska_sdp_screen_fitting_amd import _lib
    text = open(HEADER).read()
    m = re.search(rf"^#define\s+{name}\s+(\d+)\b", text, flags=re.M)
    assert m and int(m.group(1)) == value
    assert getattr(_lib, name) == value


def test_binding_declares_the_wide_pool():
    from ska_sdp_screen_fitting_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"^int\s+sf_get_fit_pool_wide\s*\(\s*sf_ctx\s*\*", text, flags=re.M)
    assert "sf_get_fit_pool_wide" in _lib.EXPORTED
    assert callable(_lib.Context.fit_pool_wide)
    lib = _lib.load_library()
    assert lib.sf_get_fit_pool_wide(None, None, None, 0, None) == -22
