#!/opt/conda/bin/python3.9
"""Golden header cards of the dTEC a-term cube: the reference's own
``make_template_image(..., aterm_type="tec")`` (utils/processing_utils.py:
144-292) run under the conda interpreter (same shims as make_golden.py), the
file read back with astropy and its cards stored as data, in order:

* "t3f1a2_5x5": 3 times (a shorter last interval), 1 frequency (CDELT 1e8),
  2 antennas, 5 x 5 pixels;
* "t1f2a3_4x6": 1 time (CDELT 1.0), 2 frequencies, 3 antennas, nx = 6, ny = 4.

Each case holds its inputs beside the cards, so the test needs nothing else.

Usage:  /opt/conda/bin/python3.9 tests/golden/make_golden_tec_header.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (applies the shims)

import numpy as np  # noqa: E402

CASES = {
    "t3f1a2_5x5": dict(rad=126.23, dec=64.5, nx=5, ny=5, cellsize_deg=0.2,
                       freqs=[1.3e8], times=[4.9e9, 4.9e9 + 8.0, 4.9e9 + 12.0],
                       n_ant=2),
    "t1f2a3_4x6": dict(rad=10.75, dec=-30.25, nx=6, ny=4, cellsize_deg=0.05,
                       freqs=[1.2e8, 1.25e8], times=[4.9e9], n_ant=3),
}


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, c in CASES.items():
            path = os.path.join(tmp, name + ".fits")
            mg.misc.make_template_image(
                path, c["rad"], c["dec"], ximsize=c["nx"], yimsize=c["ny"],
                cellsize_deg=c["cellsize_deg"], freqs=np.array(c["freqs"]),
                times=np.array(c["times"]),
                antennas=[f"A{i}" for i in range(c["n_ant"])], aterm_type="tec")
            cards = [(k, v if not isinstance(v, bool) else int(v))
                     for k, v in mg.header_cards(path)]
            shape = list(mg.pyfits.getdata(path).shape)
            out[name] = dict(c, cards=cards, shape=shape)
            print(name, shape, len(cards), "cards")
    with open(os.path.join(HERE, "tec_header.json"), "w") as fh:
        json.dump(out, fh, indent=0)


if __name__ == "__main__":
    main()
