#!/usr/bin/env python3
"""Mint tests/golden/timeline_2016.npz: the masks, priors and scales of 32 run dates of the 2016 campaign (every fourth day up to election
day) on the design of tests/golden/data_2016.npz, from the reference's CSVs through dataprep.build_timeline.  Data only.

  python scripts/make_timeline_fixture.py [reference data directory] [output file]
"""
import sys
from pathlib import Path

import numpy as np
import pandas as pd

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from us_potus_model_amd import dataprep, timeline  # noqa: E402

N_DATES, EVERY_DAYS = 32, 4


def run_dates():
    last = pd.Timestamp("2016-11-08")
    return [str((last - pd.Timedelta(days=EVERY_DAYS * k)).date()) for k in range(N_DATES - 1, -1, -1)]


def main(data_dir, out):
    design = dataprep.build_timeline(data_dir, 2016, run_dates())
    golden = dataprep.load_npz(ROOT / "tests" / "golden" / "data_2016.npz")["data"]
    for k, v in design["data"].items():      # the fixture indexes the polls of the committed 2016 design
        assert np.asarray(v).tobytes() == np.asarray(golden[k]).tobytes(), k
    timeline.save_fixture(out, design)
    print(out, "dates", design["run_dates"][0], "..", design["run_dates"][-1], "state polls kept", design["keep_state"].sum(1)[[0, -1]])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference/data", sys.argv[2] if len(sys.argv) > 2 else ROOT / "tests" / "golden" / "timeline_2016.npz")
