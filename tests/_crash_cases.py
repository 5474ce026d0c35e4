"""The reference-pinned crash episodes of tests/golden/crash_modes.npz
(golden/make_crash_golden.py) and the error bit each exception maps to.

TEST INFRASTRUCTURE: shared by tests/test_oracle_crash_cpu.py (which pins the
oracle to the reference's raises) and tests/test_gpu_crash_modes.py (which
holds the device to the oracle on the same episodes).
"""
import json

import numpy as np

import _oracle

ERRF_ZERODIV, ERRF_NAN_ROUND = 1, 2  # include/lnw.h LNW_ERRF_*
EXC_BIT = {"ZeroDivisionError": ERRF_ZERODIV, "ValueError": ERRF_NAN_ROUND,
           "OverflowError": ERRF_NAN_ROUND}
FX = np.load(_oracle.GOLDEN + "/crash_modes.npz")
META = {m["name"]: m for m in json.loads(str(FX["meta"]))}
