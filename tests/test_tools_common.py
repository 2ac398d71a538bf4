"""The pure functions of tools/refbuild.py and tools/perf_common.py: nothing here compiles the reference or needs a GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import perf_common  # noqa: E402
import refbuild  # noqa: E402

LINK_STDERR = """\
/usr/bin/ld: /tmp/x/harness.o: in function `harness_run':
harness.c:(.text.harness_run+0x1c): undefined reference to `svt_aom_pack2d_src'
/usr/bin/ld: harness.c:(.text.harness_run+0x4a): undefined reference to `svt_av1_predict_intra_block'
/usr/bin/ld: /tmp/x/mode_decision.o: in function `pick':
mode_decision.c:(.text.pick+0x91): undefined reference to `svt_aom_pack2d_src'
/usr/bin/ld: /tmp/x/libxref.so: hidden symbol `svt_log' isn't defined
collect2: error: ld returned 1 exit status
"""


def test_undefined_symbols_of_a_failed_link():
    assert refbuild.undefined_symbols(LINK_STDERR) == ["svt_aom_pack2d_src", "svt_av1_predict_intra_block"]
    assert refbuild.undefined_symbols("collect2: error: ld returned 1 exit status\n") == []


def test_quartiles_of_seven_values():
    # sorted: 1 3 5 7 9 11 13; the exclusive method puts the quartiles of seven values at the 2nd, 4th and 6th
    assert perf_common.quartiles([5.0, 1.0, 9.0, 3.0, 7.0, 13.0, 11.0]) == dict(median=7.0, q1=3.0, q3=11.0, min=1.0, max=13.0)


def test_compare_names_what_differs():
    committed = {"same": np.arange(4, dtype=np.int32), "gone": np.zeros(2, np.uint8), "dtype": np.arange(3, dtype=np.int32),
                 "value": np.array([1, 2, 3], np.int16), "shape": np.zeros((2, 3), np.uint8)}
    made = {"same": np.arange(4, dtype=np.int32), "added": np.zeros(2, np.uint8), "dtype": np.arange(3, dtype=np.int64),
            "value": np.array([1, 2, 4], np.int16), "shape": np.zeros((3, 2), np.uint8)}
    assert refbuild.compare(committed, made) == ["added", "dtype", "gone", "shape", "value"]
    assert refbuild.compare(committed, dict(committed)) == []
