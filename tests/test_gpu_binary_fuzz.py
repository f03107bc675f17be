"""A bounded run of the --binary draw of the differential fuzzer (scripts/fuzz_vs_scipy.py): 1500 seeded random calls of
every binary_* function on real masks, judged bit for bit against the plain NumPy reference of tests/helpers/binary_ref.py
(which tests/test_binary_yardstick.py holds against SciPy).

The run is host bound (many tiny launches), so its wall time varies with the machine's load.  NOT YET MEASURED on an
MI355X: the time budget handed to the script (240 s) is the one of the --measure run of the same size
(tests/test_gpu_measure_fuzz.py) and has to be replaced by three times the first measured wall time."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bounded_binary_fuzz(gpu):
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_vs_scipy.py"), "--binary", "240", "7", "1500"],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    tail = "\n".join(proc.stdout.splitlines()[-25:])
    assert proc.returncode == 0, tail
    m = re.search(r"binary: cases (\d+), failures (\d+), per op (\{.*\})", proc.stdout)
    assert m, tail
    assert int(m.group(1)) >= 1500 and int(m.group(2)) == 0, tail
    for name in ("erosion", "dilation", "opening", "closing", "hit_or_miss", "propagation", "fill_holes"):
        assert "'%s'" % name in m.group(3), tail
