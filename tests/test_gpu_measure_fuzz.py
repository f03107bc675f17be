"""A bounded run of the --measure draw of the differential fuzzer (scripts/fuzz_vs_scipy.py): 1500 seeded random
cases of ndimage.label and of every labelled reduction, judged against SciPy and a host float64 reference with written
bounds (tests/helpers/measure_ref.py)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bounded_measure_fuzz(gpu):
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_vs_scipy.py"), "--measure", "240", "5", "1500"],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    tail = "\n".join(proc.stdout.splitlines()[-25:])
    assert proc.returncode == 0, tail
    m = re.search(r"measure: cases (\d+), failures (\d+)", proc.stdout)
    assert m, tail
    assert int(m.group(1)) >= 1500 and int(m.group(2)) == 0, tail
