"""Longer soak of one family of tests/stress_cases.py on a GPU box (the first cases of each are what
`pytest -m gpu` runs as tests/test_gpu_stress.py).

    python tools/stress.py <tiles|lists|listbuild|seglists|counts> [cases] [first case]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import stress_cases as sc  # noqa: E402
from scoary_amd.engine import AssociationEngine  # noqa: E402

KINDS = ("tiles", "lists", "listbuild", "seglists", "counts")
if len(sys.argv) < 2 or sys.argv[1] not in KINDS:
    sys.exit(__doc__)
run_case = getattr(sc, sys.argv[1] + "_case")
eng = AssociationEngine(0)
cases = int(sys.argv[2]) if len(sys.argv) > 2 else 200
first = int(sys.argv[3]) if len(sys.argv) > 3 else 0      # cases are seeded by their number: a later range = new cases
bad = 0
for case in range(first, first + cases):
    ok, what = run_case(eng, case)
    bad += not ok
    print(case, what, "ok" if ok else "MISMATCH")
print("mismatching cases:", bad)
sys.exit(1 if bad else 0)
