"""The plans of the op cases (tests/*_cases.py: concat, upsample, slice / shuffle, windowed pool, transposed conv) are those of the library before
the planner and executor code of the gathers was folded into one mode rule, emitter and walker: `tools/plan_digest.py --cases`, line for line
against tests/golden/plan_digest_cases.txt, which was recorded with that earlier library (F8NET_LIB).  No GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_digests_of_the_op_cases_are_the_parents():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import plan_digest
    want = open(os.path.join(ROOT, 'tests', 'golden', 'plan_digest_cases.txt')).read().splitlines()
    got = plan_digest.case_lines()
    assert len(want) > 400 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
