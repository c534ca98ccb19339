"""The CPU reference values of the op cases are the recorded ones: one digest per case of the seven case modules that have `reference(name)`, against
tests/golden/case_reference_digest.txt.  The file was produced by the per-module `_Graph` classes that tests/refgraph.py replaced (the commit before
RefGraph existed), so it holds RefGraph and tests/ref_ops.py to the values those computed.  No GPU.

To regenerate (only where a case table or a reference changes on purpose):  python tests/test_case_reference_digest.py > tests/golden/case_reference_digest.txt"""
import hashlib
import importlib
import os

import numpy as np

MODULES = ('concat_cases', 'upsample_cases', 'avgpool_cases', 'deconv_cases', 'chanmap_cases', 'mul_cases', 'table_cases')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'case_reference_digest.txt')


def digest_lines():
    """`module.case sha256[:24]` over the concatenated bytes of every output array of reference(name), in output order."""
    lines = []
    for mod in MODULES:
        m = importlib.import_module(mod)
        for name in sorted(m.CASES):
            g, outs, _ = m.reference(name)
            h = hashlib.sha256()
            for o in outs:
                h.update(np.ascontiguousarray(g.v[o][0]).tobytes())
            lines.append(f'{mod}.{name} {h.hexdigest()[:24]}')
    return lines


def test_reference_values_of_every_case_are_the_recorded_ones():
    want = open(GOLDEN).read().splitlines()
    got = digest_lines()
    assert [l.split()[0] for l in got] == [l.split()[0] for l in want]
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:5]


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print('\n'.join(digest_lines()))
