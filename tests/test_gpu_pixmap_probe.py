"""The byte-mode kernels of f8_pixmap.hip launched directly (tools/ubench/pixmap_probe.hip, built by f8net_amd/csrc/build.sh) on sources whose pad bytes
are poisoned, into destinations with a guard region in front of and behind them: every output byte is compared with the formulas of include/f8net.h
written out on the host — the output's pad bytes included, which a planned net shows through no interface (its convs multiply them by zero weights) —
and the guards are untouched.  A source's pad bytes never reach the output, pad channels hold the format's zero (0x80 unsigned, 0 signed), nothing is
written outside the tensor.  The (op, order, r, C) are the table of tests/pixmap_cases.py; the kernel instance of each is written by hand, and every
shape a specialised instance serves runs on the general kernel as well."""
import os
import re
import subprocess

import pytest

import pixmap_cases as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (op, order, r, C of the small side) -> the planned instance: DCR and C % 16 == 0: the run mover; CRD, r = 2 and C % 4 == 0: the transposer
PLANNED = {
    ('d2s', 'dcr', 2, 64): pm.RUN, ('d2s', 'crd', 2, 64): pm.TD, ('d2s', 'dcr', 2, 16): pm.RUN, ('d2s', 'crd', 2, 16): pm.TD,
    ('d2s', 'dcr', 2, 48): pm.RUN, ('d2s', 'crd', 2, 48): pm.TD, ('d2s', 'dcr', 2, 12): pm.GEN, ('d2s', 'crd', 2, 12): pm.TD,
    ('d2s', 'dcr', 2, 20): pm.GEN, ('d2s', 'crd', 2, 20): pm.TD, ('d2s', 'dcr', 2, 3): pm.GEN, ('d2s', 'crd', 2, 3): pm.GEN,
    ('d2s', 'dcr', 2, 19): pm.GEN, ('d2s', 'crd', 2, 19): pm.GEN, ('d2s', 'dcr', 2, 40): pm.GEN, ('d2s', 'crd', 2, 40): pm.TD,
    ('d2s', 'crd', 3, 3): pm.GEN, ('d2s', 'dcr', 3, 3): pm.GEN, ('d2s', 'crd', 3, 8): pm.GEN, ('d2s', 'dcr', 3, 8): pm.GEN,
    ('d2s', 'crd', 4, 16): pm.GEN, ('d2s', 'dcr', 4, 16): pm.RUN, ('d2s', 'crd', 8, 19): pm.GEN, ('d2s', 'dcr', 8, 19): pm.GEN,
    ('s2d', 'dcr', 4, 3): pm.GEN, ('s2d', 'crd', 4, 3): pm.GEN, ('s2d', 'dcr', 2, 3): pm.GEN, ('s2d', 'crd', 2, 3): pm.GEN,
    ('s2d', 'dcr', 2, 16): pm.RUN, ('s2d', 'crd', 2, 16): pm.TS, ('s2d', 'dcr', 2, 32): pm.RUN, ('s2d', 'crd', 2, 32): pm.TS,
    ('s2d', 'dcr', 2, 12): pm.GEN, ('s2d', 'crd', 2, 12): pm.TS, ('s2d', 'dcr', 2, 19): pm.GEN, ('s2d', 'crd', 2, 19): pm.GEN,
    ('s2d', 'dcr', 2, 40): pm.GEN, ('s2d', 'crd', 2, 40): pm.TS, ('s2d', 'dcr', 3, 8): pm.GEN, ('s2d', 'crd', 3, 8): pm.GEN,
}


def test_the_probe_covers_the_case_table():
    assert set(PLANNED) == set(pm.SHAPES)


@pytest.mark.gpu
def test_no_pad_byte_reaches_the_output_and_the_guards_are_untouched():
    exe = os.path.join(ROOT, 'tools', 'ubench', 'pixmap_probe.bin')
    assert os.path.exists(exe), 'run f8net_amd/csrc/build.sh (it builds the probe)'
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    got = [((m[1], m[2], int(m[3]), int(m[4])), m[5], int(m[6]), int(m[7]))
           for m in re.finditer(r'(d2s|s2d) order=(crd|dcr) r=(\d+) C=(\d+) kernel=(\S+) mismatches=(\d+) guard=(\d+)', r.stdout)]
    want = []
    for key, sym in PLANNED.items():
        want.append((key, sym, 0, 0))
        if sym != pm.GEN:
            want.append((key, pm.GEN, 0, 0))
    assert sorted(got) == sorted(want), r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
