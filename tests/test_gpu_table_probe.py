"""The byte kernels of f8_table.hip launched directly (tools/ubench/table_probe.hip, built by f8net_amd/csrc/build.sh) on sources whose pad bytes
are poisoned, every output byte of both forms compared with the lookup written out on the host, the output's pad bytes included, which a planned net
shows through no interface (its convs multiply them by zero weights): a real channel's byte is the byte table's entry at the stored byte ^ 0x80, pad
channels hold the format's zero (0x80 unsigned, 0 signed) whatever the source's pads hold — no entry of the probe's tables is that zero —, for the
replica counts 1, 4 and 16, V = 16 and V = 4 with its end mask; the fused channel gate takes the image of each lane's own pixel (three images of 49
pixels: waves span them).  The cases are written by hand."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = [(16, 1, 64), (16, 4, 48), (16, 16, 16), (4, 1, 20), (4, 4, 8), (4, 16, 61), (4, 1, 64)]              # (V, R, C)
CHMUL = [(16, 64, 0, 0), (16, 48, 1, 1), (4, 20, 1, 0), (4, 8, 0, 1), (4, 61, 0, 0)]                          # (V, C, a signed, b signed)


@pytest.mark.gpu
def test_real_channels_looked_up_and_pad_bytes_the_formats_zero():
    exe = os.path.join(ROOT, 'tools', 'ubench', 'table_probe.bin')
    assert os.path.exists(exe), 'run f8net_amd/csrc/build.sh (it builds the probe)'
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    got = [tuple(int(v) for v in m.groups()) for m in re.finditer(r'^table V=(\d+) R=(\d+) C=(\d+) mismatches=(-?\d+)$', r.stdout, re.M)]
    assert got == [c + (0,) for c in TABLE], r.stdout + r.stderr
    got = [tuple(int(v) for v in m.groups()) for m in re.finditer(r'^table\+chmul V=(\d+) C=(\d+) signs=(\d),(\d) mismatches=(-?\d+)$', r.stdout, re.M)]
    assert got == [c + (0,) for c in CHMUL], r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.rstrip().endswith('ok'), r.stdout + r.stderr
