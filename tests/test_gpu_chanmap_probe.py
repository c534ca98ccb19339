"""The byte-mode kernels of f8_chanmap.hip launched directly (tools/ubench/chanmap_probe.hip, built by f8net_amd/csrc/build.sh) on sources whose pad
bytes are poisoned, every output byte compared with the gather written out on the host — the output's pad bytes included, which a planned net shows
through no interface (its convs multiply them by zero weights): bytes past a slice's last channel and a source's own pad bytes never reach the output,
and pad channels hold the format's zero (0x80 unsigned, 0 signed).  The slices and shuffles are the tables of tests/chanmap_cases.py and two aligned
slices that end inside a dword / at the source's last real channel; the kernel instance of each is written by hand."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT, LF = 'f8::slice_i8_kernel<true>', 'f8::slice_i8_kernel<false>'
S16, S4, S2, SG = 'f8::shuffle_i8_kernel<16>', 'f8::shuffle_i8_kernel<4>', 'f8::shuffle_i8_kernel<2>', 'f8::shuffle_i8_general_kernel'
SLICES = {(0, 58, 116): LT, (58, 58, 116): LF, (16, 32, 64): LT, (32, 16, 64): LT, (17, 30, 64): LF, (49, 15, 64): LF, (29, 29, 58): LF, (0, 1, 8): LT,
          (0, 17, 64): LT, (48, 10, 58): LT}
SHUFFLES = {(2, 64): S16, (2, 352): S16, (2, 24): S4, (2, 232): S4, (2, 116): S2, (2, 58): SG, (3, 24): SG, (4, 16): SG, (4, 48): SG, (8, 24): SG, (8, 256): SG}


@pytest.mark.gpu
def test_no_byte_past_the_gather_reaches_the_output():
    exe = os.path.join(ROOT, 'tools', 'ubench', 'chanmap_probe.bin')
    assert os.path.exists(exe), 'run f8net_amd/csrc/build.sh (it builds the probe)'
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sl = {(int(m[1]), int(m[2]), int(m[3])): (m[4], int(m[5])) for m in re.finditer(r'slice first=(\d+) channels=(\d+) C=(\d+) kernel=(\S+) mismatches=(\d+)', r.stdout)}
    sh = {(int(m[1]), int(m[2])): (m[3], int(m[4])) for m in re.finditer(r'shuffle groups=(\d+) C=(\d+) kernel=(\S+) mismatches=(\d+)', r.stdout)}
    assert sl == {k: (v, 0) for k, v in SLICES.items()}, r.stdout + r.stderr
    assert sh == {k: (v, 0) for k, v in SHUFFLES.items()}, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
