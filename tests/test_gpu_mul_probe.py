"""The byte kernels of f8_mul.hip launched directly (tools/ubench/mul_probe.hip, built by f8net_amd/csrc/build.sh) on operands whose pad bytes are
poisoned — the int8 rows of a and b, and the int32 gate rows of the fused instances —, every output byte of both forms compared with the product
written out on the host, the output's pad bytes included, which a planned net shows through no interface (its convs multiply them by zero weights):
the real channels are exact (round half to even, ties occur), pad channels hold the format's zero (0x80 unsigned, 0 signed) whatever the operands'
pads hold, and the broadcast takes the image of each lane's own pixel (three images of 49 pixels: waves span them).  The kernel instance of each
case is written by hand: V = 16 where C is a multiple of 16, else 4."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 'f8::mul_i8_kernel<%s, %s, %d>'
# (bcast, gate, C, a signed, b signed, relu) -> kernel
CASES = {(0, 0, 8, 0, 0, 0): K % ('false', 'false', 4), (0, 0, 20, 1, 0, 1): K % ('false', 'false', 4), (0, 0, 48, 0, 1, 0): K % ('false', 'false', 16),
         (0, 0, 64, 1, 1, 1): K % ('false', 'false', 16), (0, 0, 6, 1, 1, 0): K % ('false', 'false', 4),
         (1, 0, 8, 1, 0, 0): K % ('true', 'false', 4), (1, 0, 20, 0, 0, 0): K % ('true', 'false', 4), (1, 0, 48, 1, 1, 1): K % ('true', 'false', 16),
         (1, 0, 64, 0, 1, 0): K % ('true', 'false', 16),
         (1, 1, 8, 0, 0, 0): K % ('true', 'true', 4), (1, 1, 20, 1, 0, 1): K % ('true', 'true', 4), (1, 1, 48, 1, 0, 0): K % ('true', 'true', 16),
         (1, 1, 64, 0, 1, 0): K % ('true', 'true', 16)}


@pytest.mark.gpu
def test_real_channels_exact_and_pad_bytes_the_formats_zero():
    exe = os.path.join(ROOT, 'tools', 'ubench', 'mul_probe.bin')
    assert os.path.exists(exe), 'run f8net_amd/csrc/build.sh (it builds the probe)'
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    got = {tuple(int(m[i]) for i in range(1, 7)): (m[8], int(m[7]))
           for m in re.finditer(r'mul bcast=(\d) gate=(\d) C=(\d+) signs=(\d),(\d) relu=(\d) mismatches=(-?\d+) kernel=(.+)', r.stdout)}
    assert got == {k: (v, 0) for k, v in CASES.items()}, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
