#!/usr/bin/env python3
"""depth_to_space / space_to_depth: the planned byte instance of each shape against a device-to-device copy of the output's bytes, the general byte
kernel and the int32 mode (profiles/pixmap_r17.md).

The measurement itself is tools/ubench/pixmap_probe.bin --bench (built by f8net_amd/csrc/build.sh): it launches the kernels of f8_pixmap.hip directly,
which is the only way to run the general kernel on a shape the planner gives a specialised instance.  Per shape the four legs are interleaved in one
process, 7 rounds of 100 launches between two events after 10 warm-up launches each, on random bytes; it prints median / minimum microseconds per
launch.  The copy leg is hipMemcpyAsync device-to-device of the int8 output's bytes — what torch.Tensor.copy_ issues for two contiguous tensors of one
dtype — so that all legs run in one process.  The int32 leg reads the int32 source and writes one int8 form (ESPCN: the int32 form, a network output).

    python tools/ab_pixmap.py [--raw profiles/pixmap_r17_raw.txt] [--md profiles/pixmap_r17.md]

Batch 128; the DUC head at batch 32.  No tensor of these shapes passes 2 GiB at that batch (the largest, Focus's int32 source, is 1.7 GB).
Not measured: hardware counters, split > 1, whole-net throughput."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r'bench (\S+) op=(\S+) order=(\S+) r=(\d+) C=(\d+) map=(\d+)x(\d+) N=(\d+) out_bytes=(\d+) planned=(\S+) copy_us=([\d.]+)/([\d.]+) '
                  r'planned_us=([\d.]+)/([\d.]+) general_us=([\d.]+)/([\d.]+) i32_us=([\d.]+)/([\d.]+) i32_writes=(\S+)')


def table(raw):
    rows = ['| shape | op | planned instance | out MB | copy us | planned us | general us | int32 us | planned / copy | planned / general | int32 / planned |',
            '|---|---|---|---|---|---|---|---|---|---|---|']
    for m in LINE.finditer(raw):
        name, op, order, r, C, h, w, N, nbytes, sym = m.group(1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
        copy, planned, general, i32 = (float(m.group(k)) for k in (11, 13, 15, 17))      # medians
        rows.append(f'| {name} (C {C}, {h}x{w}, N {N}) | {op}{r}{order} | `{sym.replace("f8::", "")}` | {int(nbytes) / 1e6:.1f} | {copy:.1f} | {planned:.1f} | '
                    f'{general:.1f} | {i32:.1f} ({m.group(19)}) | {planned / copy:.2f} | {planned / general:.2f} | {i32 / planned:.2f} |')
    return '\n'.join(rows) + '\n'


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--raw', help='write the probe\'s output here')
    ap.add_argument('--md', help='write the table here')
    ap.add_argument('--from-raw', help='format an earlier raw output instead of measuring')
    args = ap.parse_args()
    if args.from_raw:
        raw = open(args.from_raw).read()
    else:
        exe = os.path.join(ROOT, 'tools', 'ubench', 'pixmap_probe.bin')
        r = subprocess.run([exe, '--bench'], capture_output=True, text=True, timeout=500)
        raw = r.stdout + r.stderr
        if r.returncode:
            sys.exit(raw)
    if args.raw:
        open(args.raw, 'w').write(raw)
    md = table(raw)
    if args.md:
        open(args.md, 'w').write(md)
    print(raw + '\n' + md)


if __name__ == '__main__':
    main()
