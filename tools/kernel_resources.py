#!/usr/bin/env python3
"""One sorted line per kernel symbol from the -Rpass-analysis=kernel-resource-usage remarks of a build (f8net_amd/csrc/build.sh
writes them to build/f8_*.log): TotalSGPRs VGPRs AGPRs ScratchSize Occupancy SGPRs-Spill VGPRs-Spill LDS-Size.  Two builds compare with diff:
    python tools/kernel_resources.py [BUILD_DIR] > table.txt          (--no-sgprs leaves TotalSGPRs out: it follows the kernarg order)
"""
import glob
import os
import re
import sys

KEYS = ('TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'SGPRs Spill', 'VGPRs Spill', 'LDS Size')


def table(build_dir, keys=KEYS):
    rows, name = {}, None
    for log in sorted(glob.glob(os.path.join(build_dir, 'f8_*.log'))):
        for line in open(log, errors='replace'):
            m = re.search(r'remark: +(Function Name|' + '|'.join(KEYS) + r')(?: \[[^\]]*\])?: (\S+)', line)
            if not m:
                continue
            if m.group(1) == 'Function Name':
                name = m.group(2)
                rows[name] = {}
            elif name:
                rows[name][m.group(1)] = m.group(2)
    return ['%s %s' % (n, ' '.join('%s=%s' % (k.replace(' ', ''), v.get(k, '?')) for k in keys)) for n, v in sorted(rows.items())]


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--no-sgprs']
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'build')
    print('\n'.join(table(args[0] if args else root, KEYS[1:] if '--no-sgprs' in sys.argv else KEYS)))
