#!/usr/bin/env python3
"""Which kernels do the DEFAULT plans of the four nets reach?  Planning needs no GPU:
    python tools/reach.py            -> markdown table (kernel symbol x net / batch), used by DESIGN.md §4
Batches 1 / 8 / 128 / 256 at 224x224; 128 and 256 also with `whole_batch_launches` (what bench.py plans under pipelining mode 2); `t` = batch 128
planned with further outputs (`taps=`: the last block of the last four stages and 'avgpool') — the only plans that reach `tap_kernel`.
    python tools/reach.py --opt fuse_irk=1 [--opt key=value ..]   -> the same table with these planning options on top of the defaults
(the fuse options that are off by default: fuse_irchain, fuse_dws, fuse_dws7, fuse_head_dws, fuse_bchain7, fuse_irk — `fuse_irk` reaches
no kernel on these four nets: none of them has a depthwise 5x5 / 7x7).
    python tools/reach.py --net resnext50_32x4d [--net NAME ..]   -> the table over the four nets AND these (topology.get names; a net with
grouped convs reaches `gconv3x3_kernel`: build_net sets `grouped = 1` by itself)."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from f8net_amd import synth, topology        # noqa: E402
from f8net_amd.net import build_net          # noqa: E402

NETS = ['resnet50', 'resnet18', 'mobilenet_v2', 'mobilenet_v1']
CASES = [(1, 0, 0), (8, 0, 0), (128, 0, 0), (128, 1, 0), (256, 1, 0), (128, 0, 1)]      # batch, whole_batch_launches, taps


def family(sym):
    return re.sub(r'<.*', '', sym.replace('f8::', ''))


def cli_options():
    opts = {}
    for i, a in enumerate(sys.argv):
        if a == '--opt' and i + 1 < len(sys.argv):
            k, v = sys.argv[i + 1].split('=')
            opts[k] = int(v)
    return opts


def cli_nets():
    return [sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == '--net' and i + 1 < len(sys.argv)]


def main():
    reach = {}
    extra = cli_options()
    for arch in NETS + cli_nets():
        spec = topology.get(arch, normalize=(arch == 'resnet50'))
        params = synth.reference_params(spec, seed=1234)
        stages = {b.name.rsplit('_layer_', 1)[0]: b.name for b in spec.blocks}
        for bs, whole, tapped in CASES:
            net = build_net(spec, params, max_batch=bs, hw=224, options=dict(extra, whole_batch_launches=1) if whole else (extra or None),
                            taps=list(stages.values())[-4:] + ['avgpool'] if tapped else ())
            whole = 'w' if whole else ('t' if tapped else '')
            for i in range(net.num_launches):
                k = net.launch_kernel(i)
                if k:
                    reach.setdefault(k, set()).add((arch, bs, whole))
    fams = {}
    for k, v in reach.items():
        fams.setdefault(family(k), []).append((k, v))
    print('| kernel family | instances reached | nets (batch sizes) |\n|---|---:|---|')
    for f in sorted(fams):
        inst = fams[f]
        where = {}
        for _, v in inst:
            for arch, bs, whole in v:
                where.setdefault(arch, set()).add(f'{bs}{whole}')
        txt = '; '.join(f'{a}: {", ".join(sorted(b, key=lambda x: (int(x.rstrip("wt")), x)))}' for a, b in sorted(where.items()))
        print(f'| `{f}` | {len(inst)} | {txt} |')
    if '-v' in sys.argv:
        for f in sorted(fams):
            for k, v in sorted(fams[f]):
                print(' ', k, sorted(v))


if __name__ == '__main__':
    main()
