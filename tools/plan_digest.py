#!/usr/bin/env python3
"""Digest of the planner's output over a matrix of (net, input size, max batch, option set): one line per configuration.

Planning touches no device, so this runs without a GPU.  A change that must not move any plan is checked by running the tool
on the library before and after it and comparing the two outputs with `diff` (F8NET_LIB selects the library, see f8net_amd/_lib.py):

    F8NET_LIB=/path/to/parent/libf8net.so python tools/plan_digest.py > parent.txt
    python tools/plan_digest.py > branch.txt && diff parent.txt branch.txt

Per configuration, through the public C ABI only: describe, arena_bytes, weight_bytes, num_launches, and for every launch
launch_info, launch_valu, launch_kernel, launch_grid (num_cu 0, 256, 64) and step_launches at N = 1 and N = max batch; num_parts.
A finalize that fails prints its status and message instead.  `--full` prints every query instead of the digest (to see WHAT moved).

`--cases` digests the op cases of tests/*_cases.py instead (concat, upsample, slice / shuffle, windowed pool, transposed conv: ops no shipped net
has), each at its default options and on the other legs of the options that steer it.  tests/golden/plan_digest_cases.txt holds that output of the
library before the gathers' planner code was folded; tests/test_plan_digest_cases.py compares.
"""
import argparse
import hashlib
import itertools
import os
import random
import sys
from concurrent.futures import ProcessPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARCHS = ['resnet18', 'resnet34', 'resnet50', 'resnet101', 'resnet152', 'mobilenet_v1', 'mobilenet_v2']
EXTRA_SIZES = [('mobilenet_v2', 64), ('mobilenet_v2', 320), ('resnet50', 220), ('resnet50', 212), ('resnet18', 96)]
BATCHES = [1, 2, 128, 256]

# the planning options of kOptKeys (f8_net.cpp): key -> (lo, hi)
PLANNING = {
    'split': (1, 4), 'fuse_blocks': (0, 1), 'fuse_stages': (-1, 7), 'fuse_dual': (0, 1), 'fuse_ds': (0, 1), 'fuse_opener': (0, 1),
    'fuse_fc': (0, 1), 'fuse_stem': (0, 1), 'fuse_input': (0, 1), 'fuse_ir': (0, 2), 'fuse_irchain': (0, 1), 'fuse_head2': (0, 1),
    'fuse_p12': (0, 1), 'fuse_chain': (0, 1), 'fuse_tail': (0, 1), 'fuse_chain7': (0, 1), 'fuse_pool': (0, 1), 'fuse_bchain': (0, 2),
    'fuse_bchain7': (0, 2), 'chain_stack': (0, 1), 'wreg': (0, 1), 's2wreg': (0, 1), 'wstat': (0, 1), 'wstat_min_tiles': (0, 1 << 20),
    'wstat_fast': (0, 1), 'patch3x3': (0, 1), 'dual_wide': (0, 1 << 30), 'deep_nk': (1, 1 << 20), 'bk128': (0, 1), 'dw_dot4': (0, 1),
    'dw_mma': (0, 1), 'stem_rows': (0, 1), 'opener_stg': (0, 1), 'requant_float': (0, 1), 'arena_copies': (0, 4), 'shared_streams': (0, 1),
    'whole_batch_launches': (0, 1), 'tap_tiled': (0, 1),
}
# keys added after the digest's matrix was fixed: each alone at every value, appended behind the matrix and only where the library under
# test knows the key — so a parent library yields exactly its old lines and the lines of a new key are additions (never part of the random mixes)
LATER = {'fuse_irk': (0, 1), 'grouped': (0, 2), 'igemm_tile': (0, 4), 'concat_i8': (0, 1), 'upsample_i8': (0, 1), 'sumpool_wide': (0, 2), 'chanmap_i8': (0, 1), 'fuse_shuffle': (0, 1), 'pixmap_i8': (0, 1), 'fuse_hgate': (0, 1), 'table_i8': (0, 1), 'fuse_table': (0, 2)}


def option_sets(defaults):
    """[(name, {key: value})]: the default; every planning option alone at each legal value (wide ranges: lo, hi, default +-1); the products of
    the options that gate each other; 64 seeded random combinations of the fuse_* options and the batch-cutting ones."""
    sets = [('default', {})]
    for k, (lo, hi) in PLANNING.items():
        vals = range(lo, hi + 1) if hi - lo <= 16 else sorted({lo, hi, max(lo, defaults[k] - 1), min(hi, defaults[k] + 1)})
        sets += [(f'{k}={v}', {k: v}) for v in vals if v != defaults[k]]

    def product(*keys):
        for vs in itertools.product(*[range(PLANNING[k][0], PLANNING[k][1] + 1) for k in keys]):
            sets.append((','.join(f'{k}={v}' for k, v in zip(keys, vs)), dict(zip(keys, vs))))
    product('fuse_chain', 'fuse_tail', 'fuse_chain7', 'fuse_opener', 'fuse_ds')
    product('fuse_bchain', 'fuse_bchain7')
    product('fuse_ir', 'fuse_irchain')
    product('fuse_head2', 'fuse_stem')
    for k in ('fuse_chain', 'fuse_tail', 'fuse_chain7', 'fuse_bchain', 'fuse_bchain7', 'fuse_irchain'):
        product('fuse_pool', k)
    rng = random.Random(20260)
    mixed = [k for k in PLANNING if k.startswith('fuse_')] + ['requant_float', 'chain_stack', 'split', 'whole_batch_launches']
    for n in range(64):
        o = {k: rng.randint(*PLANNING[k]) for k in mixed}
        sets.append((f'random{n}:' + ','.join(f'{k}={v}' for k, v in o.items()), o))
    return sets


def queries(net, max_batch):
    """Everything the public ABI tells about a finalized plan, as lines of text."""
    out = [net.describe(), f'arena={net.arena_bytes} weights={net.weight_bytes} launches={net.num_launches}']
    for N in sorted({1, max_batch}):
        out.append(f'N={N} parts={net.num_parts(N)}')
        for i in range(net.num_launches):
            grids = [net.launch_grid(i, N, cu) for cu in (0, 256, 64)]
            out.append(f'{i} {net.launch_info(i, N)!r} valu={net.launch_valu(i, N)!r} {net.launch_kernel(i)} grid={grids} launches={net.step_launches(i, N)}')
    return out


def plan_lines(job):
    """The output lines of one (arch, hw, max batch): every option set."""
    arch, hw, bs, full, only = job
    from f8net_amd import synth, topology
    from f8net_amd._lib import F8Error
    from f8net_amd.net import record_net
    spec = topology.get(arch, normalize=arch == 'resnet50')       # as bench.py builds them: the reference's learned fraclens where its logs hold them
    params = synth.reference_params(spec, seed=1234)
    probe = record_net(spec, params, hw)
    for k in PLANNING:
        probe.set_option(k, probe.get_option(k))                  # every key exists and is settable before finalize
    sets = option_sets({k: probe.get_option(k) for k in PLANNING})
    for k, (lo, hi) in LATER.items():
        try:
            dflt = probe.get_option(k)
        except F8Error:
            continue                                              # an older library
        sets += [(f'{k}={v}', {k: v}) for v in range(lo, hi + 1) if v != dflt]
    lines = []
    for name, opts in sets:
        if only and only not in name:
            continue
        net = record_net(spec, params, hw)
        for k, v in opts.items():
            net.set_option(k, v)
        head = f'{arch} hw={hw} bs={bs} [{name}]'
        try:
            net.finalize(bs)
        except F8Error as e:
            lines.append(f'{head} FAILED status={e.status}: {e}')
            continue
        q = queries(net, bs)
        kernels = sum(net.step_launches(i, bs) for i in range(net.num_launches))      # kernel launches of a run of bs images
        lines.append(f'{head} launches={net.num_launches} kernel_launches={kernels} arena={net.arena_bytes} sha256={hashlib.sha256(chr(10).join(q).encode()).hexdigest()[:24]}')
        if full:
            lines += ['    ' + l for l in '\n'.join(q).split('\n')]
    return lines


# --cases: the op-case modules of tests/ (none of the shipped nets has a concat, upsample, slice, shuffle, windowed pool or transposed conv) and
# the options that steer their plans; each module has make_input(name) and plan(name, x, max_batch=None, **opts)
CASE_MODULES = {'concat_cases': ['concat_i8'], 'upsample_cases': ['upsample_i8', 'concat_i8'], 'chanmap_cases': ['chanmap_i8', 'fuse_shuffle', 'concat_i8'],
                'avgpool_cases': ['sumpool_wide', 'upsample_i8', 'concat_i8'], 'deconv_cases': ['concat_i8']}


def case_lines(full=False, only=''):
    """One line per (module, case, option set): the default plan, then each steering option alone at its other values."""
    import importlib
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    lines = []
    for mod, keys in CASE_MODULES.items():
        m = importlib.import_module(mod)
        for name, c in m.CASES.items():
            x = m.make_input(name, 1)                              # one image records the graph; the plan is made for the case's batch
            dflt = m.plan(name, x, c['N'])[0].net
            sets = [('default', {})] + [(f'{k}={v}', {k: v}) for k in keys for v in range(LATER[k][0], LATER[k][1] + 1) if v != dflt.get_option(k)]
            for sname, opts in sets:
                head = f'{mod}.{name} bs={c["N"]} [{sname}]'
                if only and only not in head:
                    continue
                net = m.plan(name, x, c['N'], **opts)[0].net
                q = queries(net, c['N'])
                lines.append(f'{head} launches={net.num_launches} arena={net.arena_bytes} sha256={hashlib.sha256(chr(10).join(q).encode()).hexdigest()[:24]}')
                if full:
                    lines += ['    ' + l for l in '\n'.join(q).split('\n')]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--arch', action='append', help='only these architectures')
    ap.add_argument('--only', default='', help='only the option sets whose name contains this')
    ap.add_argument('--full', action='store_true', help='print every query under its configuration')
    ap.add_argument('--cases', action='store_true', help="the op cases of tests/*_cases.py instead of the shipped nets (--only: part of a line's head)")
    args = ap.parse_args()
    if args.cases:
        print('\n'.join(case_lines(args.full, args.only)))
        return
    jobs = [(a, hw, bs, args.full, args.only) for a, hw in [(a, 224) for a in ARCHS] + EXTRA_SIZES for bs in BATCHES
            if not args.arch or a in args.arch]
    with ProcessPoolExecutor(args.jobs) as ex:
        for lines in ex.map(plan_lines, jobs):
            print('\n'.join(lines), flush=True)


if __name__ == '__main__':
    main()
