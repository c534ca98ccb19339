#!/usr/bin/env python3
"""The table launches (f8_net_table, f8_table.hip) against a device-to-device copy of the same bytes: the byte gather for each replica count R, the
int32 mode against the byte mode, and the sigmoid gate fused into the channel gate against the two launches it replaces.

    python tools/ab_table.py [--reps 30] [--batch 128] [--md profiles/table_r15.md]

(a) replicas.  tools/ubench/table_probe.bin (a fresh process) launches table_i8_kernel<V, R> for R = 1, 4, 16 directly on EfficientNet-B0's activation
    shapes, one output form, random source bytes; median of 20 launches by HIP events.  Its bytes are the PADDED rows' (channels rounded up to 32:
    144 -> 160, 240 -> 256), what the launch really moves.  Behind the probe's table this process times `torch.Tensor.copy_` of the same padded bytes
    (median of 30) and prints each R's time over it.
(b) / (c).  Per row a net `input (8 ch) -> 1x1 conv to C (the map x) -> op -> 1x1 conv to 32 (an int8 reader)` is planned with split = 1 once per leg:
    swish rows   x -> swish table: table_i8 = 1 (`table_i8:`) and 0 (`table_i32:` on table_i32_kernel: int32 entries, requantised on the device; no int32 form is written here, nothing reads one)
    SE rows      x (ReLU) -> avgpool_sum -> linear C -> C -> sigmoid table -> channel gate of x: fuse_table = 2 (`table+chmul_i8:` on every size; 1, the default, fuses below 2^20 values an image by this measurement) and 0
                 (`table_i8:` on N x C bytes + `chmul_i8:`; the value is the SUM of the two steps' times)
The measured value is the step's own time from f8_net_run_profiled (HIP events around the launch).  The yardstick is `torch.Tensor.copy_` between two
device buffers sized so that the copy moves what the FIRST leg moves (its launch_info bytes: half read, half written), timed with events in the same
process, twice per repetition (copy, copy'): the gap between the two is the spread the ratios are to be read against.  Legs alternate inside one
process, `--reps` repetitions each after two warm-up runs; median (min .. max).  The outputs of a row's legs are compared bit for bit before anything
is timed.  There is no parent leg: the library before this entry point refuses the graphs."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                           # noqa: E402
import torch                                 # noqa: E402
from f8net_amd import synth, tables          # noqa: E402
from f8net_amd.net import F8Net              # noqa: E402

SHAPES = ((32, 112), (96, 112), (144, 56), (240, 28), (480, 14), (672, 14), (1152, 7))      # EfficientNet-B0: expanded channels @ map
ROWS = [('swish', 'swish', C, H) for C, H in SHAPES] + [('SE gate', 'se', C, H) for C, H in SHAPES]
TOKENS = ('table', 'chmul_')


def _w(seed, shape, sig):
    return np.clip(synth.rand_normal_int(seed, f'w{shape}', shape, sig), -127, 127).astype(np.int32)


def op_net(kind, C, H, N, opts):
    """Returns (net, [indices of the launches whose times are summed])."""
    net = F8Net().set_option('split', 1)
    for k, v in opts.items():
        net.set_option(k, v)
    x = net.input(8, H, H, 8)
    b = (synth.rand_normal_int(21, f'b.{C}', (C,), 2.0 ** 12) + (2 ** 13 if kind == 'se' else 0)).astype(np.int32)
    src = net.conv(x, _w(1, (C, 8, 1, 1), 14.0), b, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False,
                   relu=kind == 'se')                             # fraclen 13
    if kind == 'se':
        shift = 6 if H <= 8 else 8 if H <= 16 else 10 if H <= 32 else 12 if H <= 64 else 14      # log2 of the pooled pixels, rounded
        v = net.linear(net.avgpool_sum(src, shift), _w(2, (C, C), 40.0 / C ** 0.5), None, weight_fl=5, input_fl=4, input_signed=False, quant_input=True)
        gate = net.table(v, tables.sigmoid(5, True, 12), in_fl=5, in_signed=True, out_fl=12, label='gate')      # fraclen 9 read at +-4
        t = net.mul(src, gate, a_fl=4, a_signed=False, b_fl=8, label='op')                                      # 12
        rd = 5
    else:
        t = net.swish(src, in_fl=4, in_signed=True, out_fl=8, label='op')
        rd = 4
    net.output(net.conv(t, _w(40, (32, C, 1, 1), 8.0), None, stride=1, pad=0, groups=1, weight_fl=6, input_fl=rd, input_signed=kind != 'se'), as_float=False)
    net.finalize(N)
    steps = [i for i in range(net.num_launches) if net.launch_info(i, N)[0].startswith(TOKENS)]
    assert steps, net.describe()
    return net, steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--md', default=None, help='also append the table rows to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ab_table.py measures on the GPU'
    dev = torch.device('cuda:0')
    N = args.batch
    probe = subprocess.run([os.path.join(ROOT, 'tools', 'ubench', 'table_probe.bin'), 'bench', str(N)], capture_output=True, text=True, timeout=600)
    assert probe.returncode == 0, probe.stdout + probe.stderr
    ratios = ['| channels @ map | copy_ of the padded bytes us | R = 1 / copy | R = 4 / copy | R = 16 / copy |', '|---|---:|---:|---:|---:|']
    for row in probe.stdout.splitlines():
        f = [c.strip() for c in row.strip('|').split('|')]
        if len(f) != 6 or not f[1].isdigit():
            continue
        half = int(float(f[2]) * 1e6 / 2)                            # the probe reads and writes this many bytes
        a, b = torch.randint(0, 255, (half,), dtype=torch.uint8, device=dev), torch.empty((half,), dtype=torch.uint8, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us = []
        for r in range(32):
            e0.record()
            b.copy_(a)
            e1.record()
            e1.synchronize()
            if r >= 2:
                us.append(e0.elapsed_time(e1) * 1e3)
        cp = statistics.median(us)
        ratios.append(f'| {f[0]} | {cp:.1f} | ' + ' | '.join(f'{float(t) / cp:.2f}' for t in f[3:6]) + ' |')
        del a, b
    lines = [f'device: {torch.cuda.get_device_name(0)}  batch {N}  reps {args.reps}', '', '(a) replicas: table_i8_kernel<V, R>, launched directly', '',
             probe.stdout.rstrip(), ''] + ratios + ['', '(b) table_i32 against table_i8, (c) table+chmul against two launches (MB moved here is ALGORITHMIC: real channels only)', '',
             '| row | leg | plan tokens | kernels | µs median (min .. max) | MB moved (algorithmic) | GB/s | leg / copy |', '|---|---|---|---|---|---:|---:|---:|']
    print('\n'.join(lines), flush=True)
    for title, kind, C, H in ROWS:
        x = torch.from_numpy(synth.rand_uniform_int(5, f'x{H}', (N, 8, H, H), 0, 255).astype(np.int32)).to(dev)
        legs = (('fused', dict(fuse_table=2)), ('two', dict(fuse_table=0))) if kind == 'se' else (('i8', dict(table_i8=1)), ('i32', dict(table_i8=0)))
        nets, outs = {}, {}
        for leg, opts in legs:
            nets[leg] = op_net(kind, C, H, N, opts)
            for _ in range(2):                                       # warm-up (upload, code objects)
                outs[leg], _ = nets[leg][0].run_profiled(x)
            nets[leg][0].check()
        (la, _), (lb, _) = legs
        assert torch.equal(outs[la], outs[lb]), 'the two legs disagree'
        assert len(torch.unique(outs[la])) > 100, 'the row computes next to nothing'
        nbytes = int(sum(nets[la][0].launch_info(i, N)[1] for i in nets[la][1])) // 2      # the copy reads and writes this many: the first leg's bytes moved
        src = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def copy_us():
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3
        for _ in range(2):
            copy_us()
        us = {k: [] for k in (la, 'copy', lb, "copy'")}
        for _ in range(args.reps):
            for leg, cp in ((la, 'copy'), (lb, "copy'")):
                net, steps = nets[leg]
                _, ms = net.run_profiled(x)
                us[leg].append(sum(ms[i] for i in steps) * 1e3)
                us[cp].append(copy_us())
        base = statistics.median(us['copy'] + us["copy'"])
        for leg in (la, lb, 'copy', "copy'"):
            med = statistics.median(us[leg])
            if leg in nets:
                net, steps = nets[leg]
                tok = ' + '.join(net.launch_info(i, N)[0].split(':')[0] for i in steps)
                moved = sum(net.launch_info(i, N)[1] for i in steps)
                kern = ' + '.join(net.launch_kernel(i) for i in steps)
            else:
                tok, moved, kern = '-', 2.0 * nbytes, 'torch.Tensor.copy_'
            row = (f'| {title}: {C} on {H} x {H} | {leg} | {tok} | {kern} | {med:.1f} ({min(us[leg]):.1f} .. {max(us[leg]):.1f}) | '
                   f'{moved / 1e6:.1f} | {moved / med / 1e3:.0f} | {med / base:.2f} |')
            print(row, flush=True)
            lines.append(row)
        del nets, outs, x, src, dst
    if args.md:
        with open(args.md, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
