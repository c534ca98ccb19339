"""fuse_irk (planning option, off by default) at op level, without a GPU: the option itself, the plan of every case of tests/irk_cases.py with
the option off (today's three launches) and on (the hand-written table), the kernel instances as exported symbols, the graph cuts of pass 1e3,
the shipped nets' plans, and the liveness of every case on the oracle's values."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import irk_cases
from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net

ALL = dict(irk_cases.CASES, max_batch=irk_cases.MAX_BATCH_CASE, pipelined=irk_cases.PIPELINED_CASE)


@functools.lru_cache(maxsize=None)
def _planned(name):
    case = ALL[name]
    return irk_cases.plan(name, case, irk_cases.make_input(name, case), 1)


# ---- the option
def test_option_defaults_to_0_is_range_checked_and_fixed_at_finalize():
    net = F8Net()
    assert net.get_option('fuse_irk') == 0
    L = _lib.lib()
    assert L.f8_net_set_option(net._h, b'fuse_irk', 2) == -1          # F8_ERR_INVALID
    assert L.f8_net_set_option(net._h, b'fuse_irk', -1) == -1
    assert L.f8_net_set_option(net._h, b'fuse_irk', 1) == 0 and net.get_option('fuse_irk') == 1
    g, _, _ = _planned('k5s1_9x11')
    assert L.f8_net_set_option(g.net._h, b'fuse_irk', 0) == -5        # F8_ERR_STATE
    with pytest.raises(Exception):
        g.net.set_option('fuse_irk', 0)


def test_environment_seeds_a_new_handle():
    code = 'from f8net_amd.net import F8Net; print(F8Net().get_option("fuse_irk"))'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env, want in (({}, '0'), ({'F8_FUSE_IRK': '1'}, '1')):
        base = {k: v for k, v in os.environ.items() if k != 'F8_FUSE_IRK'}
        out = subprocess.run([sys.executable, '-c', code], env=dict(base, **env), capture_output=True, text=True, check=True, cwd=root).stdout.split()
        assert out == [want]


def test_build_net_and_onnx_import_pass_the_option_on():
    """options={'fuse_irk': 1} reaches build_net and IntGraph.build_net (the four shipped nets have no such block: the plan does not move)."""
    from f8net_amd import onnx_export, onnx_import
    spec = topology.get('mobilenet_v2')
    params = synth.make_params(spec, 1)
    net = build_net(spec, params, max_batch=2, hw=64, options={'fuse_irk': 1})
    assert net.get_option('fuse_irk') == 1
    ig = onnx_import.import_graph(onnx_export.export_graph(onnx_export.graph_from_params(spec, params, hw=64)), input_signed=spec.normalize)
    x_fl = int(np.asarray(params['head.0.input_fraclen']).reshape(-1)[0]) if spec.normalize else 8
    net2 = ig.build_net(max_batch=2, hw=64, input_fraclen=x_fl, options={'fuse_irk': 1})
    assert net2.get_option('fuse_irk') == 1 and net2.describe() == net.describe()


# ---- the plans of the case table
def _off_tokens(case):
    """Today's plan, by hand: pre, then conv / dwconv<K>x<K>s<S> / conv per block, the readers, their adds, the output."""
    toks = []
    for b in case['blocks']:
        toks += ['conv1x1', f'dwconv{b["K"]}x{b["K"]}s{b["stride"]}', 'conv1x1']
    return toks


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    nb = len(case['blocks'])
    g, _, _ = _planned(name)
    assert irk_cases.fused_lines(g.net) == case['expect'], g.net.describe()
    assert sum('fused_irk' in ln for ln in g.net.describe().splitlines()) == nb, g.net.describe()
    assert not any(t.startswith('dwconv') for t in irk_cases.tokens(g.net))
    off, _, _ = irk_cases.plan(name, case, irk_cases.make_input(name, case), 0)
    assert 'fused_irk' not in off.net.describe() and not irk_cases.fused_lines(off.net)
    assert off.net.num_launches == g.net.num_launches + 2 * nb
    # conv, dwconv<K>x<K>s<S>, conv per block, behind `input` and `pre`
    toks = [t.split('s1_')[0] if t.startswith('conv1x1') else t for t in irk_cases.tokens(off.net)][2:2 + 3 * nb]
    assert toks == _off_tokens(case), off.net.describe()
    i = [k for k in range(g.net.num_launches) if g.net.launch_info(k, 1)[0].startswith('fused_irk')]
    for k in i:                                                  # essential lane operations: 3 per int8 value produced, 2 per joined value
        assert g.net.launch_valu(k, 1) > 0


def test_launch_valu_counts_the_existing_rule():
    """k5s1_9x11: 32 -> 192 -> 32 on 99 pixels, joined, one int8 reader form: 3 * (99 * 192 + 99 * 192) + 2 * 99 * 32 + 3 * 99 * 32."""
    g, _, _ = _planned('k5s1_9x11')
    k = [i for i in range(g.net.num_launches) if g.net.launch_info(i, 1)[0].startswith('fused_irk')][0]
    assert g.net.launch_valu(k, 1) == pytest.approx(3 * (99 * 192 * 2) + 2 * 99 * 32 + 3 * 99 * 32)
    assert g.net.launch_valu(k, 3) == pytest.approx(3 * (3 * (99 * 192 * 2) + 2 * 99 * 32 + 3 * 99 * 32))


def test_every_expected_kernel_is_an_exported_symbol_and_the_table_covers_the_instances():
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    names = {k for c in ALL.values() for _, k in c['expect']}
    for k in sorted(names):
        assert f'void {k}(f8::IRKArgs)' in syms, k
    shipped = {ln.split('void ')[1].split('(')[0] for ln in syms.splitlines() if 'void f8::fused_irk_kernel<' in ln}
    assert shipped == {irk_cases.kernel(K, cap, inst) for K in (5, 7) for cap in (96, 192, 320) for inst in (0, 2)}
    assert names == shipped


# ---- graph cuts of pass 1e3
def _cut(K=5, cin=32, cout=32, E=64, H=6, W=6, stride=1, pad=None, second_reader=None, net_output=None, join=None, reads_input=False, opts=None):
    """pre 1x1 -> expand -> depthwise K x K -> project [-> join] -> a 1x1 reader (the net output unless `net_output` names expand / dw).
    second_reader: 'expand' / 'dw' get a second 1x1 reader (joined into the output); join: 'input' (the block input) or 'other' (another conv).
    Returns the plan's tokens."""
    rng = np.random.default_rng(0)
    w = lambda *s: rng.integers(-20, 20, s).astype(np.int32)
    conv = lambda t, wt, **kw: net.conv(t, wt, None, **dict(dict(stride=1, pad=0, groups=1, weight_fl=6, input_fl=4, input_signed=True, quant_input=True,
                                                                 relu=False), **kw))
    pad = K // 2 if pad is None else pad
    net = F8Net()
    t = net.input(cin, H, W, 5)
    if not reads_input:
        t = conv(t, w(cin, cin, 1, 1))
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    other = conv(t, w(cout, cin, K, K), stride=stride, pad=pad) if join == 'other' else None     # recorded first: the project conv then hosts the join
    e = conv(t, w(E, cin, 1, 1), relu=True)
    d = conv(e, w(E, 1, K, K), stride=stride, pad=pad, groups=E, input_fl=6, input_signed=False, relu=True)
    p = conv(d, w(cout, E, 1, 1), input_fl=6, input_signed=False)
    if join == 'input':
        p = net.add(p, t)
    elif join == 'other':
        p = net.add(p, other)
    out = conv(p, w(32, cout, 1, 1))
    if second_reader:
        src = e if second_reader == 'expand' else d
        extra = conv(src, w(32, E, 1, 1), input_fl=6, input_signed=False)
        if second_reader == 'expand' and (Ho, Wo) != (H, W):
            extra = conv(extra, w(32, 1, K, K), stride=stride, pad=pad, groups=32)
        out = net.add(out, extra)
    net.output({'expand': e, 'dw': d}.get(net_output, out), as_float=False)
    net.set_option('fuse_irk', 1)
    for k, v in (opts or {}).items():
        net.set_option(k, v)
    net.finalize(2)
    return irk_cases.tokens(net)


def _fused(toks):
    return [t for t in toks if t.startswith('fused_irk')]


def _three(toks, K, stride=1):
    """the block as today's three launches"""
    return not _fused(toks) and f'dwconv{K}x{K}s{stride}' in toks


@pytest.mark.parametrize('K', [5, 7])
def test_graph_cuts(K):
    assert _fused(_cut(K)) == [f'fused_irk{K}_s1_G3']              # 36 pixels: G = 128 // 36
    assert _fused(_cut(K, join='input')) == [f'fused_irk{K}_s1_G3']
    assert _fused(_cut(K, stride=2)) == [f'fused_irk{K}_s2_G8']     # 9 pixels
    for pad in range(K // 2):                                       # pad < K / 2 stays three launches
        assert _three(_cut(K, H=9, W=9, pad=pad), K), pad
    assert _three(_cut(K, second_reader='expand'), K)               # a tapped intermediate: the expand result has a second reader
    assert _three(_cut(K, second_reader='dw'), K)
    assert _three(_cut(K, second_reader='dw', stride=2), K, 2)
    assert _three(_cut(K, net_output='expand'), K)                  # ... is a net output
    assert _three(_cut(K, net_output='dw'), K)
    assert _three(_cut(K, join='other'), K)                         # a join with something other than the block input
    assert _three(_cut(K, reads_input=True), K)                     # a block on the net input
    assert _three(_cut(K, cin=224, E=32), K)                        # irk_supported: block inputs up to 192 padded channels
    assert _fused(_cut(K, cin=192, E=32)) == [f'fused_irk{K}_s1_G3']
    assert _three(_cut(K, cout=352, E=32), K)                       # ... outputs up to 320
    assert _fused(_cut(K, cout=320, E=32)) == [f'fused_irk{K}_s1_G3']
    assert _three(_cut(K, H=2, W=130), K)                           # 130 > 128 output pixels of one row
    assert _fused(_cut(K, H=2, W=128)) == [f'fused_irk{K}_s1_R1']


def test_a_join_on_a_stride_2_block_stays_unfused():
    """Only on a 1 x 1 map does a stride-2 block's result have the shape of its input."""
    assert _fused(_cut(5, H=1, W=1, join='input')) == ['fused_irk5_s1_G8']
    assert _fused(_cut(5, H=1, W=1, stride=2)) == ['fused_irk5_s2_G8']
    assert _three(_cut(5, H=1, W=1, stride=2, join='input'), 5, 2)


def test_3x3_blocks_stay_fuse_irs():
    """K = 3 / pad 1 is pass 1e's with the option on or off: the same plan, fused_ir where fuse_ir fuses and three launches where it does not."""
    for opts, H in (({'fuse_ir': 2}, 6), ({'fuse_ir': 1}, 6), ({'fuse_ir': 1}, 14), ({'fuse_ir': 0}, 14)):
        on = _cut(3, H=H, W=H, opts=opts)
        off = _cut(3, H=H, W=H, opts=dict(opts, fuse_irk=0))
        assert on == off and not _fused(on), (opts, H)
    assert any(t.startswith('fused_ir_s1') for t in _cut(3, opts={'fuse_ir': 2}))
    assert 'dwconv3x3s1' in _cut(3, opts={'fuse_ir': 1})               # 36 pixels: fuse_ir = 1 leaves small maps unfused, and so does this pass


def test_later_passes_find_the_depthwise_conv_claimed():
    """fuse_dws / fuse_dws7 / fuse_irchain run with the option on and leave the block alone."""
    for K in (5, 7):
        toks = _cut(K, H=14, W=14, opts={'fuse_dws': 1, 'fuse_dws7': 1, 'fuse_irchain': 1, 'fuse_ir': 2})
        assert _fused(toks) == [f'fused_irk{K}_s1_R7'] and not any('dws' in t or 'ir_chain' in t for t in toks)


@pytest.mark.parametrize('arch', ['resnet50', 'resnet18', 'mobilenet_v2', 'mobilenet_v1'])
def test_shipped_nets_keep_their_plans(arch):
    spec = topology.get(arch, normalize=arch == 'resnet50')
    params = synth.make_params(spec, 1)
    off = build_net(spec, params, max_batch=128, hw=224, options={'fuse_irk': 0})
    on = build_net(spec, params, max_batch=128, hw=224, options={'fuse_irk': 1})
    plain = build_net(spec, params, max_batch=128, hw=224)
    assert on.describe() == off.describe() == plain.describe()
    assert [on.launch_kernel(i) for i in range(on.num_launches)] == [off.launch_kernel(i) for i in range(off.num_launches)]


# ---- liveness
@pytest.mark.parametrize('name', sorted(ALL))
def test_liveness_on_the_oracle(name):
    """A dead signal hides a failure: the final value has more than 8 distinct values; every int8 tensor a depthwise, project, chained expand or
    reader conv reads has at least 16 distinct values and fewer than half of its entries at a clamp bound; a case that aims at a wrap or a
    large join shows that event in the oracle's values."""
    case = ALL[name]
    g, out, ids = _planned(name)
    assert np.unique(g.v[out][0]).size > 8
    assert len(g.taps) == sum(3 if i else 2 for i in range(len(case['blocks']))) + len(case['readers'] or [])
    for label, xq, sgn in g.taps:
        lo, hi = (-127, 127) if sgn else (0, 255)
        assert np.unique(xq).size >= 16, label
        assert ((xq == lo) | (xq == hi)).mean() < 0.5, label
    aim = case.get('aim')
    if aim == 'bias_big':
        b = case['blocks'][0]
        e, d = ids[0][0], ids[0][1]
        for t, n, chans in ((e, b['in_fl'] + b['w_fl'] - b['dw_in_fl'], (3, 7)), (d, b['dw_in_fl'] + b['dw_w_fl'] - b['pw_in_fl'], (5, 11))):
            r = g.raw[t].astype(np.int64)[:, list(chans)]           # the named channels
            assert (r > 2 ** 31 - 2 ** 13).any(), 'no accumulator next to 2^31'
            # the accumulator itself wrapped past 2^31, or the rounding add `v + 2^(n-1)` of the requantisation does
            assert (r < -2 ** 30).any() or (r + (1 << (n - 1)) > 2 ** 31 - 1).any(), 'nothing wraps'
    elif aim == 'join':
        assert (np.abs(g.v[ids[0][3]][0].astype(np.int64)) > 2 ** 30).any()
    else:
        assert aim is None
