"""GPU parity of the 7x7 BasicBlock cluster chain (f8_bcchain.hip, planning option fuse_bchain7): ResNet-18 / 34 stage 3 — the identity
blocks, optionally the JOIN of the stage-opening block in front, and the average pool behind — in one launch over clusters of eight
workgroups.  Bit for bit against the reference goldens and the oracle's IntBlock.forward applied block after block."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from f8net_amd import synth, topology
from f8net_amd.net import F8Net, build_net
from oracle import oracle


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cluster_lines(net):
    return [ln.split()[1] for ln in net.describe().splitlines() if 'basic_cluster_chain_x' in ln]


@pytest.mark.parametrize('arch', ['resnet18', 'resnet34'])
@pytest.mark.parametrize('value', [1, 2])
def test_reference_golden_logits(arch, value, golden_dir, dev):
    path = os.path.join(golden_dir, f'net_{arch}.npz')
    g = np.load(path)
    spec = topology.get(arch, normalize=bool(g['normalize']))
    params = synth.reference_params(spec, seed=1234)
    x, _ = synth.make_input(spec, params, 1, 224, seed=7)
    net = build_net(spec, params, max_batch=1, hw=224, options={'fuse_bchain7': value})
    lines = _cluster_lines(net)
    assert len(lines) == 1 and lines[0].endswith('+avgpool') and ('_ds:' in lines[0]) == (value == 2), net.describe()
    got = net.run(_t(x, dev)).cpu().numpy()
    net.check()
    np.testing.assert_array_equal(got, g['s1234_hw224_n1/logits'])


@pytest.mark.parametrize('arch,N', [('resnet18', 1), ('resnet18', 3), ('resnet18', 5), ('resnet34', 4)])
@pytest.mark.parametrize('value,rqf', [(1, 0), (2, 0), (2, 1)])
def test_fresh_seed_against_the_oracle(arch, N, value, rqf, dev):
    spec = topology.get(arch)
    params = synth.make_params(spec, seed=91)
    x, x_fl = synth.make_input(spec, params, N, 224, seed=5)
    net = build_net(spec, params, max_batch=N, hw=224, options={'fuse_bchain7': value, 'requant_float': rqf})
    assert len(_cluster_lines(net)) == 1, net.describe()
    got = net.run(_t(x, dev)).cpu().numpy()
    net.check()
    np.testing.assert_array_equal(got, oracle.net_forward(spec, params, x, x_fl))


# ---------------------------------------------------------------------------------------------------------------------------------
# stage-only graphs: [opening block (3x3 / 2 ReLU -> 3x3, 1x1 / 2 shortcut, join)] + identity blocks on 7x7 x 512 [+ the pool]
def _rand(seed, tag, shape, scale):
    return synth.rand_normal_int(seed, tag, shape, scale)


def _stage(nid, opener, variant, signed=False):
    """Blocks + fraclens.  variant: 'acc_shifts_left' (the block output's fraclen is lower: the conv result shifts left) or 'res_shifts_left'
    (every block raises the stream's fraclen: the stream shifts left); signed: the second 3x3s read a signed (symmetric) format."""
    C = 512
    blocks, fls = [], {}
    if opener:
        name = 'd.0'
        body = [topology.ConvSpec(name + '.body.0', C // 2, C, 3, 2, 1, relu=True), topology.ConvSpec(name + '.body.2', C, C, 3, 1, 1, signed_in=signed)]
        blocks.append(topology.BlockSpec(name, body, topology.ConvSpec(name + '.shortcut.0', C // 2, C, 1, 2, 0), residual=True, post_relu=True))
        if variant == 'acc_shifts_left':
            fls[name + '.body.0'], fls[name + '.body.2'], fls[name + '.shortcut.0'] = (4, 7), (3, 6), (4, 7)     # body 9 < shortcut 11
        else:
            fls[name + '.body.0'], fls[name + '.body.2'], fls[name + '.shortcut.0'] = (4, 7), (4, 7), (3, 6)     # shortcut 9 < body 11
    for k in range(nid):
        name = f'b.{k}'
        body = [topology.ConvSpec(name + '.body.0', C, C, 3, 1, 1, relu=True), topology.ConvSpec(name + '.body.2', C, C, 3, 1, 1, signed_in=signed)]
        blocks.append(topology.BlockSpec(name, body, None, residual=True, post_relu=True))
        if variant == 'acc_shifts_left':
            fls[name + '.body.0'], fls[name + '.body.2'] = (4, 7), (3, 5 + (k % 2))
        else:
            fls[name + '.body.0'], fls[name + '.body.2'] = (4, 7), (min(5 + k, 7), 7)
    return blocks, fls


def _params(convs, fls, seed, tag, big_bias=False):
    p = {}
    for c in convs:
        in_fl, w_fl = fls[c.key]
        p[c.key + '.weight'] = np.clip(_rand(seed, c.key + 'w' + tag, (c.cout, c.cin, c.k, c.k), 30.0), -127, 127).astype(np.int32)
        p[c.key + '.bias'] = _rand(seed + 1, c.key + 'b' + tag, (c.cout,), 2.0 ** (in_fl + w_fl)).astype(np.int32)
        if big_bias and c.key.endswith('body.2'):
            p[c.key + '.bias'][[1, 77]] = [2 ** 31 - 40, 2 ** 31 - 2 ** 10]     # the join wraps / reaches the clamp at 2^31 - 1
        p[c.key + '.weight_fraclen'] = np.array(w_fl, np.int32)
        p[c.key + '.input_fraclen'] = np.array([in_fl], np.int32)
    return p


def _run_stage(dev, N, nid, opener, value, variant='acc_shifts_left', pool=True, signed=False, big_bias=False, options=None, pipelined=False):
    C = 512
    HWI = 14 if opener else 7
    CIN = C // 2 if opener else C
    blocks, fls = _stage(nid, opener, variant, signed)
    convs = [c for b in blocks for c in b.body] + [b.shortcut for b in blocks if b.shortcut is not None]
    pre = topology.ConvSpec('pre.0', CIN, CIN, 1, 1, 0)
    fc = topology.ConvSpec('fc.0', C, 64, 1, 1, 0)
    fls['pre.0'], fls['fc.0'] = (4, 7), (2, 7)
    tag = f'{variant}{int(signed)}{int(opener)}'
    params = _params(convs + [pre, fc], fls, 51, tag, big_bias)
    x_fl = 9
    x = _rand(23, 'bcc' + tag, (N, CIN, HWI, HWI), 3.0e3).astype(np.int32)

    net = F8Net()
    net.set_option('fuse_bchain7', value)
    for k, v in (options or {}).items():
        net.set_option(k, v)
    t = net.input(CIN, HWI, HWI, x_fl)
    r = net.conv(t, params['pre.0.weight'], params['pre.0.bias'], stride=1, pad=0, groups=1, weight_fl=7, input_fl=4, input_signed=False,
                 quant_input=True, relu=True)
    for b in blocks:
        xin = r
        for c in b.body:
            r = net.conv(r, params[c.key + '.weight'], params[c.key + '.bias'], stride=c.stride, pad=c.pad, groups=1,
                         weight_fl=fls[c.key][1], input_fl=fls[c.key][0], input_signed=c.signed_in, quant_input=True, relu=c.relu)
        if b.shortcut is not None:
            c = b.shortcut
            xin = net.conv(xin, params[c.key + '.weight'], params[c.key + '.bias'], stride=2, pad=0, groups=1,
                           weight_fl=fls[c.key][1], input_fl=fls[c.key][0], input_signed=False, quant_input=True, relu=False)
        r = net.add(r, xin, relu=True)
    if pool:
        r = net.avgpool_sum(r, 6)
        # a 1x1 on the pooled vector: the pool is not the net output (as the classifier behind it in ResNet-18 / 34)
        r = net.conv(r, params['fc.0.weight'], params['fc.0.bias'], stride=1, pad=0, groups=1, weight_fl=7, input_fl=2, input_signed=False,
                     quant_input=True, relu=False)
    net.output(r, as_float=False)
    net.finalize(N)
    lines = _cluster_lines(net)
    fused = opener and value == 2
    assert len(lines) == 1 and lines[0].startswith(f'basic_cluster_chain_x{nid + (1 if fused else 0)}' + ('_ds:' if fused else ':')), net.describe()
    assert lines[0].endswith('+avgpool') == pool, net.describe()
    assert 'avgpool_sum' not in net.describe(), net.describe()

    w, fl = oracle._conv_layer(pre, params, x, x_fl)
    w = np.maximum(w, 0)
    for b in blocks:
        w, fl = oracle.block_forward(b, params, w, fl)
    if pool:
        w = oracle.avgpool_sum(w)
        w, fl = oracle._conv_layer(fc, params, w.reshape(N, C, 1, 1), fl + 6)
    if pipelined:
        net.set_pipelined(2)
        xt = _t(x, dev)
        outs = [torch.empty((N, 64), dtype=torch.int32, device=dev) for _ in range(3)]
        for k in range(3):
            net.run(xt, out=outs[k])
        torch.cuda.synchronize()
        net.check()
        got = [o.cpu().numpy().reshape(w.shape) for o in outs]
        for gg in got:
            np.testing.assert_array_equal(gg, w)
        return
    got = net.run(_t(x, dev)).cpu().numpy().reshape(w.shape)
    net.check()
    np.testing.assert_array_equal(got, w)
    if N > 2:
        got2 = net.run(_t(x[:N - 1], dev)).cpu().numpy().reshape((N - 1,) + w.shape[1:])
        net.check()
        np.testing.assert_array_equal(got2, w[:N - 1])


@pytest.mark.parametrize('nid,N', [(1, 3), (2, 5), (1, 130)])
@pytest.mark.parametrize('variant', ['acc_shifts_left', 'res_shifts_left'])
def test_opener_join_and_identity_blocks(dev, nid, N, variant):
    _run_stage(dev, N, nid, True, 2, variant)


@pytest.mark.parametrize('nid,N', [(1, 4), (2, 5), (3, 3), (2, 128)])
@pytest.mark.parametrize('variant', ['acc_shifts_left', 'res_shifts_left'])
def test_identity_blocks_only(dev, nid, N, variant):
    _run_stage(dev, N, nid, False, 1, variant)


@pytest.mark.parametrize('opener', [False, True])
def test_signed_formats_run_the_general_instance(dev, opener):
    _run_stage(dev, 5, 2, opener, 2 if opener else 1, 'res_shifts_left', signed=True)


@pytest.mark.parametrize('opener', [False, True])
def test_stage_output_without_the_pool(dev, opener):
    _run_stage(dev, 5, 2, opener, 2 if opener else 1, pool=False)


def test_join_at_the_int32_clamp(dev):
    _run_stage(dev, 3, 2, True, 2, pool=False, big_bias=True)


def test_bench_schedule_pipelined_and_split(dev):
    _run_stage(dev, 130, 1, True, 2, options={'split': 2, 'arena_copies': 3, 'pipeline_depth': 3}, pipelined=True)
