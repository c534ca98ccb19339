"""GPU parity of the stage chains of 14x14 maps tiled by image PAIRS (option chain_stack, f8_chain.hip ChainCfg::STACKABLE): a pair is one 28-row
map of 7 tiles, the 3x3 reads zeros across the seam between its two images, and an odd batch leaves one image in the last pair.  Both 14x14
chain forms — identity blocks only (ResNet-101 / -152) and opened by the join of a stride-2 block (TAIL, ResNet-50) — against the oracle's
IntBlock.forward, with the option on and off; whole networks at odd batches against the goldens and the oracle."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from f8net_amd import synth, topology
from f8net_amd.net import F8Net, build_net
from oracle import oracle

from test_gpu_chain import _params, _run_stage_chain, _stage

NS = [1, 2, 3, 64, 70, 131]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _stage2(net):
    return [i for i in range(net.num_launches) if net.launch_kernel(i).startswith('f8::chain_kernel<1024, 256, 14, 14, 4, ')]


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('stack', [0, 1])
@pytest.mark.parametrize('requant_float', [0, 1])
def test_identity_14x14_chain_matches_oracle(dev, N, stack, requant_float):
    _run_stage_chain(dev, (1024, 256, 14, 3, 1024, N), 'acc_shifts_left', 'int32_out' if N > 8 else 'int8_out',
                     options={'chain_stack': stack, 'requant_float': requant_float})


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('stack', [0, 1])
@pytest.mark.parametrize('requant_float', [0, 1])
def test_tail_14x14_chain_matches_oracle(dev, N, stack, requant_float):
    """A stride-2 opening block (28x28x512 -> 14x14x1024) whose join opens the chain, and two identity blocks behind it."""
    C, MID, HW, CIN0 = 1024, 256, 14, 512
    name = 'o.0'
    body = [topology.ConvSpec(name + '.body.0', CIN0, MID, 1, 1, 0, relu=True), topology.ConvSpec(name + '.body.2', MID, MID, 3, 2, 1, relu=True),
            topology.ConvSpec(name + '.body.4', MID, C, 1, 1, 0)]
    sc = topology.ConvSpec(name + '.shortcut.0', CIN0, C, 1, 2, 0)
    blocks = [topology.BlockSpec(name, body, sc, residual=True, post_relu=True)]
    idb, fls = _stage(C, MID, 2, C, 'acc_shifts_left')
    blocks += idb
    fls[name + '.body.0'], fls[name + '.body.2'], fls[name + '.body.4'], fls[name + '.shortcut.0'] = (4, 7), (3, 6), (3, 6), (4, 7)
    params = _params([c for b in blocks for c in b.body] + [sc], fls, 61, 'stack')
    x_fl = 9
    x = np.abs(synth.rand_normal_int(29, 'stackx', (N, CIN0, 2 * HW, 2 * HW), 60.0)).astype(np.int32)

    net = F8Net()
    net.set_option('chain_stack', stack)
    net.set_option('requant_float', requant_float)
    r = net.input(CIN0, 2 * HW, 2 * HW, x_fl)
    for b in blocks:
        xin = r
        for c in b.body:
            r = net.conv(r, params[c.key + '.weight'], params[c.key + '.bias'], stride=c.stride, pad=c.pad, groups=1,
                         weight_fl=fls[c.key][1], input_fl=fls[c.key][0], input_signed=False, quant_input=True, relu=c.relu)
        if b.shortcut is not None:
            c = b.shortcut
            xin = net.conv(xin, params[c.key + '.weight'], params[c.key + '.bias'], stride=2, pad=0, groups=1,
                           weight_fl=fls[c.key][1], input_fl=fls[c.key][0], input_signed=False, quant_input=True, relu=False)
        r = net.add(r, xin, relu=True)
    net.output(r, as_float=False)
    net.finalize(N)
    assert 'stage_chain_x3_tail' in net.describe(), net.describe()
    (i,) = _stage2(net)
    assert net.launch_grid(i, N)[3] == (2 if stack else 1)
    got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy().reshape(N, C, HW, HW)
    net.check()
    w, fl = x, x_fl
    for b in blocks:
        w, fl = oracle.block_forward(b, params, w, fl)
    assert net.output_fraclen == fl
    np.testing.assert_array_equal(got, w)


@pytest.mark.parametrize('arch', ['resnet50', 'resnet101'])
def test_whole_net_odd_batch_matches_oracle(dev, arch):
    spec = topology.get(arch, normalize=True)
    params = synth.make_params(spec, seed=5, fraclens=topology.R50_NVIDIA_FRACLENS if arch == 'resnet50' else None)
    N = 3
    x, fl = synth.make_input(spec, params, N, 224, seed=6)
    want = oracle.net_forward(spec, params, x, fl)
    for stack in (1, 0):
        net = build_net(spec, params, max_batch=N, hw=224, options={'chain_stack': stack})
        assert all(net.launch_grid(i, N)[3] == (2 if stack else 1) for i in _stage2(net))
        got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy()
        net.check()
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('arch', ['resnet50', 'resnet101'])
def test_whole_net_matches_reference_golden_with_and_without_stacking(arch, golden_dir, dev):
    """The goldens' 224x224 batch is ONE image: the stacked launch's only pair holds one image (its seam tile is the image's ragged tile)."""
    g = np.load(os.path.join(golden_dir, f'net_{arch}.npz'))
    spec = topology.get(arch, normalize=bool(g['normalize']))
    params = synth.reference_params(spec, seed=1234)
    x, _ = synth.make_input(spec, params, 1, 224, seed=7)
    for stack in (1, 0):
        net = build_net(spec, params, max_batch=1, hw=224, options={'chain_stack': stack})
        got = net.run(torch.from_numpy(x).to(dev)).cpu().numpy()
        np.testing.assert_array_equal(got, g['s1234_hw224_n1/logits'], err_msg=f'{arch} chain_stack={stack}')
