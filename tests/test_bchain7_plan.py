"""fuse_bchain7 (planning option, off by default): which 7x7 BasicBlock runs the planner puts in one cluster launch (f8_bcchain.hip), with
the stage-opening block's join in front and the average pool behind; its geometry, kernel symbol and accounting (no GPU)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(arch, value=None, hw=224, mb=128, params=None, **opts):
    spec = topology.get(arch)
    if value is not None:
        opts['fuse_bchain7'] = value
    return build_net(spec, params or synth.reference_params(spec), max_batch=mb, hw=hw, options=opts)


def _cluster(net):
    return [i for i in range(net.num_launches) if 'basic_cluster_chain' in net.launch_info(i, 1)[0]]


def _names(net):
    return [net.launch_info(i, 1)[0] for i in range(net.num_launches)]


@pytest.mark.parametrize('arch', ['resnet18', 'resnet34'])
def test_option_off_is_todays_plan(arch):
    plain = _plan(arch)
    off = _plan(arch, 0)
    assert plain.get_option('fuse_bchain7') == 0
    assert plain.describe() == off.describe() and not _cluster(plain)


def test_environment_seeds_a_new_handle():
    code = ('from f8net_amd import synth, topology; from f8net_amd.net import build_net; s = topology.get("resnet18"); '
            'n = build_net(s, synth.make_params(s, 1), max_batch=4, hw=224); print(n.get_option("fuse_bchain7"), n.num_launches)')
    env = dict(os.environ, F8_FUSE_BCHAIN7='2')
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True, cwd=ROOT).stdout.split()
    assert out == ['2', '8']


def test_resnet18_value2_opener_join_identity_block_and_pool():
    net = _plan('resnet18', 2)
    names = _names(net)
    assert net.num_launches == 8, net.describe()
    cl = _cluster(net)
    assert len(cl) == 1
    assert names[cl[0]] == 'basic_cluster_chain_x2_ds:stage_3_layer_0.body.2..stage_3_layer_1.body.2+avgpool'
    assert not any(n.startswith('avgpool_sum') for n in names)
    assert names[cl[0] - 1] == 'conv3x3s2_wreg:stage_3_layer_0.body.0'          # the stride-2 body.0 stays a launch of its own
    assert names[cl[0] + 1].startswith('linear_dense')
    assert not any('stage_3' in n for i, n in enumerate(names) if i not in (cl[0], cl[0] - 1))


def test_resnet34_value2_has_every_stage3_block():
    net = _plan('resnet34', 2)
    names = [net.launch_info(i, 1)[0] for i in _cluster(net)]
    assert names == ['basic_cluster_chain_x3_ds:stage_3_layer_0.body.2..stage_3_layer_2.body.2+avgpool'], net.describe()
    assert 'avgpool_sum' not in net.describe()


def test_resnet18_value1_identity_blocks_only():
    net = _plan('resnet18', 1)
    assert net.num_launches == 10
    names = _names(net)
    assert [names[i] for i in _cluster(net)] == ['basic_cluster_chain_x1:stage_3_layer_1.body.0..stage_3_layer_1.body.2+avgpool']
    join = [l for l in net.describe().splitlines() if 'stage_3_layer_0.shortcut.0' in l]
    assert len(join) == 1 and '_res:' in join[0] and 'i32=1 i8=0' in join[0], net.describe()


def test_no_7x7_map_no_cluster_launch():
    net = _plan('resnet18', 2, hw=96, mb=4)
    assert not _cluster(net)
    assert _plan('resnet18', 2, hw=96, mb=4).describe() == _plan('resnet18', 0, hw=96, mb=4).describe()


def test_fuse_blocks_0_fuses_nothing():
    assert _plan('resnet18', 2, fuse_blocks=0).describe() == _plan('resnet18', 0, fuse_blocks=0).describe()


def _graph(C=512, HW=7, nblk=2, second_reader=False, value=2, signed=False, finalize=True):
    """Hand-built stage: pre conv, identity BasicBlocks on HW x HW x C, pool, a 1x1 classifier.  second_reader: a 1x1 also reads the stage output."""
    rng = np.random.default_rng(0)
    w = lambda *s: rng.integers(-20, 20, s).astype(np.int32)
    net = F8Net()
    net.set_option('fuse_bchain7', value)
    t = net.input(C, HW, HW, 9)
    r = net.conv(t, w(C, C, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=7, input_fl=4, input_signed=False, quant_input=True, relu=True)
    for _ in range(nblk):
        x = r
        r = net.conv(r, w(C, C, 3, 3), None, stride=1, pad=1, groups=1, weight_fl=7, input_fl=4, input_signed=False, quant_input=True, relu=True)
        r = net.conv(r, w(C, C, 3, 3), None, stride=1, pad=1, groups=1, weight_fl=7, input_fl=3, input_signed=signed, quant_input=True, relu=False)
        r = net.add(r, x, relu=True)
    p = net.avgpool_sum(r, 6)
    y = net.conv(p, w(64, C, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=7, input_fl=2, input_signed=False, quant_input=True, relu=False)
    if second_reader:
        z = net.conv(r, w(64, C, 1, 1), None, stride=1, pad=0, groups=1, weight_fl=7, input_fl=3, input_signed=False, quant_input=True, relu=False)
        y = net.add(y, net.avgpool_sum(z, 6))
    net.output(y, as_float=False)
    if finalize:
        net.finalize(4)
    return net


def test_hand_built_graph_runs_as_one_cluster_launch():
    net = _graph()
    cl = _cluster(net)
    assert len(cl) == 1 and re.match(r'basic_cluster_chain_x2:.*\+avgpool$', _names(net)[cl[0]]), net.describe()
    assert not any(n.startswith('avgpool_sum') for n in _names(net))


def test_refused_7x7_stage_not_512_wide():
    assert not _cluster(_graph(C=256))


def test_second_reader_keeps_the_pool_out_and_writes_output_forms():
    net = _graph(second_reader=True)
    cl = _cluster(net)
    assert len(cl) == 1 and not _names(net)[cl[0]].endswith('+avgpool')
    line = net.describe().splitlines()[cl[0]]
    assert 'i32=1' in line, line
    assert sum(n.startswith('avgpool_sum') for n in _names(net)) == 2


def test_option_is_fixed_at_finalize_and_range_checked():
    net = _graph(finalize=False)
    with pytest.raises(Exception):
        net.set_option('fuse_bchain7', 3)
    net.finalize(4)
    with pytest.raises(Exception):
        net.set_option('fuse_bchain7', 1)
    L = _lib.lib()
    assert L.f8_net_set_option(net._h, b'fuse_bchain7', 1) == -5          # F8_ERR_STATE
    fresh = F8Net()
    assert L.f8_net_set_option(fresh._h, b'fuse_bchain7', 3) == -1          # F8_ERR_INVALID
    assert L.f8_net_set_option(fresh._h, b'fuse_bchain7', 2) == 0


def test_launch_grid():
    net = _plan('resnet18', 2)
    i = _cluster(net)[0]
    tiles, groups, grid, stack = net.launch_grid(i, 128, 256)
    assert (groups, grid) == (32, 256)
    groups130 = -(-130 // 4)                               # 33 groups of four images on at most 32 clusters: two rounds, the fewest clusters
    rounds = -(-groups130 // 32)
    assert net.launch_grid(i, 130, 256)[1:3] == (-(-groups130 // rounds), 8 * -(-groups130 // rounds))
    assert net.launch_grid(i, 4, 256)[1:3] == (1, 8)
    assert net.launch_grid(i, 128, 4)[1:3] == (0, 0)


def test_kernel_names_and_instances():
    r18 = _plan('resnet18', 2)
    assert r18.launch_kernel(_cluster(r18)[0]) == 'f8::bcchain_kernel<2>'
    rf = _plan('resnet18', 2, requant_float=1)
    assert rf.launch_kernel(_cluster(rf)[0]) == 'f8::bcchain_kernel<2>'
    sg = _graph(signed=True, value=1)
    assert sg.launch_kernel(_cluster(sg)[0]) == 'f8::bcchain_kernel<0>'


def test_every_planned_kernel_name_is_a_symbol_of_the_library_with_the_option_on():
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('needs binutils nm')
    syms = subprocess.run([nm, '-C', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = set(re.findall(r'(?:void )?(f8::[A-Za-z0-9_]+(?:<[^()]*>)?)\(', syms))
    assert 'f8::bcchain_kernel<2>' in have and 'f8::bcchain_kernel<0>' in have
    for arch in ('resnet18', 'resnet34'):
        for value in (1, 2):
            for opts in ({}, {'requant_float': 1}):
                net = _plan(arch, value, **opts)
                for i in range(net.num_launches):
                    k = net.launch_kernel(i)
                    if k and 'bcchain' in k:
                        assert k in have, (arch, value, opts, k)


def test_launch_valu_and_ops_by_hand():
    net = _plan('resnet18', 2)
    i = _cluster(net)[0]
    px, C = 49.0, 512.0
    # TAIL join: 2 per value, block 1's int8 input: 3, its mid: 3, its join: 2; the pool adds 1 per summed value; one int8 output form of the pool (classifier's input)
    want = px * C * (2 + 3 + 3 + 2) + px * C + 3 * C
    assert net.launch_valu(i, 1) == pytest.approx(want)
    assert net.launch_valu(i, 128) == pytest.approx(128 * want)
    ops = 2 * px * (C * C * 9 * 3 + C * 256)                 # body.2 of the opener, both 3x3s of the identity block, the 1x1 / 2 shortcut
    assert net.launch_info(i, 1)[2] == pytest.approx(ops)
