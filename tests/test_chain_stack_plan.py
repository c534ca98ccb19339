"""Planning of the 14x14 stage chains over image pairs (option chain_stack, environment F8_CHAIN_STACK, default 1).  A pair is one 28-row map of
7 tiles (f8_chain.hip ChainCfg::STACKABLE); the stacking is a launch argument of the chain instance (ChainArgs::stack), so the planned kernel
symbol is the same with and without it.  The geometry is read through f8_net_launch_grid: (workgroups per tile column, groups, grid, images
per tile column) for a batch on a device with a given number of compute units."""
import re
import shutil
import subprocess

import pytest

from f8net_amd import _lib, synth, topology
from f8net_amd.net import build_net


def _nets(arch, **opts):
    spec = topology.get(arch, normalize=True)
    return build_net(spec, synth.reference_params(spec), max_batch=128, hw=224, options=opts)


def _stage2(net):
    idx = [i for i in range(net.num_launches) if net.launch_kernel(i).startswith('f8::chain_kernel<1024, 256, 14, 14, 4, ')]
    assert idx, [net.launch_kernel(i) for i in range(net.num_launches)]
    return idx


def test_resnet50_stage2_is_tiled_by_image_pairs():
    on, off = _nets('resnet50'), _nets('resnet50', chain_stack=0)
    (i,) = _stage2(on)
    assert on.launch_grid(i, 128) == (7, 32, 224, 2)               # 64 pairs on 32 groups of 7 tiles: 2 rounds on 224 CUs
    assert on.launch_grid(i, 128, 256) == (7, 32, 224, 2)
    (j,) = _stage2(off)
    assert off.launch_grid(j, 128) == (4, 64, 256, 1)              # 128 images on 64 groups of 4 tiles
    assert on.launch_grid(i, 3) == (7, 2, 14, 2)                    # odd batch: the last pair holds one image
    assert on.launch_grid(i, 1) == (7, 1, 7, 2)


def test_other_chains_are_not_stacked():
    on, off = _nets('resnet50'), _nets('resnet50', chain_stack=0)
    stage2 = set(_stage2(on))
    assert on.num_launches == off.num_launches
    for i in range(on.num_launches):
        g = on.launch_grid(i, 128)
        if i not in stage2:
            assert g == off.launch_grid(i, 128), (i, on.launch_info(i, 1)[0])
            assert g[3] in (0, 1), (i, g)
    assert on.describe() == off.describe()


def test_small_devices_fall_back_to_one_image_per_column():
    net = _nets('resnet50')
    (i,) = _stage2(net)
    assert net.launch_grid(i, 128, 7) == (7, 1, 7, 2)                # 7 slots still hold a pair
    assert net.launch_grid(i, 128, 6) == (4, 1, 4, 1)                # 6 do not: 4 tiles of one image
    assert net.launch_grid(i, 128, 4) == (4, 1, 4, 1)
    assert net.launch_grid(i, 128, 3)[1:3] == (0, 0)                  # and 3 cannot run the launch at all


@pytest.mark.parametrize('arch', ['resnet101', 'resnet152'])
def test_deep_resnets_stack_every_14x14_chain(arch):
    net = _nets(arch)
    idx = _stage2(net)
    assert len(idx) >= 2                                            # the TAIL chain and identity-first chains (kChainMaxBlocks cuts)
    assert any(', 1024, ' in net.launch_kernel(i) for i in idx), [net.launch_kernel(i) for i in idx]
    for i in idx:
        assert net.launch_grid(i, 128) == (7, 32, 224, 2), net.launch_kernel(i)
    off = _nets(arch, chain_stack=0)
    for i in _stage2(off):
        assert off.launch_grid(i, 128) == (4, 64, 256, 1)


@pytest.mark.parametrize('arch', ['resnet50', 'resnet101'])
def test_stacking_keeps_the_kernel_symbols(arch):
    on, off = _nets(arch), _nets(arch, chain_stack=0)
    ks = [on.launch_kernel(i) for i in range(on.num_launches)]
    assert ks == [off.launch_kernel(i) for i in range(off.num_launches)]
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('needs binutils nm')
    syms = subprocess.run([nm, '-C', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for k in ks:
        if re.match(r'f8::chain_kernel<', k):
            assert k + '(' in syms, k


def test_chain_stack_option_range():
    spec = topology.get('resnet50', normalize=True)
    p = synth.reference_params(spec)
    for v in (0, 1):
        build_net(spec, p, max_batch=3, hw=224, options={'chain_stack': v})
    with pytest.raises(Exception):
        build_net(spec, p, max_batch=3, hw=224, options={'chain_stack': 2})
