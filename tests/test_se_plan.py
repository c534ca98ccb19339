"""Option fuse_se (f8_se.hip) without a GPU: the key; per case of tests/se_cases.py the token, the symbol and launch_info, all by hand."""
import os
import subprocess

import pytest

import se_cases as sc
from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, record_net
from graph_cases import ROOT, plan_digest_tool


def test_the_key(monkeypatch):
    net = F8Net()
    assert net.get_option('fuse_se') == 0
    for v in (1, 2, 0):
        net.set_option('fuse_se', v)
        assert net.get_option('fuse_se') == v
    for bad in (-1, 3):
        with pytest.raises(_lib.F8Error):
            net.set_option('fuse_se', bad)
    monkeypatch.setenv('F8_FUSE_SE', '1')
    assert F8Net().get_option('fuse_se') == 1 and net.get_option('fuse_se') == 0      # the environment seeds new handles only


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_plan(name):
    c = sc.CASES[name]
    x = sc.make_input(name, 1)
    g, _, (p, f1, _) = sc.plan(name, x, c['N'], fuse_se=c['key'])
    on, off, rule = g.net, sc.plan(name, x, c['N'])[0].net, sc.plan(name, x, c['N'], fuse_se=1)[0].net
    kernels = lambda net: [net.launch_kernel(i) for i in range(net.num_launches)]
    if c['key'] == 2 or not c['sym']:                                                 # above the size rule with the key at 1, or no match: the three launches
        assert rule.describe() == off.describe() and kernels(rule) == kernels(off)
    if not c['sym']:
        return
    assert sc.lines(on) == [(sc.TOKEN, c['sym'])] and [t for t, _ in sc.lines(off)] == ['avgpool_sum:'], on.describe()
    assert on.num_launches == off.num_launches - 2
    # the pooled vector and fc1's result: no launch of the fused plan writes them (every launch is named by what it writes: a label, or t<tensor id>)
    names = [on.launch_info(i, 1)[0] for i in range(on.num_launches)]
    assert not [n for n in names if n.endswith((':fc1', f':t{p}', f':t{f1}'))], names
    # launch_info by hand: the map once at 4 B a value + fc2's forms; both weight sets (K padded to 16, outputs to 32, 4 B of bias each); 2 (C mid + mid C)
    (i,) = [i for i, n in enumerate(names) if n.startswith(sc.TOKEN)]
    C, mid, r16, r32 = c['C'], c['mid'], (lambda v: -(-v // 16) * 16), (lambda v: -(-v // 32) * 32)
    forms = {'hgate': 4, 'table': 1, 'both': 5}[c['tail']]
    want = c['H'] * c['W'] * r32(C) * 4 + r32(C) * forms + r32(mid) * (r16(C) + 4) + r32(C) * (r16(mid) + 4)
    assert on.launch_info(i, 1)[1:] == (want, 2.0 * (C * mid + mid * C))
    assert on.launch_valu(i, 1) == c['H'] * c['W'] * C + 3 * (C + mid) + 3 * r32(C) * (forms % 4)


def test_the_shipped_nets_plan_as_before_with_the_key_on():
    """None has an SE branch: describe(), the kernels and both sizes are the default plan's."""
    for arch in plan_digest_tool().ARCHS:
        spec = topology.get(arch)
        params = synth.reference_params(spec, seed=1234)
        plans = []
        for v in (0, 2):
            net = record_net(spec, params, 64)
            net.set_option('fuse_se', v)
            net.finalize(2)
            plans.append((net.describe(), [net.launch_kernel(i) for i in range(net.num_launches)], net.arena_bytes, net.weight_bytes))
        assert plans[0] == plans[1], arch


def test_the_example_with_its_switch(tmp_path):
    """examples/se_host.c --fuse-se: the option line through the C ABI; its se graph plans the one launch, every refusal probe still runs."""
    subprocess.check_call(['gcc', '-std=c99', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'examples', 'se_host.c'), _lib.LIB_PATH, '-o', tmp_path / 'se_host'])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(_lib.LIB_PATH) + ':/opt/rocm/lib:' + os.environ.get('LD_LIBRARY_PATH', ''))
    out = subprocess.run([tmp_path / 'se_host', '--fuse-se'], text=True, capture_output=True, env=env, check=True).stdout
    assert out.rstrip().endswith('ok') and out.count('avgpool+fc+fc:') == 1 and out.count('avgpool_sum:') == 2      # (the probe's pool, `shared`'s pool)
