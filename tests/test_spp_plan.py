"""Stride-1 max pools on the LDS-tile kernel (option maxpool_tile) and the SPP / SPPF pyramid in one launch (option fuse_spp) without a GPU: the two
planning keys and what every case of tests/spp_cases.py plans on each leg.  tests/test_gpu_spp.py runs the cases on the device."""
import os
import subprocess

import pytest

import spp_cases as sc
from f8net_amd import _lib
from f8net_amd.net import F8Net


@pytest.mark.parametrize('key, env, top', [('maxpool_tile', 'F8_MAXPOOL_TILE', 2), ('fuse_spp', 'F8_FUSE_SPP', 1)])
def test_the_options_are_planning_keys(key, env, top, monkeypatch):
    assert F8Net().get_option(key) == 0 and [F8Net().set_option(key, v).get_option(key) for v in range(top + 1)] == list(range(top + 1))
    for bad in (-1, top + 1):
        with pytest.raises(_lib.F8Error):
            F8Net().set_option(key, bad)
    g, _, _ = sc.plan('one_pool', sc.make_input('one_pool'))
    with pytest.raises(_lib.F8Error):                                # a planning key: refused once the plan exists
        g.net.set_option(key, 1)
    monkeypatch.setenv(env, str(top))
    assert F8Net().get_option(key) == top


@pytest.mark.parametrize('name', sorted(sc.CASES))
def test_tokens_and_symbols_of_every_case(name):
    sc.reference(name)                                               # (asserts what the table promises about the data)
    x = sc.make_input(name)
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    for leg, opts in sc.LEGS.items():
        net = sc.plan(name, x, **opts)[0].net
        assert sc.lines(net) == sc.want(name, leg), (leg, net.describe())
        assert all(f' {sym}(f8::' in syms for _, sym in sc.lines(net))
    # both keys 0: the plan of a handle that never heard of them
    assert sc.plan(name, x, maxpool_tile=0, fuse_spp=0)[0].net.describe() == sc.plan(name, x)[0].net.describe()


def test_the_pyramid_is_one_launch_and_reports_its_own_figures():
    x = sc.make_input('spp_11x13_rev')
    nets = {leg: sc.plan('spp_11x13_rev', x, **opts)[0].net for leg, opts in sc.LEGS.items()}
    assert nets['P'].num_launches - nets['F'].num_launches == 3 and len(sc.lines(nets['P'])) == 4 and len(sc.lines(nets['F'])) == 1
    (i, _, _), = sc.launch_lines(nets['F'], 'spp')
    px, C = 11 * 13, 64
    # x read once, the four slices written once; doubling steps per byte: three levels of window 5 = 3 x 3 (1 + 1 + 2 + 1 = 5)
    assert nets['F'].launch_info(i, 1)[1] == px * C * 5 and nets['F'].launch_valu(i, 1) == px * C * 9
    (j, _, _), = sc.launch_lines(nets['T'], 'maxpool_')[2:]          # the stand-alone 13-window: x in, the pool out; 1 + 1 + 2 + 4 + 4 + 1: five steps
    assert nets['T'].launch_info(j, 1)[1] == nets['P'].launch_info(j, 1)[1] == px * C * 2 and nets['T'].launch_valu(j, 1) == px * C * 5
