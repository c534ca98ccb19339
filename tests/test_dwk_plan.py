"""The general depthwise launches (dwconvk_dot4_kernel and dwconvk_kernel of f8_dwk.hip: kernel 3 / 5 / 7, stride 1 / 2, pad 0 .. kernel / 2 — all
but 3x3 / pad 1) at op level, without a GPU: what the builder accepts and refuses, the plan of every case of tests/dwk_cases.py against the
hand-written table on both legs, the kernel instances as exported symbols, the 3x3 / pad 1 plans and the fusion passes left as they were, and the
liveness of every case on the oracle's values."""
import functools
import os
import subprocess

import numpy as np
import pytest

import dw_cases
import dwk_cases
from f8net_amd import _lib
from f8net_amd.net import F8Net
from ir_cases import _b, _w
from oracle import oracle
from refgraph import RefGraph

ALL = dict(dwk_cases.CASES, max_batch=dwk_cases.MAX_BATCH_CASE, pipelined=dwk_cases.PIPELINED_CASE)
F8_ERR_UNSUPPORTED = -2
FUSE_ALL = dict(fuse_ir=2, fuse_irchain=1, fuse_dws=1, fuse_dws7=1, fuse_head2=1, fuse_head_dws=1)


@functools.lru_cache(maxsize=None)
def _planned(name):
    case = ALL[name]
    return dwk_cases.plan(name, case, dwk_cases.make_input(name, case))


def _dw_net(K, stride, pad, groups=16, C=16, hw=16):
    net = F8Net()
    t = net.input(C, hw, hw, 8)
    t = net.conv(t, np.ones((C, C // groups, K, K), np.int32), None, stride=stride, pad=pad, groups=groups, weight_fl=4, input_fl=8, input_signed=False,
                 quant_input=False, relu=True)
    net.output(t, as_float=False)
    return net


@pytest.mark.parametrize('K', [3, 5, 7])
def test_the_accepted_set_builds_and_finalizes(K):
    for stride in (1, 2):
        for pad in range(K // 2 + 1):
            net = _dw_net(K, stride, pad).finalize(2)
            tok = [net.launch_info(i, 1)[0] for i in range(net.num_launches) if net.launch_info(i, 1)[0].startswith('dwconv')]
            assert len(tok) == 1 and tok[0].startswith(f'dwconv{K}x{K}s{stride}:'), net.describe()


@pytest.mark.parametrize('K, stride, pad', [(9, 1, 4), (4, 1, 1), (5, 3, 2), (5, 1, 3), (7, 2, 4), (3, 1, 2)])
def test_everything_else_depthwise_is_unsupported(K, stride, pad):
    with pytest.raises(_lib.F8Error) as e:
        _dw_net(K, stride, pad)
    assert e.value.status == F8_ERR_UNSUPPORTED
    assert 'kernel 3, 5 or 7' in str(e.value) and 'stride 1 or 2' in str(e.value) and 'pad 0 .. kernel / 2' in str(e.value)


def test_groups_between_1_and_cin_are_still_refused():
    with pytest.raises(_lib.F8Error) as e:
        _dw_net(3, 1, 1, groups=2)
    assert e.value.status == F8_ERR_UNSUPPORTED and 'groups' in str(e.value)


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    x = dwk_cases.make_input(name, case)
    for leg in dwk_cases.LEGS:
        g, _, ids = _planned(name) if leg == 'own' else dwk_cases.plan(name, case, x, leg)
        lines = dwk_cases.dw_lines(g.net)
        assert [ln[1:] for ln in lines] == dwk_cases.expect(case, leg), (leg, g.net.describe())
        assert len(lines) == len(ids)                                # one launch per depthwise conv, an int32 form next to int8 ones included
        hw = (case['H'], case['W'])
        for (i, _, _), (K, s, _), pad in zip(lines, dwk_cases._convs(case), (case['pad'], None)):
            P, Q = dwk_cases.out_hw(case, K, s, K // 2 if pad is None else pad, hw)
            assert g.net.launch_info(i, case['N'])[2] == 2.0 * K * K * case['C'] * P * Q * case['N'], (leg, i)
            hw = (P, Q)
        if case['join_i32']:                                         # the planner keeps the int32 form and the int8 form on the one launch
            assert 'out[i32=1 i8=1' in [ln for ln in g.net.describe().splitlines() if 'dwconv' in ln][0], g.net.describe()


def test_every_expected_kernel_is_an_exported_symbol_and_the_table_covers_the_instances():
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    names = {k for c in ALL.values() for leg in dwk_cases.LEGS for k in dwk_cases.leg_kernels(c, leg)}
    for k in sorted(names):
        assert f'void {k}(f8::DwArgs)' in syms, k
    for K in (3, 5, 7):
        for s in (1, 2):
            assert dwk_cases.dot4(K, s) in names, (K, s)
    for sgn in (False, True):
        assert dwk_cases.generic(sgn) in names, sgn


@pytest.mark.parametrize('dwk_dot4', [0, 1])
@pytest.mark.parametrize('name', ['s_12x29', 'u_14x14', 't_28x28', 'd_7x7', 'd_7x13_s2', 'f_gen_i32', 'f_gen_i32_and_i8', 'f_rq1_29'])
def test_3x3_pad_1_plans_as_before(name, dwk_dot4):
    """The 3x3 / pad 1 launches keep their token and their three kernels, whatever dwk_dot4 says: dw_cases' own hand-written table, on its legs."""
    case = dw_cases.CASES[name]
    x = dw_cases.make_input(name, case)
    for leg in dw_cases.LEGS:
        g, _, _ = dw_cases.build_graph(case, x)
        for k, v in dict(case['opts'], dwk_dot4=dwk_dot4, **dw_cases.LEGS[leg]).items():
            g.net.set_option(k, v)
        g.net.finalize(x.shape[0])
        assert [ln[1:] for ln in dw_cases.dw_lines(g.net)] == dw_cases.expect(case, leg), (leg, g.net.describe())


def _inverted_residual(K):
    """input -> pre 1x1 -> [1x1 expand + ReLU -> K x K / 1 depthwise + ReLU -> 1x1 project] + the block input -> output"""
    x = np.zeros((2, 32, 14, 14), np.int32)
    g = RefGraph(x, 4)
    t = next(iter(g.v))
    kw = dict(groups=1, pad=0, weight_fl=6, input_signed=False)
    pre = g.conv(t, _w(1, (32, 32, 1, 1), 8.0), _b(2, 32, 64.0), input_fl=4, relu=False, quant_input=False, **kw)
    e = g.conv(pre, _w(3, (192, 32, 1, 1), 8.0), _b(4, 192, 64.0), input_fl=6, relu=True, **kw)
    d = g.conv(e, _w(5, (192, 1, K, K), 8.0), _b(6, 192, 64.0), stride=1, pad=K // 2, groups=192, weight_fl=6, input_fl=6, input_signed=False, relu=True)
    p = g.conv(d, _w(7, (32, 192, 1, 1), 8.0), _b(8, 32, 64.0), input_fl=6, relu=False, **kw)
    g.net.output(g.add(p, pre), as_float=False)
    for k, v in FUSE_ALL.items():
        g.net.set_option(k, v)
    g.net.finalize(2)
    return g.net


def test_no_fusion_pass_takes_a_general_depthwise_conv():
    """Every matcher of the planner asks for kernel 3 and pad 1: with all of them on, an inverted residual around a 5x5 is conv, dwconv5x5s1, conv —
    the join in the last conv's epilogue — and the same block around a 3x3 is the fused launch it was."""
    def block(net):
        names = [net.launch_info(i, 1)[0] for i in range(net.num_launches)]
        assert names[0].startswith('input') and names[1].startswith('conv1x1') and names[-1].startswith('output'), net.describe()
        return [n.split(':')[0] for n in names[2:-1]], net.describe()                 # (behind the input and the `pre` conv)
    names5, text5 = block(_inverted_residual(5))
    assert len(names5) == 3 and names5[0].startswith('conv1x1') and names5[1] == 'dwconv5x5s1' and names5[2].startswith('conv1x1') and \
        names5[2].endswith('_res'), text5
    names3, text3 = block(_inverted_residual(3))
    assert len(names3) == 1 and names3[0].startswith('fused_ir'), text3


def _pad_as_half(case, x, w, b):
    """What a kernel that addressed its windows with pad K // 2 whatever the argument would give: the first P x Q results of that conv."""
    P, Q = dwk_cases.out_hw(case)
    return oracle.conv2d(x, w, b, case['stride'], case['K'] // 2, case['C'])[:, :, :P, :Q]


@pytest.mark.parametrize('name', sorted(ALL))
def test_liveness_on_the_oracle(name):
    """A dead signal hides a failure — conditions on the case table, not measurements: the final value has more than 8 distinct values; every int8
    tensor a reader (or the second depthwise conv and the 1x1 in front of it) reads has at least 16 distinct values and fewer than half of its entries
    at a clamp bound; a pad below K // 2 changes the border ring of the depthwise result; a case that aims at a wrap shows it."""
    case = ALL[name]
    g, out, ids = _planned(name)
    assert np.unique(g.v[out][0]).size > 8
    assert len(g.taps) == len(case['readers'] or []) + (2 if case.get('second') else 0)
    for label, xq, sgn in g.taps:
        lo, hi = (-127, 127) if sgn else (0, 255)
        assert np.unique(xq).size >= 16, label
        assert ((xq == lo) | (xq == hi)).mean() < 0.5, label
    if case['pad'] != case['K'] // 2:
        x = dwk_cases.make_input(name, case)
        bd = _b(40, case['C'], case['b_sig'], case['b_mean'])
        other = _pad_as_half(case, x, dwk_cases._dw_weight(30, case['C'], case['K'], case['w_sig']), bd)
        raw = g.raw[ids[0]]
        ring = np.ones(raw.shape[2:], bool)
        ring[1:-1, 1:-1] = False
        assert raw.shape == other.shape and (raw[:, :, ring] != other[:, :, ring]).mean() > 0.5
    if case['aim'] == 'bias_big':
        (fl, _), = case['readers']
        n = case['in_fl'] + case['w_fl'] - fl
        r = g.raw[ids[0]].astype(np.int64)
        assert (r > 2 ** 31 - 2 ** 13).any(), 'no accumulator next to 2^31'
        # the accumulator itself wrapped past 2^31, or the rounding add `v + 2^(n-1)` of the requantisation does: the reference then clamps to 0
        wraps = (r < -2 ** 30) | (r + (1 << (n - 1)) > 2 ** 31 - 1)
        assert wraps[:, 3].any() and wraps[:, 17].any(), 'nothing wraps'
        assert (g.taps[0][1][wraps] == 0).all()
    else:
        assert case['aim'] is None


def test_the_relu_floor_matters_where_a_signed_reader_follows_it():
    """Behind a ReLU an unsigned reader's clamp at 0 does what the floor does; a signed reader's does not.  Those cases have accumulators below 0
    that a signed reader would keep, so a missing floor shows."""
    seen = 0
    for name, case in ALL.items():
        if not (case['relu'] and any(sgn for _, sgn in case['readers'] or [])):
            continue
        g, _, ids = _planned(name)
        fl = min(fl for fl, sgn in case['readers'] if sgn)
        assert (g.raw[ids[0]] < -(1 << (case['in_fl'] + case['w_fl'] - fl))).mean() > 0.01, name
        seen += 1
    assert seen >= 4
