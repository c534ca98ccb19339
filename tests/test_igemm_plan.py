"""The implicit-GEMM conv kernel (conv_igemm_kernel of f8_kernels.hip) at op level, without a GPU: the plan of every case of tests/igemm_cases.py
against the hand-written table, the kernel instances as exported symbols, table A against the list of instances launch_conv can dispatch, the
boundaries of pick_conv_tile's default selection, the option igemm_tile, and the liveness of every case on the oracle's values."""
import functools
import os
import subprocess

import numpy as np
import pytest

import igemm_cases as ic
from f8net_amd import _lib, synth, topology
from f8net_amd.net import F8Net, build_net

ALL = ic.CASES
F8_ERR_INVALID, F8_ERR_STATE = -1, -5


@functools.lru_cache(maxsize=None)
def _planned(name):
    case = ALL[name]
    return ic.plan(name, case, ic.make_input(name, case))


def _tile(kernel):
    """(bm, bn, bk, pad, res, ring, dual) of a kernel name."""
    f = kernel[kernel.index('<') + 1:-1].split(', ')
    return int(f[0]), int(f[1]), int(f[2]), f[5] == 'true', f[6] == 'true', int(f[7]), f[8] == 'true'


@pytest.mark.parametrize('name', sorted(ALL))
def test_plan(name):
    case = ALL[name]
    g, _, _, _ = _planned(name)
    assert ic.under_test(g.net) == [(case['token'], case['kernel'])], g.net.describe()
    ls = ic.lines(g.net)
    for e in case['extra_tokens']:
        assert e in ls, g.net.describe()
    # the K loop the table says the case has: taps x padded channels / bk (the dual pair: both products)
    bm, bn, bk, pad, res, ring, dual = _tile(case['kernel'])
    ck = ((case['dual']['mid'] if dual else case['cin']) + 31) // 32 * 32
    nk = case['k'] ** 2 * ck // bk + ((case['c0'] + 31) // 32 * 32 // bk if dual else 0)
    assert nk == case['nk'] and pad == (case['pad'] > 0) and res == bool(case['join'] or dual), (nk, case['nk'])
    assert ring == (ic.deep_stages(bm, bn, bk) if nk >= g.net.get_option('deep_nk') else 2)


def test_every_expected_kernel_is_an_exported_symbol():
    so = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'libf8net.so')
    syms = subprocess.run(['nm', '-DC', so], capture_output=True, text=True, check=True).stdout
    for k in sorted({c['kernel'] for c in ALL.values()} | ic.all_instances()):
        assert f'void {k}(f8::ConvArgs)' in syms, k
    for k, args in ((ic.ADD_KERNEL, 'AddArgs'), (ic.MAXPOOL_I32, 'PoolArgs'), (ic.MAXPOOL_I8, 'PoolArgs'), (ic.AVGPOOL, 'AvgArgs')):
        assert f'{k}(f8::{args})' in syms, k
    # ... and the library exports no instance of the kernel the list does not have
    exported = {ln.split('void ')[1].split('(f8::ConvArgs)')[0] for ln in syms.splitlines() if 'void f8::conv_igemm_kernel<' in ln}
    assert exported == ic.all_instances()


def test_table_a_is_exactly_the_dispatchable_instances():
    """106 = 14 tiles x HAS_PAD x HAS_RES x {ring 2, ring 4 where 4 slots fit 64 KB} + the dual pair on three tiles at both depths; 86 of them by the
    default selection, the twenty joins on 128-wide tiles by igemm_tile."""
    want = ic.all_instances()
    assert len(want) == 106
    got = {c['kernel'] for c in ic.TABLE_A.values()}
    assert got == want
    forced = {c['kernel'] for c in ic.TABLE_A.values() if 'igemm_tile' in c['opts']}
    default = {c['kernel'] for c in ic.TABLE_A.values() if 'igemm_tile' not in c['opts']}
    assert len(forced) == 20 and len(default) == 86 and not (forced & default)
    for k in forced:
        bm, bn, bk, pad, res, ring, dual = _tile(k)
        assert bn == 128 and res and not dual
    for c in ic.TABLE_A.values():
        assert c['N'] == 3 and c['max_batch'] in (3, 512, 1024) and (c['H'], c['W']) == (8, 8)


def test_table_a_k_loops_per_ring_depth():
    """Each ring depth sees K loops of 1, 2, 3 and 9 steps, on tiles whose waves own equal numbers of DMA slots (the counted waits of wait_ahead's
    first branch) and on ragged ones (its second): a loop shorter than the prologue, one as long as the ring, and the slot wrap-around."""
    seen = {}
    for c in ic.TABLE_A.values():
        bm, bn, bk, pad, res, ring, dual = _tile(c['kernel'])
        seen.setdefault((ring, ic.uniform_ld(bm, bn, bk)), set()).add(c['nk'])
    assert set(seen) == {(2, True), (2, False), (4, True), (4, False)}
    for key, nks in seen.items():
        assert {1, 2, 3} <= nks and max(nks) >= 9, (key, nks)
    assert not ic.uniform_ld(64, 64, 32) and not ic.uniform_ld(128, 32, 64) and ic.uniform_ld(64, 64, 64) and ic.uniform_ld(128, 128, 32)


def _one_conv(cout, max_batch, join, **opts):
    """A 1x1 conv 32 -> cout on a 16 x 8 map (128 pixels: one 128-row tile per image), with a join or without: its plan token."""
    net = F8Net()
    for k, v in dict(ic.BASE_OPTS, fuse_dual=0, **opts).items():
        net.set_option(k, v)
    t0 = net.input(32, 16, 8, 8)
    kw = dict(stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False, quant_input=False)
    y = net.conv(t0, np.ones((cout, 32, 1, 1), np.int32), None, relu=True, **kw)
    if join:
        y = net.add(y, net.conv(t0, np.ones((cout, 32, 1, 1), np.int32), None, relu=False, **kw))
    net.output(y, as_float=False)
    net.finalize(max_batch)
    toks = [ln[0] for ln in ic.lines(net) if ln[0].startswith('conv1x1s1_t') and (ln[0].endswith('_res:') == join)]
    return toks[-1]


# (cout, join) -> [(max_batch, tile)]: one max_batch either side of every boundary of pick_conv_tile.  128 pixels per image: a 128-row tile per image
BOUNDARIES = {
    (32, False): [(1, '128x32'), (511, '128x32'), (512, '128x32')],
    (32, True): [(1, '128x32'), (512, '128x32')],
    (64, False): [(511, '64x64'), (512, '128x64')],                              # 512 tiles of 128x64
    (64, True): [(511, '64x64'), (512, '128x64')],
    (96, False): [(255, '64x64'), (256, '64x128'), (511, '64x128'), (512, '128x128')],   # bn 128: 512 tiles of 64x128 at 256 images
    (128, False): [(255, '64x64'), (256, '64x128'), (511, '64x128'), (512, '128x128')],
    (96, True): [(255, '64x64'), (256, '128x64')],                                # a join: bn 64, two tiles per image row
    (128, True): [(255, '64x64'), (256, '128x64'), (1024, '128x64')],
}


@pytest.mark.parametrize('cout,join', sorted(BOUNDARIES))
def test_default_selection_boundaries(cout, join):
    for max_batch, tile in BOUNDARIES[(cout, join)]:
        assert _one_conv(cout, max_batch, join) == f'conv1x1s1_t{tile}x32{"_res" if join else ""}:', (cout, join, max_batch)


def test_igemm_tile_follows_autotunes_admissibility():
    want = {1: '128x128', 2: '128x64', 3: '64x128', 4: '64x64'}
    for v, tile in want.items():
        for join in (False, True):
            assert _one_conv(128, 2, join, igemm_tile=v) == f'conv1x1s1_t{tile}x32{"_res" if join else ""}:'
            # no 128-wide tile over coutP <= 64; never 64x32 (coutP 32 keeps 128x32 under 1 and 3, and takes 128x64 / 64x64)
            narrow = tile if tile.endswith('x64') else '64x64'
            assert _one_conv(64, 2, join, igemm_tile=v) == f'conv1x1s1_t{narrow}x32{"_res" if join else ""}:'
            assert _one_conv(32, 2, join, igemm_tile=v) == f'conv1x1s1_t{tile if tile.endswith("x64") else "128x32"}x32{"_res" if join else ""}:'
    # the dual pair (coutP 64): 128x64 and 64x64; the 128-wide tiles are refused and the default stays
    for v, tile in ((1, '64x64'), (2, '128x64'), (3, '64x64'), (4, '64x64')):
        case = dict(ic.TABLE_C['c_dual'], opts={'igemm_tile': v})
        g, _, _, _ = ic.plan('c_dual', case, ic.make_input('c_dual', case))
        assert ic.under_test(g.net)[0][0] == f'conv1x1s1_t{tile}x64_dual:', v
    # bk stays
    case = dict(ic.TABLE_A['a_64x64x128_nn2'], opts=dict(ic.TABLE_A['a_64x64x128_nn2']['opts'], igemm_tile=2))
    g, _, _, _ = ic.plan('x', case, ic.make_input('x', case))
    assert ic.under_test(g.net)[0][0] == 'conv1x1s1_t128x64x128:'


def test_igemm_tile_is_a_planning_key_and_zero_by_default(monkeypatch):
    assert F8Net().get_option('igemm_tile') == 0
    net = F8Net().set_option('igemm_tile', 4)
    t = net.input(32, 4, 4, 8)
    net.output(net.conv(t, np.ones((32, 32, 1, 1), np.int32), None, stride=1, pad=0, groups=1, weight_fl=5, input_fl=8, input_signed=False,
                        quant_input=False, relu=True), as_float=False)
    net.finalize(2)
    with pytest.raises(_lib.F8Error) as e:
        net.set_option('igemm_tile', 1)
    assert e.value.status == F8_ERR_STATE
    with pytest.raises(_lib.F8Error) as e:
        F8Net().set_option('igemm_tile', 5)
    assert e.value.status == F8_ERR_INVALID
    monkeypatch.setenv('F8_IGEMM_TILE', '3')
    assert F8Net().get_option('igemm_tile') == 3


@pytest.mark.parametrize('arch', ['resnet18', 'resnet50', 'mobilenet_v1', 'mobilenet_v2'])
def test_shipped_plans_do_not_move_with_the_key_at_zero(arch):
    spec = topology.get(arch, normalize=arch == 'resnet50')
    params = synth.make_params(spec, seed=3)
    for bs in (2, 128):
        a = build_net(spec, params, max_batch=bs, hw=224)
        b = build_net(spec, params, max_batch=bs, hw=224, options={'igemm_tile': 0})
        assert a.get_option('igemm_tile') == 0 and a.describe() == b.describe()
        assert [a.launch_kernel(i) for i in range(a.num_launches)] == [b.launch_kernel(i) for i in range(b.num_launches)]


# ---- liveness on the oracle's values

def _forms(name):
    """[(label, int32 value the launch requantises, int8 value, shift, signed)] of the int8 forms the launch under test writes."""
    case = ALL[name]
    g, _, _, t = _planned(name)
    if case['pool'] or not case['readers']:
        return []
    v, fl = g.v[t]
    out = []
    for (rfl, sgn), (label, xq, s2) in zip(case['readers'], [tp for tp in g.taps if tp[0].startswith('reader')]):
        assert sgn == s2
        out.append((label, v.astype(np.int64), xq, fl - rfl, sgn))
    assert len(out) == len(case['readers'])
    return out


def _joined_sum(name):
    """The aligned sum of a join before its clamp, as wrapping int32 arithmetic gives it; None without a join."""
    case = ALL[name]
    g, _, y, t = _planned(name)
    if not (case['join'] or case['dual']):
        return None
    ov, (acc_shl, res_shl) = g.v[g.other][0], g.shl
    s = ((g.v[y][0].astype(np.int64) << acc_shl) + (ov.astype(np.int64) << res_shl)) & 0xFFFFFFFF
    return np.where(s >= 2 ** 31, s - 2 ** 32, s)


@pytest.mark.parametrize('name', sorted(ALL))
def test_liveness_on_the_oracle(name):
    """A dead signal hides a failure.  Every int8 form the launch writes has at least 16 distinct values, reaches each end of its clamp and keeps at
    most a quarter of its values at each (behind a ReLU the lower end of a signed form is the floor's 0); a right shift meets an exact tie above an even and above an odd quotient (round-half-even goes both ways).
    A join's sum exceeds 2^30 somewhere and is exactly -2^31 somewhere (the value the clamp at -(2^31 - 1) changes); a ReLU has accumulators on both
    sides of its floor; an unsigned input under padding has two border classes along each axis that has two outputs."""
    case = ALL[name]
    g, outs, y, t = _planned(name)
    for o in outs:
        assert np.unique(g.v[o][0]).size > 8
    for label, v, xq, n, sgn in _forms(name):
        lo, hi = (-127, 127) if sgn else (0, 255)
        assert np.unique(xq).size >= 16, label
        floored = case['join_relu'] if (case['join'] or case['dual']) else case['relu']     # behind a ReLU a signed form's lower end is the floor's 0
        assert (xq == (0 if floored else lo)).any() and (xq == hi).any(), (label, int(xq.min()), int(xq.max()))
        assert (xq == lo).mean() <= 0.25 and (xq == hi).mean() <= 0.25, (label, (xq == lo).mean(), (xq == hi).mean())
        if n > 0:
            tie = (v & ((1 << n) - 1)) == (1 << (n - 1))
            q = v >> n
            inside = tie & (q >= lo) & (q < hi)
            assert (inside & (q % 2 == 0)).any() and (inside & (q % 2 == 1)).any(), (label, int(tie.sum()))
    s = _joined_sum(name)
    if s is not None:
        assert (np.abs(s) > 2 ** 30).any(), 'no joined value above 2^30'
        assert (s == -2 ** 31).any(), 'no joined value the clamp changes'
        assert (g.v[t][0] >= -(2 ** 31 - 1)).all()
    if case['relu']:
        raw = g.raw[y]
        assert (raw < 0).mean() > 0.01 and (raw > 0).mean() > 0.25, ((raw < 0).mean(), (raw > 0).mean())
    if case['join_relu']:
        assert (s < 0).mean() > 0.01 and (s > 0).mean() > 0.25
    if case['pad'] > 0 and not case['in_signed']:
        P, Q = ic.out_hw(case)
        for size, outn in ((case['H'], P), (case['W'], Q)):
            masks = {tuple(0 <= p * case['stride'] - case['pad'] + r < size for r in range(case['k'])) for p in range(outn)}
            assert len(masks) >= min(2, outn), (size, outn)
    if name == 'b_2x2_under_7x7':
        masks = {tuple(0 <= p * case['stride'] - case['pad'] + r < case['H'] for r in range(case['k'])) for p in range(ic.out_hw(case)[0])}
        assert any(not m[0] and not m[-1] and any(m) for m in masks)
    if case['bias_big']:
        raw = g.raw[y].astype(np.int64)
        assert (raw > 2 ** 31 - 2 ** 13).any() and (raw < -2 ** 31 + 2 ** 13).any()


def test_table_b_covers_the_grids_and_ragged_pixel_counts():
    """Workgroups = ceil(M / bm) * ceil(coutP / bn) of the run (N images): 1, 7, 9 and 17 are there (fewer than eight, and both sides of a multiple of
    eight, for the XCD remap); M one either side of a multiple of 32, of 64 and of 128."""
    grids, ms = set(), set()
    for name, c in ic.TABLE_B.items():
        bm, bn = _tile(c['kernel'])[:2]
        P, Q = ic.out_hw(c)
        M = c['N'] * P * Q
        grids.add(-(-M // bm) * -(-((c['cout'] + 31) // 32 * 32) // bn))
        ms.add((M, bm))
    assert {1, 7, 9, 17} <= grids, sorted(grids)
    assert {(63, 64), (65, 64), (31, 64), (33, 64), (127, 128), (129, 128)} <= ms
