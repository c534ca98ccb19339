"""The pool, join and classifier launches on the CPU: every case of tests/glue_cases.py plans to exactly its hand-written tokens and kernel symbols at
max_batch N and N + 1 and with every fusing pass on; the data conditions of its five tables hold on the reference alone (`check_data`, asserted by
`reference`); every int8 max-pool of the table is maxpool_i8x16_kernel (maxpool_kernel has no int8 branch); oracle.maxpool pinned to torch's
F.max_pool2d in float64 on the table's geometries — the -inf padding held against something other than the C oracle —, also behind the requantisation
to both int8 forms; three cases through ONNX and back.  tests/test_gpu_glue.py runs every case on the device."""
import numpy as np
import pytest

import glue_cases as gc
from f8net_amd import onnx_export, onnx_import, synth
from graph_cases import same_ops
from oracle import oracle
from refgraph import graph_forward


@pytest.mark.parametrize('name', sorted(gc.CASES))
def test_tokens_and_symbols_of_every_case(name):
    c = gc.CASES[name]
    x = gc.make_input(name)
    for max_batch in (c['N'], c['N'] + 1):
        for opts in ({}, gc.FUSE_ALL):
            g, _, _ = gc.plan(name, x, max_batch=max_batch, **opts)
            assert gc.lines(g.net) == gc.expected(name, **opts), g.net.describe()


@pytest.mark.parametrize('name', sorted(gc.CASES))
def test_data_conditions_hold_on_the_reference(name):
    """`reference` asserts glue_cases.check_data: negative maxima in border windows, distinct 16-byte groups, both clamps, the wrapped sums, the
    clamped and the kept extremes, the wrapped and the unrepresentable logits — and no output of one repeated value."""
    g, outs, ops = gc.reference(name)
    assert g.v[outs[0]][0].shape[0] == gc.CASES[name]['N'] + 1


def test_the_tables_hold_what_they_promise():
    A = [gc.CASES[n] for n in gc.TABLES['A']]
    assert {(c['k'], c['s'], c['pad']) for c in A} >= {(1, 1, 0), (2, 2, 0), (2, 1, 1), (3, 2, 1), (3, 1, 1), (3, 3, 0), (4, 2, 2), (5, 1, 2), (5, 3, 1)}
    assert {(c['H'], c['W']) for c in A} >= {(17, 18), (7, 5)} and {c['C'] for c in A} == {8, 40, 96}
    assert any(gc.out_size(c['H'], c['k'], c['s'], c['pad']) == 1 and gc.out_size(c['W'], c['k'], c['s'], c['pad']) == 1 for c in A)
    assert any((c['H'] + 2 * c['pad'] - c['k']) % c['s'] and (c['W'] + 2 * c['pad'] - c['k']) % c['s'] for c in A)
    assert all(not c['relu'] for c in A if c['pad'] > 0) and any(c['relu'] and c['form'] == 's8' for c in A)
    for tag in gc.GEOMETRY:                                        # every row on the int32 form and on both int8 forms
        assert [gc.CASES[f'a_{tag}_{f}']['exp'][0][0] for f in ('i32', 's8', 'u8')] == ['maxpool_i32:', 'maxpool_i8:', 'maxpool_i8:']
    C = [gc.CASES[n] for n in gc.TABLES['C']]
    assert {c['H'] * c['W'] for c in C} == {1, 3, 8, 9, 49, 64, 200}
    assert {(c['C'], c['N']) for c in C} >= {(C_, N) for C_ in (8, 40, 96) for N in (1, 3)} and {c['form'] for c in C} == {'i32', 'i8', 'two'}
    D = [gc.CASES[n] for n in gc.TABLES['D'] if 'd' in gc.CASES[n]]
    assert {c['d'] for c in D} == {0, 1, -1, 5, -5, 12} and {c['relu'] for c in D} == {True, False} and {c['C'] for c in D} == {8, 96}
    assert {c['form'] for c in D} == {'i32', 'i32_i8', 'two', 'three'} and {c['N'] * c['H'] * c['W'] for c in D} == {1, 33, 189}
    E = [gc.CASES[n] for n in gc.TABLES['E']]
    assert {c['features'] for c in E} == {256, 512, 500, 1024, 1280, 1250, 2048} and {c['classes'] for c in E} == {1, 10, 32, 33, 1000}
    assert sum(c['classes'] == 1000 for c in E) == 1 and {c['N'] for c in E} == {1, 3, 33} and {c['signed'] for c in E} == {True, False}
    assert all(c['N'] <= 3 and c['H'] * c['W'] <= 18 * 18 and c.get('C', 0) <= 96 for c in gc.CASES.values() if c['N'] != 33)


def test_every_int8_maxpool_is_the_16_byte_kernel():
    """maxpool_kernel reads int32 only: a pool on bytes — one int8 reader, any geometry f8_net_maxpool accepts, any channel count — is
    maxpool_i8x16_kernel, and a pool on int32 never is."""
    seen = set()
    for name, c in gc.CASES.items():
        for tok, sym in c['exp']:
            if tok.startswith('maxpool'):
                assert sym == {'maxpool_i8:': gc.MAXPOOL_I8, 'maxpool_i32:': gc.MAXPOOL_I32}[tok], name
                seen.add(tok)
    assert seen == {'maxpool_i8:', 'maxpool_i32:'}
    assert sum(c['exp'][0][0] == 'maxpool_i8:' for c in gc.CASES.values()) == 2 * len(gc.GEOMETRY)


# ---- the max-pool reference against torch
POOL_GEOMETRIES = sorted({(c['k'], c['s'], c['pad'], c['H'], c['W']) for c in gc.CASES.values() if c['table'] in 'AB'})


def pin_to_torch(x, k, s, pad):
    """oracle.maxpool == F.max_pool2d in float64 (-inf padding; |x| < 2^53: exact), on the int32 values and behind the requantisation to a signed
    and an unsigned int8 form (requant is monotone: it commutes with the maximum)."""
    import torch
    import torch.nn.functional as F
    assert np.abs(x).max() < 2 ** 53
    want = F.max_pool2d(torch.from_numpy(x.astype(np.float64)), k, s, pad).numpy()
    got = oracle.maxpool(x, k, s, pad)
    np.testing.assert_array_equal(got.astype(np.float64), want)
    for fl, sgn in ((5, True), (5, False)):
        q = oracle.requant(x, fl, 13, sgn)
        want8 = F.max_pool2d(torch.from_numpy(q.astype(np.float64)), k, s, pad).numpy()
        np.testing.assert_array_equal(oracle.maxpool(q, k, s, pad).astype(np.float64), want8)
        np.testing.assert_array_equal(oracle.requant(got, fl, 13, sgn).astype(np.float64), want8)


@pytest.mark.parametrize('k, s, pad, H, W', POOL_GEOMETRIES)
def test_maxpool_reference_is_torch_float64(k, s, pad, H, W):
    x = synth.rand_uniform_int(9, f'gluepin{k}{s}{pad}{H}{W}', (2, 5, H, W), -2 ** 16, 2 ** 13).astype(np.int32)      # mostly negative: border maxima below 0
    pin_to_torch(x, k, s, pad)
    full = synth.rand_uniform_int(10, f'gluepinfull{k}{s}{pad}{H}{W}', (1, 3, H, W), -2 ** 31, 2 ** 31 - 1).astype(np.int64)
    full.reshape(-1)[:2] = [-2 ** 31, 2 ** 31 - 1]
    import torch
    import torch.nn.functional as F
    np.testing.assert_array_equal(oracle.maxpool(full.astype(np.int32), k, s, pad).astype(np.float64),
                                  F.max_pool2d(torch.from_numpy(full.astype(np.float64)), k, s, pad).numpy())


# ---- ONNX
@pytest.mark.parametrize('name', ['a_3s2p1_s8', 'c_hw49', 'e_2048_1000_pooled'])
def test_onnx_round_trip(name):
    """A pool, a global pool and a classifier: exported, imported, the same ops field for field, the walker's values the reference graph's, and the
    imported graph plans to the case's tokens and symbols."""
    ig, g, out = gc.int_graph(name)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    same_ops(ig, back)
    assert back.solve_fraclens(gc.X_FL) == ig.solve_fraclens(gc.X_FL)
    x = gc.make_input(name)
    np.testing.assert_array_equal(graph_forward(back, x, gc.X_FL), g.v[out][0])
    net = back.build_net(3, input_fraclen=gc.X_FL)
    assert [l for l in gc.lines(net) if not l[0].startswith('conv')] == gc.expected(name), net.describe()


def test_onnx_round_trip_of_a_join():
    """(its operands are outputs of the case; an IntGraph has one output: the join graph is drawn here, on two convs that a second join also reads)"""
    from refgraph import record_int_graph
    c = gc.CASES['d_p5_two']
    x = gc.make_input('d_p5_two')

    def build(g, x0):
        a = gc._operand(g, x0, 0, c['C'], 15, 18, {})
        b = gc._operand(g, x0, 1, c['C'], 10, 13, {})
        return g.add(g.add(a, b, relu=False), g.add(a, b, relu=True))
    ig, g, out = record_int_graph(x, gc.X_FL, build)
    back = onnx_import.import_graph(onnx_export.export_graph(ig))
    same_ops(ig, back)
    np.testing.assert_array_equal(graph_forward(back, x, gc.X_FL), g.v[out][0])
    net = back.build_net(3, input_fraclen=gc.X_FL)
    assert gc.lines(net) == [('add:', gc.ADD)] * 3, net.describe()
