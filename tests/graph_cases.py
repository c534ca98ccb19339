"""What the op-case modules and their two test files share: the launches of a plan by token, the functions every case module binds to its own case
table (`build_graph`, `reference`, `plan`, `int_graph`), the runner of one case on the device, and the helpers of the _plan files (IntGraph equality,
the shipped nets' digests, the host code under the sanitizers).  The reference graph and the IntGraph walker are tests/refgraph.py, the per-op
references tests/ref_ops.py.  No test functions here."""
import functools
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

import dil_cases
from f8net_amd import synth, topology
from f8net_amd.net import record_net
from oracle import oracle
from refgraph import RefGraph, record_int_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_lines(net, prefix='', label=None):
    """[(launch index, plan token 'xyz:', kernel symbol)] of the handle's launches whose token starts with `prefix` (a string or a tuple of them)
    and, if given, whose tensor is labelled `label`, in launch order."""
    out = []
    for i in range(net.num_launches):
        tok, _, what = net.launch_info(i, 1)[0].partition(':')
        if tok.startswith(prefix) and label in (None, what):
            out.append((i, tok + ':', net.launch_kernel(i)))
    return out


# ---- the functions of a case module.  A case is a dict with 'build': build(graph, input id, case, **extra) -> (output ids, op ids), 'N', and
# optionally 'x_fl' (else the module's X_FL) and 'opts' (planning options of its own)
def bind_cases(mod, spare_image=True, check_data=None):
    """Gives the case module `mod` (its CASES, X_FL and make_input(name, n)) the functions every such module has:
        build_graph(name, x, record=True, **extra)  -> (graph, output ids, op ids); extra: keywords of the module's builders
        reference(name)                             the same on the reference alone over N + 1 images (spare_image=False: N), once; read-only;
                                                    check_data(name, graph, output ids, op ids) asserts what the module's table promises about the data
        plan(name, x, max_batch=None, **opts)       build_graph finalized for max_batch (else x's) images under the case's and these options
        int_graph(name)                             -> (IntGraph, graph, output id): the case as an IntGraph, op for op what build_graph records
                                                    (cases whose first output is the only one)"""
    def x_fl(c):
        return c.get('x_fl', mod.X_FL)

    def build_graph(name, x, record=True, **extra):
        c = mod.CASES[name]
        g = RefGraph(x, x_fl(c), record=record)
        outs, ops = c['build'](g, next(iter(g.v)), c, **extra)
        return g, outs, ops

    @functools.lru_cache(maxsize=None)
    def reference(name):
        g, outs, ops = build_graph(name, mod.make_input(name, mod.CASES[name]['N'] + (1 if spare_image else 0)), record=False)
        if check_data:
            check_data(name, g, outs, ops)
        return g, outs, ops

    def plan(name, x, max_batch=None, **opts):
        g, outs, ops = build_graph(name, x)
        for k, v in dict(mod.CASES[name].get('opts', {}), **opts).items():
            g.net.set_option(k, v)
        g.net.finalize(max_batch or x.shape[0])
        return g, outs, ops

    def int_graph(name):
        c = mod.CASES[name]
        return record_int_graph(mod.make_input(name), x_fl(c), lambda g, x0: c['build'](g, x0, c)[0][0])

    mod.build_graph, mod.reference, mod.plan, mod.int_graph = build_graph, reference, plan, int_graph


# ---- one case on the device
def run_case(mod, name, dev, check_plan, *, spare_image=True, float_last_only=False, **opts):
    """The case planned under `opts` for N + 1 images (spare_image=False: N) and run at N and N - 1 from that one handle, every output bit for bit
    against mod.reference(name).  check_plan(net, name, opts) is the caller's assertion about the plan's tokens.  A case with 'as_float' compares
    its outputs (float_last_only: its last output) as float32."""
    c = mod.CASES[name]
    N = c['N']
    M = N + 1 if spare_image else N
    ref, routs, _ = mod.reference(name)
    wants = [ref.v[o][0] for o in routs]
    x = mod.make_input(name, M)
    g, _, _ = mod.plan(name, x, max_batch=M, **opts)
    check_plan(g.net, name, opts)
    xt = torch.from_numpy(x).to(dev)
    for n in (N, N - 1):
        if n < 1:
            continue
        got = g.net.run(xt[:n])
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == len(wants)
        for k, (y, w) in enumerate(zip(got, wants)):
            if c.get('as_float') and (k == len(wants) - 1 or not float_last_only):
                w = w.astype(np.float32)
            np.testing.assert_array_equal(y.cpu().numpy().reshape((n,) + w.shape[1:]), w[:n], err_msg=f'{name} {opts} n={n} output {k}')
    g.net.check()


def se_branch_on_resnet50_stage(dev, build_branch, token, *, lines):
    """ResNet-50 at 64 x 64: stage_1_layer_1's output (512 x 8 x 8 at fraclen 10, values up to 2^20) sits in the middle of what the stage chain runs as
    one launch.  build_branch(g, src) -> scaled map id draws an SE branch on it (and asserts what it wants of its own gate); the scaled map is output 1,
    so the launch is cut there.  `lines` is the calling module's own `lines(net)`: what it lists holds the one launch `token` (plan token, kernel
    symbol) and nothing else; the logits stay the plain net's; on the default plan and with every fusing pass on."""
    name = 'stage_1_layer_1'
    spec = topology.get('resnet50')
    params = synth.make_params(spec, seed=17)
    x, x_fl = synth.make_input(spec, params, 2, 64, seed=3)
    seen = {}
    tspec, tparams = dil_cases.stuffed_twin(spec, params)
    logits = oracle.net_forward(tspec, tparams, x, x_fl, tap=lambda k, v, fl: seen.__setitem__(k, (v.copy(), fl)) if k == name else None)
    assert seen[name][0].shape[1:] == (512, 8, 8) and seen[name][1] == 10
    xt = torch.from_numpy(x).to(dev)
    for options in (None, dil_cases.FUSE_ALL):
        net = record_net(spec, params, 64, options=options)
        src = net.tap_ids[name]
        g = RefGraph.on(net, {src: seen[name]})
        s = build_branch(g, src)
        assert net.output(s, as_float=False) == 1
        for k, val in (options or {}).items():
            net.set_option(k, val)
        net.finalize(2)
        assert [(t, k) for _, t, k in lines(net)] == [token], net.describe()
        want = g.v[s][0]
        assert np.unique(want).size > 100
        got, scaled = net.run(xt)
        net.check()
        np.testing.assert_array_equal(got.cpu().numpy(), logits, err_msg=f'logits {options}')
        np.testing.assert_array_equal(scaled.cpu().numpy().reshape(want.shape), want, err_msg=f'scaled map {options}')


# ---- the _plan files
OP_FIELDS = ('kind', 'src', 'src2', 'stride', 'pad', 'groups', 'kernel', 'shift', 'signed', 'signed2', 'relu', 'dilation', 'srcs', 'shifts', 'shape', 'mode',
             'scale', 'output_padding', 'key', 'first', 'channels', 'in_fl', 'out_fl')


def same_ops(a, b):
    """Two IntGraphs hold the same ops, field for field (a field an op does not have compares default == default)."""
    assert len(a.ops) == len(b.ops) and a.output == b.output and a.output_float == b.output_float
    for p, q in zip(a.ops, b.ops):
        for f in OP_FIELDS:
            assert getattr(p, f) == getattr(q, f), (p.kind, f, getattr(p, f), getattr(q, f))
        for f in ('weight', 'bias', 'table'):
            assert (getattr(p, f) is None) == (getattr(q, f) is None)
            if getattr(p, f) is not None:
                np.testing.assert_array_equal(getattr(p, f), getattr(q, f))


def plan_digest_tool():
    """tools/plan_digest.py as a module."""
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import plan_digest
    return plan_digest


def shipped_digest_membership(jobs):
    """Every job's line, planned now under tools/plan_digest.py's DEFAULT option column, is one of the recorded lines
    (tests/golden/plan_digest_default.txt).  Membership, not file equality: tests/test_plan_digest.py compares the whole file and the whole matrix."""
    plan_digest = plan_digest_tool()
    want = open(os.path.join(ROOT, 'tests', 'golden', 'plan_digest_default.txt')).read().splitlines()
    assert len(want) == (len(plan_digest.ARCHS) + len(plan_digest.EXTRA_SIZES)) * len(plan_digest.BATCHES)
    for job in jobs:
        (line,) = plan_digest.plan_lines(job)
        assert line in want, line


def all_shipped_jobs():
    """Every net at 224 x 224 for 2 and 128 images, the extra sizes for 128."""
    plan_digest = plan_digest_tool()
    return ([(a, 224, bs, False, 'default') for a in plan_digest.ARCHS for bs in (2, 128)] +
            [(a, hw, 128, False, 'default') for a, hw in plan_digest.EXTRA_SIZES])


SANITIZERS = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
_sanitized = {}                                                    # one compile of f8_net.cpp per test session


def _sanitized_net_object(hipcc):
    if 'net_o' not in _sanitized:
        _sanitized['dir'] = tempfile.TemporaryDirectory(prefix='f8_net_san_')      # removed when the session ends
        net_o = os.path.join(_sanitized['dir'].name, 'f8_net_san.o')
        subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O1', '-g', '-std=c++17', '-fPIC'] + [a for s in SANITIZERS for a in ('-Xarch_host', s)] +
                              ['-x', 'hip', '-c', os.path.join(ROOT, 'f8net_amd', 'csrc', 'f8_net.cpp'), '-o', net_o])
        _sanitized['net_o'] = net_o
    return _sanitized['net_o']


def sanitized_host_program(example_c, libs=()):
    """examples/<example_c> as a stand-alone program (its own main) on f8_net.cpp's host side compiled with AddressSanitizer and
    UndefinedBehaviorSanitizer, linked with the library's other objects (and `libs`, such as '-lm'); runs it, asserts a clean exit and a clean
    stderr, returns its stdout."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    objs = [o for o in sorted(glob.glob(os.path.join(ROOT, 'build', 'f8_*.o'))) if os.path.basename(o) != 'f8_net.o']
    assert os.path.exists(hipcc) and len(objs) >= 32, 'build libf8net.so first (__graft_entry__.build()): its objects are linked here'
    net_o = _sanitized_net_object(hipcc)
    stem = os.path.join(os.path.dirname(net_o), os.path.splitext(example_c)[0])
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include')] + SANITIZERS +
                          ['-c', os.path.join(ROOT, 'examples', example_c), '-o', stem + '.o'])
    subprocess.check_call([hipcc, '--offload-arch=gfx950'] + SANITIZERS + [stem + '.o', net_o] + objs + list(libs) + ['-o', stem])
    env = dict(os.environ, LD_LIBRARY_PATH='/opt/rocm/lib:' + os.environ.get('LD_LIBRARY_PATH', ''), ASAN_OPTIONS='detect_leaks=1')
    r = subprocess.run([stem], text=True, capture_output=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr
    return r.stdout
