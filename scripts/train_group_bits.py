#!/usr/bin/env python3
"""The bits the grouped training-mode forward writes, for comparing two builds of libgnnloop.so (the library GNNKERAS_AMD_LIB names;
default: the built one): every case of tests/test_gpu_train_group_forms.py - all twelve instantiations of k_train_group_fwd /
k_train_group_fwd_types - plus layer 0 of the two MUTAG starter stacks (homogeneous: d = 0, selu / softmax, BatchNormalization, threshold
0.01; composite: one node type, state 10) over the first `--graphs` MUTAG graphs as ONE grouped call each.  Per case k_groups, the state,
the node-level output and every network's moving mean / variance go to an .npz.

    python scripts/train_group_bits.py --out FILE.npz [--graphs 512]
    python scripts/train_group_bits.py --compare A.npz B.npz C.npz     A, B: two runs of one build; C: the other build

--compare names every array that differs between A and B (run-to-run differences of one build), then holds C to A: an array that is
bit-equal between A and B must be bit-equal in C; one that is not must differ from A by no more than B does.  Exit status 1 otherwise."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'tests'))

import numpy as np


def moving(gnn):
    nets = (list(gnn.net_state) if isinstance(gnn.net_state, (list, tuple)) else [gnn.net_state]) + [gnn.net_output]
    return {f'moving{i}_{part}': np.array(n_.get_weights()[2 + j], copy=True) for i, n_ in enumerate(nets) for j, part in enumerate(('mean', 'var'))
            if len(n_.get_weights()) >= 4}


def mutag_case(kind, count):
    """(model, merged batch, group table, per-graph state_0) of layer 0 of the starter stack of `kind`."""
    import lgnn_propagate_perf as hom
    from gnnkeras_amd.load_MUTAG import load_graphs, load_composite_graphs
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNgraphBased
    from gnnkeras_amd.Models.MLP import MLP
    from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer, CompositeMultiGraphSequencer
    rng = np.random.default_rng(0)
    if kind == 'homogeneous':
        graphs = load_graphs()[:count]
        gnn, seq_cls, d = hom.stack('grouped').gnns[0], MultiGraphSequencer, 0
    else:
        graphs = load_composite_graphs(limit=count)
        d, L0, A, T = 10, 14, 3, 2                                  # (scripts/composite_lgnn_propagate_perf.py, layer 0)
        ns = [MLP((L0 + 2 * d + L0 + A,), [d], 'selu', 'lecun_normal', 'lecun_normal', rng=0)]
        gnn, seq_cls = CompositeGNNgraphBased(ns, MLP((d,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=1), d, 5, 0.01), CompositeMultiGraphSequencer
    for g in graphs: g.setAggregation('average')
    graphs = [g for g in graphs if g.nodes.shape[0] <= 256]
    x = seq_cls(list(graphs), 'g', 'average', len(graphs), shuffle=False)[0][0]
    begin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in graphs])])
    s0s = [rng.normal(0, 0.1, (g.nodes.shape[0], d)).astype(np.float32) for g in graphs]
    return gnn, x, begin, s0s


def dump(path, count):
    import torch
    from gnnkeras_amd import _native as nat
    import test_gpu_train_group_forms as forms
    out = {}
    for kind, d, weighted in forms.CASES:
        gnn, x, begin, _ops, s0s, _graphs = forms.build_case(kind, d, weighted)
        k, state, y = forms.run_case(kind, gnn, x, begin, s0s)
        tag = f'{kind}_d{d}_{"weighted" if weighted else "uniform"}'
        out.update({f'{tag}/k_groups': k, f'{tag}/state': state, f'{tag}/y_pred': y}, **{f'{tag}/{n}': v for n, v in moving(gnn).items()})
        print(tag, nat.lib().gnn_last_kernel_name().decode(), k.tolist(), flush=True)
    for kind in ('homogeneous', 'composite'):
        gnn, x, begin, s0s = mutag_case(kind, count)
        if kind == 'homogeneous':                                   # (d = 0: the state is the label matrix)
            k, state, y = (v.cpu().numpy() for v in gnn.Loop(*gnn.process_inputs(x), training=True, groups=begin, node_level=True))
        else: k, state, y = forms.run_case(kind, gnn, x, begin, s0s)
        tag = f'mutag_{kind}'
        name = nat.lib().gnn_last_kernel_name().decode()
        assert name.startswith('train_step: grouped forward kernels'), name
        out.update({f'{tag}/k_groups': k, f'{tag}/state': state, f'{tag}/y_pred': y}, **{f'{tag}/{n}': v for n, v in moving(gnn).items()})
        print(tag, name, len(begin) - 1, 'groups, k histogram', dict(zip(*[v.tolist() for v in np.unique(k, return_counts=True)])), flush=True)
    torch.cuda.synchronize()
    np.savez(path, library=np.array(nat.lib()._name), **out)
    print(f'{len(out)} arrays from {nat.lib()._name} -> {path}')


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def compare(pa, pb, pc):
    A, B, C = (np.load(p) for p in (pa, pb, pc))
    names = [n for n in A.files if n != 'library']
    assert sorted(names) == sorted(n for n in B.files if n != 'library') == sorted(n for n in C.files if n != 'library')
    print('A', A['library'], '\nB', B['library'], '\nC', C['library'])
    bad = 0
    for n in names:
        if same(A[n], B[n]):
            if not same(A[n], C[n]):
                bad += 1
                print(f'DIFFERS  {n}: bit-equal between A and B, max |C - A| = {np.max(np.abs(C[n].astype(np.float64) - A[n].astype(np.float64)))}')
        else:
            own = float(np.max(np.abs(B[n].astype(np.float64) - A[n].astype(np.float64))))
            other = float(np.max(np.abs(C[n].astype(np.float64) - A[n].astype(np.float64))))
            print(f'run-to-run  {n}: max |B - A| = {own}, max |C - A| = {other}')
            if other > own: bad += 1
    print(f'{len(names)} arrays, {bad} outside what A and B allow')
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--graphs', type=int, default=512)
    ap.add_argument('--compare', nargs=3)
    args = ap.parse_args()
    if args.compare: return compare(*args.compare)
    if not args.out: ap.error('--out or --compare')
    sys.path.insert(0, os.path.join(HERE, 'scripts'))
    dump(args.out, args.graphs)
    return 0


if __name__ == '__main__':
    sys.exit(main())
