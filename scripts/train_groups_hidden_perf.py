#!/usr/bin/env python3
"""One layer boundary of a serial stack whose state networks have a hidden layer, over the 3 587 MUTAG training graphs: the per-graph route
against the grouped route with `FLAG_TRAIN_GROUPS_HIDDEN` (include/gnnloop.h) on the layer - `LGNN._propagate` of layer 0, wall time with
a final synchronise.  Both routes run in ONE process, alternating, `--pairs` pairs (default 5) after a warm-up propagation of each route on
a 64-graph subset; every run starts from a fresh layer (same weights: the initialisers are seeded).  The baseline is the per-graph route of
this checkout - what ran for these models before the flag existed.

  homogeneous   the starter shape (d = 0, H = 14, 5 iterations, threshold 0.01) and d = 32 / H = 32 / 50 iterations
  composite     the composite starter shape (one node type, d = 10, H = 10, 5 iterations, threshold 0.01)
Records the medians and the range of the per-pair ratios per_graph / grouped in profiles/train_groups_hidden.json.

    python scripts/train_groups_hidden_perf.py [--pairs 5] [--limit N] [--only NAME] [--out FILE]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import numpy as np
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd.load_MUTAG import load_graphs, load_composite_graphs
from gnnkeras_amd.Models.CompositeGNN import CompositeGNNgraphBased
from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
from gnnkeras_amd.Models.GNN import GNNgraphBased
from gnnkeras_amd.Models.LGNN import LGNN
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.training import Adam
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer, MultiGraphSequencer

L, A, T = 14, 3, 2
CONFIGS = {
    'starter d=0 H=14 x5':        dict(kind='homogeneous', d=0, H=14, iters=5),
    'd=32 H=32 x50':              dict(kind='homogeneous', d=32, H=32, iters=50),
    'composite starter d=10 H=10 x5': dict(kind='composite', d=10, H=10, iters=5),
}


def stack(cfg, route):
    """Two layers (the boundary between them is what is timed); the flag on every layer of the grouped route."""
    d, H, iters = cfg['d'], cfg['H'], cfg['iters']
    gnns = []
    for i in range(2):
        if cfg['kind'] == 'homogeneous':
            inp, lay = get_inout_dims('state', L, A, T, 'g', d, hidden_units=[H], layer=i, get_state=True, get_output=True)
            ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=10 * i)
            inp, lay = get_inout_dims('output', L, A, T, 'g', d, layer=i, get_state=True, get_output=True)
            no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=10 * i + 1)
            gnns.append(GNNgraphBased(ns, no, d, iters, 0.01))
        else:
            d_t = L + (d + T if i > 0 else 0)
            ns = [MLP((d_t + 2 * d + d_t + A,), [H, d], 'selu', 'lecun_normal', 'lecun_normal', rng=10 * i)]
            no = MLP((d,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=10 * i + 1)
            gnns.append(CompositeGNNgraphBased(ns, no, d, iters, 0.01))
        gnns[-1].native_flags = nat.FLAG_TRAIN_GROUPS_HIDDEN if route == 'grouped' else 0
    lg = (LGNN if cfg['kind'] == 'homogeneous' else CompositeLGNN)(gnns, True, True)
    lg.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', average_st_grads=True, metrics=['accuracy'], training_mode='serial',
               serial_propagation=route)
    return lg


def one_boundary(cfg, route, graphs):
    lg = stack(cfg, route)
    seq_cls = MultiGraphSequencer if cfg['kind'] == 'homogeneous' else CompositeMultiGraphSequencer
    seq_now, seq_t0 = seq_cls(list(graphs), 'g', 'average', 32, shuffle=False), seq_cls(list(graphs), 'g', 'average', 32, shuffle=False)
    s0 = None
    if cfg['d'] > 0:
        rng = np.random.default_rng(0)
        s0 = [torch.from_numpy(rng.normal(0, 0.1, (g.nodes.shape[0], cfg['d'])).astype(np.float32)).cuda() for g in graphs]
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    new_seq, ks = lg._propagate(lg.gnns[0], seq_now, seq_t0, s0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec = dict(seconds=dt, kernel=nat.lib().gnn_last_kernel_name().decode(), **lg.last_propagate)
    rec['k_histogram'] = {int(k): int(c) for k, c in zip(*np.unique(ks, return_counts=True))}
    if rec['route'] != route: raise SystemExit(f'{route} was asked for, {rec["route"]} ran: {rec}')
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--limit', type=int, default=None)
    ap.add_argument('--only', default=None, help='substring of the configurations to run (default: all)')
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'train_groups_hidden.json'))
    args = ap.parse_args()
    data = {}
    for kind, load in (('homogeneous', load_graphs), ('composite', load_composite_graphs)):
        graphs = load()
        for g in graphs: g.setAggregation('average')
        train = graphs[:-750]
        data[kind] = train[:args.limit] if args.limit else train
    sizes = np.array([g.nodes.shape[0] for g in data['homogeneous']])
    out = dict(graphs=len(sizes), nodes=int(sizes.sum()), graphs_above_group_size=int((sizes > nat.TRAIN_GROUP_MAX_NODES).sum()), pairs=args.pairs,
               sources=nat.source_hash(), device=torch.cuda.get_device_name(0),
               baseline="the per-graph route of the same checkout: what runs for these models without GNN_FLAG_TRAIN_GROUPS_HIDDEN", configurations={})
    for name, cfg in CONFIGS.items():
        if args.only and args.only not in name: continue
        graphs = data[cfg['kind']]
        for route in ('per_graph', 'grouped'): one_boundary(cfg, route, graphs[:64])          # warm-up: every kernel of the timed runs
        runs = {'per_graph': [], 'grouped': []}
        for p in range(args.pairs):
            for route in ('per_graph', 'grouped'):
                runs[route].append(one_boundary(cfg, route, graphs))
                print(name, p, route, json.dumps(runs[route][-1]), flush=True)
        ratios = [a['seconds'] / b['seconds'] for a, b in zip(runs['per_graph'], runs['grouped'])]
        rec = dict(cfg, median_seconds={r: statistics.median(x['seconds'] for x in runs[r]) for r in runs}, pair_ratios=ratios,
                   ratio_range=[min(ratios), max(ratios)], ratio_median=statistics.median(ratios), grouped_wins_every_pair=min(ratios) > 1.0,
                   same_k=all(x['k_histogram'] == runs['per_graph'][0]['k_histogram'] for r in runs for x in runs[r]), runs=runs)
        out['configurations'][name] = rec
        print(f'{name}: per_graph {rec["median_seconds"]["per_graph"]:.3f} s, grouped {rec["median_seconds"]["grouped"]:.3f} s, '
              f'ratio {min(ratios):.2f} .. {max(ratios):.2f} (median {rec["ratio_median"]:.2f})', flush=True)
        with open(args.out, 'w') as fh: json.dump(out, fh, indent=1)
    print(json.dumps({k: (v['median_seconds'], v['ratio_range']) for k, v in out['configurations'].items()}))


if __name__ == '__main__':
    main()
