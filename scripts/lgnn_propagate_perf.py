#!/usr/bin/env python3
"""Serial LGNN propagation on all of MUTAG, both routes (`LGNN.serial_propagation`): the starter stack (3 layers, d = 0, selu / softmax,
BatchNormalization, max_iteration 5, threshold 0.01) over 3 587 training + 750 validation graphs.

  * one `_propagate` of the training set per route at each of the two layer boundaries (layer i + 1 is fed what the route itself
    relabelled), wall time with a final synchronise, after a warm-up propagation of every shape on a 64-graph subset;
  * one serial `fit()` epoch per route.
Prints the record and writes it to profiles/lgnn_grouped_propagate.json.

    python scripts/lgnn_propagate_perf.py [--skip-fit] [--out profiles/lgnn_grouped_propagate.json]"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd.load_MUTAG import load_graphs
from gnnkeras_amd.Models.GNN import GNNgraphBased
from gnnkeras_amd.Models.LGNN import LGNN
from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
from gnnkeras_amd.Models.training import Adam
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer

L, A, T, LAYERS = 14, 3, 2, 3


def stack(route):
    gnns = []
    for i in range(LAYERS):
        inp, lay = get_inout_dims('state', L, A, T, 'g', 0, layer=i, get_state=True, get_output=True)
        ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=10 * i)
        inp, lay = get_inout_dims('output', L, A, T, 'g', 0, layer=i, get_state=True, get_output=True)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=10 * i + 1)
        gnns.append(GNNgraphBased(ns, no, 0, 5, 0.01))
    lg = LGNN(gnns, True, True)
    lg.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', average_st_grads=True, metrics=['accuracy'], training_mode='serial',
               serial_propagation=route)
    return lg


def seq_of(graphs, batch=32):
    return MultiGraphSequencer(list(graphs), 'g', 'average', batch, shuffle=False)


def propagate_all(lg, graphs, timed):
    """Both layer boundaries over `graphs`; returns one record per boundary."""
    rows, cur = [], list(graphs)
    for li in range(LAYERS - 1):
        seq_now, seq_t0 = seq_of(cur), seq_of(graphs)
        gc.collect()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        new_seq, ks = lg._propagate(lg.gnns[li], seq_now, seq_t0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rec = dict(boundary=li, seconds=dt, graphs=len(cur), kernel=nat.lib().gnn_last_kernel_name().decode(), **lg.last_propagate)
        if lg.last_propagate['route'] == 'grouped': rec['split_seconds'] = dict(lg.last_propagate_seconds)
        rec['k_histogram'] = {int(k): int(c) for k, c in zip(*np.unique(ks, return_counts=True))}
        if timed: rows.append(rec)
        cur = new_seq.data
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-fit', action='store_true')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'lgnn_grouped_propagate.json'))
    args = ap.parse_args()
    graphs = load_graphs()
    for g in graphs: g.setAggregation('average')
    train, valid = graphs[:-750], graphs[-750:]
    sizes = np.array([g.nodes.shape[0] for g in train])
    out = dict(train_graphs=len(train), valid_graphs=len(valid), nodes=int(sizes.sum()), graphs_above_group_size=int((sizes > nat.TRAIN_GROUP_MAX_NODES).sum()),
               sources=nat.source_hash(), device=torch.cuda.get_device_name(0), propagate={}, fit_epoch_seconds={})
    for route in ('per_graph', 'grouped'):
        lg = stack(route)
        propagate_all(lg, train[:64], timed=False)              # warm-up: every kernel and width of the timed passes
        lg = stack(route)                                       # (fresh moving statistics; same weights: the initialisers are seeded)
        out['propagate'][route] = propagate_all(lg, train, timed=True)
        for r_ in out['propagate'][route]: print(route, json.dumps(r_), flush=True)
    for b in range(LAYERS - 1):
        a_, g_ = out['propagate']['per_graph'][b], out['propagate']['grouped'][b]
        out.setdefault('speedup', []).append(a_['seconds'] / g_['seconds'])
        print(f'boundary {b}: per_graph {a_["seconds"]:.3f} s ({a_["library_calls"]} calls), grouped {g_["seconds"]:.3f} s ({g_["library_calls"]} calls, '
              f'{g_["fallback_graphs"]} fallback graphs): x{a_["seconds"] / g_["seconds"]:.1f}', flush=True)
    if not args.skip_fit:
        for route in ('per_graph', 'grouped'):
            lg = stack(route)
            np.random.seed(0)
            tr, va = MultiGraphSequencer(list(train), 'g', 'average', 32), MultiGraphSequencer(list(valid), 'g', 'average', 32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lg.fit(tr, epochs=1, validation_data=va, verbose=0)
            torch.cuda.synchronize()
            out['fit_epoch_seconds'][route] = time.perf_counter() - t0
            print(f'serial fit, 1 epoch per layer, {route}: {out["fit_epoch_seconds"][route]:.2f} s', flush=True)
    with open(args.out, 'w') as fh: json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
