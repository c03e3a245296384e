#!/usr/bin/env python3
"""Batch assembly of heterogeneous data sets: `CompositeMultiGraphSequencer(assemble='host')` (numpy `CompositeGraphObject.merge` + upload
per batch) against `assemble='device'` (`gnnkeras_amd/device_batch.py` `CompositeDeviceDataset`: the data set uploaded once, every merge
one descriptor upload + one `gnn_ragged_copy` launch) on composite MUTAG, all labels kept: one node type as `load_composite_graphs` builds
it ('average'), and the same graphs with three types - the atom kind modulo 3, label widths (14, 9, 5), 'composite_average'.  Batch sizes
32 and 500 (what starter_composite.py uses).  Timed, wall clock with a device synchronise at both ends:

  epoch_end   `on_epoch_end()` with a shuffle: every batch of the epoch merged again
  fit_epoch   one `fit()` epoch (graph focus, state 10, 5 iterations, threshold 0: the same arithmetic whatever the weights)
  propagate   the `assemble` entry of `last_propagate_seconds` of one grouped `CompositeLGNN` propagation over the data set

Both assemblies alternate inside this one process: a warm-up pair, then `--pairs` pairs; medians, ranges and the ratio host / device of
every pair go to profiles/composite_device_assembly.json.

    python scripts/composite_assemble_perf.py [--pairs 5] [--limit N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from gnnkeras_amd import CompositeGraphObject                                   # noqa: E402
from gnnkeras_amd.load_MUTAG import load_composite_graphs                       # noqa: E402
from gnnkeras_amd.Models.CompositeGNN import CompositeGNNgraphBased             # noqa: E402
from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN                     # noqa: E402
from gnnkeras_amd.Models.MLP import MLP                                         # noqa: E402
from gnnkeras_amd.Models.training import Adam                                   # noqa: E402
from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer  # noqa: E402

D, A, T_OUT = 10, 3, 2
CONFIGS = {'one_type': ((14,), 'average'), 'three_types': ((14, 9, 5), 'composite_average')}


def typed(graphs, dims, mode):
    if len(dims) == 1:
        for g in graphs: g.setAggregation(mode)
        return graphs
    return [CompositeGraphObject(nodes=g.nodes, arcs=g.arcs, targets=g.targets, focus='g', dim_node_label=dims, aggregation_mode=mode,
                                 type_mask=np.eye(len(dims), dtype=bool)[np.argmax(g.nodes, axis=1) % len(dims)]) for g in graphs]


def gnn(dims, seed, widen=0):
    w_comp = sum(dims) + len(dims) * widen + A
    ns = [MLP((d_t + widen + 2 * D + w_comp,), [D], 'selu', 'lecun_normal', 'lecun_normal', rng=seed + t) for t, d_t in enumerate(dims)]
    no = MLP((D,), [T_OUT], 'softmax', 'glorot_normal', 'glorot_normal', rng=seed + 9)
    return CompositeGNNgraphBased(ns, no, D, 5, 0.0)


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(graphs, dims, mode, batch_size, assemble, seed):
    seq = CompositeMultiGraphSequencer(list(graphs), 'g', mode, batch_size, shuffle=True, assemble=assemble)
    np.random.seed(seed)
    out = dict(epoch_end=wall(seq.on_epoch_end))
    model = gnn(dims, 0)
    model.compile(optimizer=Adam(0.001), loss='categorical_crossentropy', metrics=['accuracy'])
    np.random.seed(seed)
    out['fit_epoch'] = wall(lambda: model.fit(seq, epochs=1, verbose=0))
    lg = CompositeLGNN([gnn(dims, 20), gnn(dims, 40, widen=D + T_OUT)], True, True)
    lg.compile(optimizer=Adam(0.001), loss='categorical_crossentropy', training_mode='serial', serial_propagation='grouped')
    t0 = CompositeMultiGraphSequencer(list(graphs), 'g', mode, batch_size, shuffle=False, assemble=assemble)
    wall(lambda: lg._propagate(lg.gnns[0], t0._view(), t0))
    assert lg.last_propagate['route'] == 'grouped', lg.last_propagate
    out['propagate'] = lg.last_propagate_seconds['assemble']
    out['propagate_runs'] = lg.last_propagate['runs']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--limit', type=int, default=None)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'composite_device_assembly.json'))
    args = ap.parse_args()
    result = dict(device=torch.cuda.get_device_name(0), graphs=None, pairs=args.pairs, protocol='host and device assembly alternate in '
                  'one process after a warm-up pair; wall seconds with a device synchronise at both ends; ratio = host / device per pair',
                  configs={})
    for name, (dims, mode) in CONFIGS.items():
        graphs = typed(load_composite_graphs(limit=args.limit), dims, mode)
        result['graphs'] = len(graphs)
        for batch_size in (32, 500):
            rows = []
            for pair in range(args.pairs + 1):
                row = {a: measure(graphs, dims, mode, batch_size, a, pair) for a in ('host', 'device')}
                if pair: rows.append(row)                    # pair 0 warms up both paths
            entry = dict(mode=mode, dims=list(dims), batch_size=batch_size, propagate_runs=rows[0]['device']['propagate_runs'])
            for what in ('epoch_end', 'fit_epoch', 'propagate'):
                h, d = [r['host'][what] for r in rows], [r['device'][what] for r in rows]
                entry[what] = dict(host_median=float(np.median(h)), host_range=[min(h), max(h)], device_median=float(np.median(d)),
                                   device_range=[min(d), max(d)], ratio_per_pair=[a / b for a, b in zip(h, d)])
                print(f"{name} batch {batch_size} {what}: host {np.median(h) * 1e3:.2f} ms, device {np.median(d) * 1e3:.2f} ms, "
                      f"host / device {min(entry[what]['ratio_per_pair']):.2f} .. {max(entry[what]['ratio_per_pair']):.2f}", flush=True)
            result['configs'][f'{name}_b{batch_size}'] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f: json.dump(result, f, indent=1)
    print(json.dumps({k: {w: v[w]['ratio_per_pair'] for w in ('epoch_end', 'fit_epoch', 'propagate')} for k, v in result['configs'].items()}))


if __name__ == '__main__':
    main()
