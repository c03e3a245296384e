#!/usr/bin/env python3
"""Serial CompositeLGNN propagation on the composite MUTAG data set (`load_composite_graphs`: one node type; the reference's
starter_composite.py): 5 layers, dim_state = 10, get_state and get_output, selu / softmax with BatchNormalization, max_iteration 5,
threshold 0.01, over the 3 587 training graphs.  One `_propagate` of the training set at each of the four layer boundaries (layer i + 1 is
fed what the route itself relabelled), wall time with a final synchronise, after a warm-up propagation of every width on a 64-graph subset.

Three routes, every run in a fresh child process, alternating, `--repeat` runs each:
  parent_per_graph   the per-graph route of ANOTHER checkout of this repository (`--parent PATH`, built; typically the parent commit)
  per_graph          this checkout's per-graph route (one library call per graph)
  grouped            this checkout's grouped route (one library call per run)
Writes profiles/composite_lgnn_grouped_propagate.json: per boundary the range over the runs, the call counts, the per-phase split of the
grouped route (`last_propagate_seconds`) and the two acceptance ratios grouped / parent_per_graph and per_graph / parent_per_graph.

    python scripts/composite_lgnn_propagate_perf.py [--parent PATH] [--repeat 3] [--limit N] [--out FILE]
    python scripts/composite_lgnn_propagate_perf.py --child ROUTE [--repo PATH]        (one run; prints one JSON line)"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, A, T, LAYERS, L0 = 10, 3, 2, 5, 14


def child(route, repo, limit):
    sys.path.insert(0, repo)
    import numpy as np
    import torch
    from gnnkeras_amd import _native as nat
    from gnnkeras_amd.load_MUTAG import load_composite_graphs
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNgraphBased
    from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
    from gnnkeras_amd.Models.MLP import MLP
    from gnnkeras_amd.Models.training import Adam
    from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer

    def stack():
        gnns = []
        for i in range(LAYERS):
            d_t = L0 + (D + T if i > 0 else 0)                    # the ORIGINAL labels widened by the previous layer's state and output
            ns = [MLP((d_t + 2 * D + d_t + A,), [D], 'selu', 'lecun_normal', 'lecun_normal', rng=10 * i)]
            no = MLP((D,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=10 * i + 1)
            gnns.append(CompositeGNNgraphBased(ns, no, D, 5, 0.01))
        lg = CompositeLGNN(gnns, True, True)
        lg.compile(optimizer=Adam(0.01), loss='categorical_crossentropy', average_st_grads=True, metrics=['accuracy'], training_mode='serial',
                   serial_propagation=route)
        return lg

    seq_of = lambda gl: CompositeMultiGraphSequencer(list(gl), 'g', 'average', 32, shuffle=False)

    def propagate_all(lg, graphs, timed):
        rows, cur = [], list(graphs)
        for li in range(LAYERS - 1):
            seq_now, seq_t0 = seq_of(cur), seq_of(graphs)
            rng = np.random.default_rng(li)
            s0 = [torch.from_numpy(rng.normal(0, 0.1, (g.nodes.shape[0], D)).astype(np.float32)).cuda() for g in cur]
            gc.collect()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            new_seq, ks = lg._propagate(lg.gnns[li], seq_now, seq_t0, s0)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rec = dict(boundary=li, seconds=dt, graphs=len(cur), kernel=nat.lib().gnn_last_kernel_name().decode(), **lg.last_propagate)
            if lg.last_propagate['route'] == 'grouped': rec['split_seconds'] = dict(lg.last_propagate_seconds)
            rec['k_histogram'] = {int(k): int(c) for k, c in zip(*np.unique(ks, return_counts=True))}
            if timed: rows.append(rec)
            cur = new_seq.data
        return rows

    graphs = load_composite_graphs(limit=limit)
    for g in graphs: g.setAggregation('average')
    train = graphs[:-750] if len(graphs) > 1500 else graphs
    propagate_all(stack(), train[:64], timed=False)                # warm-up: every kernel and width of the timed pass
    rows = propagate_all(stack(), train, timed=True)               # (fresh moving statistics; same weights: the initialisers are seeded)
    sizes = np.array([g.nodes.shape[0] for g in train])
    print('RESULT ' + json.dumps(dict(route=route, repo=repo, sources=nat.source_hash(), device=torch.cuda.get_device_name(0), graphs=len(train),
                                      nodes=int(sizes.sum()), rows=rows)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None)
    ap.add_argument('--repo', default=HERE)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--limit', type=int, default=None)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'composite_lgnn_grouped_propagate.json'))
    args = ap.parse_args()
    if args.child: return child(args.child, os.path.abspath(args.repo), args.limit)
    jobs = ([('parent_per_graph', 'per_graph', os.path.abspath(args.parent))] if args.parent else []) + [('per_graph', 'per_graph', HERE), ('grouped', 'grouped', HERE)]
    runs = {name: [] for name, _, _ in jobs}
    for rep in range(args.repeat):
        for name, route, repo in jobs:                              # alternating: every route sees the same drift of the box
            cmd = [sys.executable, os.path.abspath(__file__), '--child', route, '--repo', repo] + (['--limit', str(args.limit)] if args.limit else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            line = next((l_ for l_ in res.stdout.splitlines() if l_.startswith('RESULT ')), None)
            if res.returncode or line is None:
                print(res.stdout[-2000:], res.stderr[-4000:], flush=True)
                raise SystemExit(f'{name} run {rep} failed ({res.returncode})')
            rec = json.loads(line[7:])
            runs[name].append(rec)
            print(name, rep, [round(r_['seconds'], 4) for r_ in rec['rows']], [r_['library_calls'] for r_ in rec['rows']], flush=True)
    out = dict(device=runs['grouped'][0]['device'], graphs=runs['grouped'][0]['graphs'], nodes=runs['grouped'][0]['nodes'], repeat=args.repeat,
               sources={name: r_[0]['sources'] for name, r_ in runs.items()}, boundaries=[])
    for b in range(LAYERS - 1):
        rec = dict(boundary=b)
        for name, rs in runs.items():
            secs = [r_['rows'][b]['seconds'] for r_ in rs]
            last = rs[-1]['rows'][b]
            rec[name] = dict(seconds_min=min(secs), seconds_max=max(secs), seconds_median=sorted(secs)[len(secs) // 2], seconds=secs, library_calls=last['library_calls'], runs=last['runs'],
                             fallback_graphs=last['fallback_graphs'], route=last['route'], kernel=last['kernel'], k_histogram=last['k_histogram'])
            if 'split_seconds' in last: rec[name]['split_seconds'] = last['split_seconds']
        if 'parent_per_graph' in runs:
            # the worst case for the branch: its slowest run against the other checkout's fastest
            rec['grouped_over_parent'] = rec['grouped']['seconds_max'] / rec['parent_per_graph']['seconds_min']
            rec['per_graph_over_parent'] = rec['per_graph']['seconds_max'] / rec['parent_per_graph']['seconds_min']
            rec['per_graph_over_parent_median'] = rec['per_graph']['seconds_median'] / rec['parent_per_graph']['seconds_median']
        out['boundaries'].append(rec)
    if 'parent_per_graph' in runs:
        out['acceptance'] = dict(grouped_at_most_half_of_parent=all(r_['grouped_over_parent'] <= 0.5 for r_ in out['boundaries']),
                                 per_graph_not_slower_than_parent=all(r_['per_graph_over_parent_median'] <= 1.0 for r_ in out['boundaries']))
    with open(args.out, 'w') as fh: json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
