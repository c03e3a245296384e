#!/usr/bin/env python3
"""predict() / evaluate() of a composite (heterogeneous) model over all of composite MUTAG (`load_composite_graphs`: 4 337 graphs, one node
type; the reference's starter_composite.py) in batches of 32, wall time with a final synchronise, in two configurations:

  starter   d = 10, max_iteration 5, threshold 0.01            (the composite starter's)
  long      d = 32, max_iteration 50, threshold 0.01

Two checkouts, every run in a fresh child process, ALTERNATING, `--repeat` pairs (at least five):
  parent    ANOTHER checkout of this repository (`--parent PATH`, built; typically the parent commit): its walk, whatever it plans
  grouped   this checkout: the planner's grouped launches (`CompositeGNN*.Loop(groups=...)` on k_state_lds_types)
  ungrouped this checkout with `group_batches = False` (the batch-by-batch walk, for reference)
Inside a child: two warm-up walks (merges, uploads, plans and kernels cached - what every epoch of fit(validation_data=...) after the first
sees), then `--walks` timed walks of each call; the child reports their median.  Writes profiles/composite_predict_groups.json: per
configuration and call the medians and ranges over the pairs, the ratio grouped / parent of every alternation pair, and the acceptance
(no pair slower than the parent).

    python scripts/composite_predict_perf.py --parent PATH [--repeat 5] [--walks 5] [--limit N] [--out FILE]
    python scripts/composite_predict_perf.py --child MODE [--repo PATH]        (one run; prints one JSON line)"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {'starter': dict(d=10, max_iteration=5, threshold=0.01), 'long': dict(d=32, max_iteration=50, threshold=0.01)}
L0, A, T = 14, 3, 2


def child(mode, repo, limit, walks):
    sys.path.insert(0, repo)
    import numpy as np
    import torch
    from gnnkeras_amd import _native as nat
    from gnnkeras_amd.load_MUTAG import load_composite_graphs
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNgraphBased
    from gnnkeras_amd.Models.MLP import MLP
    from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer

    graphs = load_composite_graphs(limit=limit)
    for g in graphs: g.setAggregation('average')
    seq = CompositeMultiGraphSequencer(list(graphs), 'g', 'average', 32, shuffle=False)
    dev = torch.device('cuda', 0)
    rows = {}
    for name, cfg in CONFIGS.items():
        d = cfg['d']
        ns = [MLP((L0 + 2 * d + L0 + A,), [d], 'selu', 'lecun_normal', 'lecun_normal', rng=0)]
        ns[0].set_weights([a * 0.3 if a.ndim == 2 else a for a in ns[0].get_weights()])
        no = MLP((d,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=1)
        model = CompositeGNNgraphBased(ns, no, d, cfg['max_iteration'], cfg['threshold'])
        model.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
        if mode == 'ungrouped': model.group_batches = False
        plan = model._group_plan(seq, dev)
        rec = dict(plan=None if plan is None else [dict(batches=len(bs), resident=bool(getattr(bs, 'resident', False)), cut=len(getattr(bs, 'parts', {}) or {})) for bs in plan])
        for call in ('predict', 'evaluate'):
            fn = (lambda: model.predict(seq)) if call == 'predict' else (lambda: model.evaluate(seq))
            for _ in range(2): fn()
            torch.cuda.synchronize()
            secs = []
            for _ in range(walks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
            rec[call] = dict(seconds_median=sorted(secs)[len(secs) // 2], seconds=secs, kernel=nat.lib().gnn_last_kernel_name().decode())
        rows[name] = rec
    sizes = np.array([g.nodes.shape[0] for g in graphs])
    print('RESULT ' + json.dumps(dict(mode=mode, repo=repo, sources=nat.source_hash(), device=torch.cuda.get_device_name(0), graphs=len(graphs),
                                      nodes=int(sizes.sum()), batches=len(seq), rows=rows)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None)
    ap.add_argument('--repo', default=HERE)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--walks', type=int, default=5)
    ap.add_argument('--limit', type=int, default=None)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'composite_predict_groups.json'))
    args = ap.parse_args()
    if args.child: return child(args.child, os.path.abspath(args.repo), args.limit, args.walks)
    jobs = ([('parent', 'grouped', os.path.abspath(args.parent))] if args.parent else []) + [('grouped', 'grouped', HERE), ('ungrouped', 'ungrouped', HERE)]
    runs = {name: [] for name, _, _ in jobs}
    for rep in range(args.repeat):
        for name, mode, repo in jobs:                              # alternating: every checkout sees the same drift of the box
            cmd = [sys.executable, os.path.abspath(__file__), '--child', mode, '--repo', repo, '--walks', str(args.walks)] + (['--limit', str(args.limit)] if args.limit else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            line = next((l_ for l_ in res.stdout.splitlines() if l_.startswith('RESULT ')), None)
            if res.returncode or line is None:
                print(res.stdout[-2000:], res.stderr[-4000:], flush=True)
                raise SystemExit(f'{name} run {rep} failed ({res.returncode})')
            rec = json.loads(line[7:])
            runs[name].append(rec)
            print(name, rep, {c: {k_: round(rec['rows'][c][k_]['seconds_median'] * 1e3, 3) for k_ in ('predict', 'evaluate')} for c in CONFIGS}, flush=True)
    first = runs['grouped'][0]
    out = dict(device=first['device'], graphs=first['graphs'], nodes=first['nodes'], batches=first['batches'], batch_size=32, repeat=args.repeat, walks=args.walks,
               unit='seconds per walk over the whole data set (median of the timed walks of a child)',
               sources={name: r_[0]['sources'] for name, r_ in runs.items()}, configurations={})
    ok_all = True
    for c, cfg in CONFIGS.items():
        rec = dict(cfg)
        for call in ('predict', 'evaluate'):
            per = {}
            for name, rs in runs.items():
                secs = [r_['rows'][c][call]['seconds_median'] for r_ in rs]
                per[name] = dict(seconds_median=sorted(secs)[len(secs) // 2], seconds_min=min(secs), seconds_max=max(secs), seconds=secs,
                                 kernel=rs[-1]['rows'][c][call]['kernel'], plan=rs[-1]['rows'][c]['plan'])
            if 'parent' in runs:
                pairs = [g_ / p_ for g_, p_ in zip(per['grouped']['seconds'], per['parent']['seconds'])]
                per['grouped_over_parent_pairs'] = pairs
                per['grouped_over_parent_median'] = per['grouped']['seconds_median'] / per['parent']['seconds_median']
                per['not_slower_in_any_pair'] = all(p_ <= 1.0 for p_ in pairs)
                ok_all = ok_all and per['not_slower_in_any_pair']
            rec[call] = per
        out['configurations'][c] = rec
    if 'parent' in runs: out['acceptance'] = dict(grouped_not_slower_than_parent_in_any_pair=ok_all)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh: json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
