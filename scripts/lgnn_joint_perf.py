#!/usr/bin/env python3
"""The joint LGNN step ('parallel' / 'residual') on both routes of `LGNN.joint_step` (docs/joint_lgnn_step.md): 'blocks' - the building
blocks driven from Python, the arithmetic and launch sequence of the step before the library route existed - against 'library' - two
library calls per layer.  One process, the routes alternating, five pairs, warm-up excluded; medians, ranges and the ratio of every pair.

  * one joint `train_step` on a MUTAG batch of 32 graphs (wall time of `--steps` steps ending in a synchronise, per step);
  * one `fit()` epoch over `--graphs` MUTAG graphs (default: the 3 587 training graphs) in batches of 32;
for the 3-layer starter stack (d = 0, selu / softmax, BatchNormalization, max_iteration 5, threshold 0.01, get_state and get_output) and
for d = 32 / max_iteration 50, both training modes.  Writes profiles/lgnn_joint_step.json.

    python scripts/lgnn_joint_perf.py [--graphs N] [--steps K] [--pairs P] [--skip-fit] [--out FILE]

Launches per step come from a kernel trace taken in runs of their own (tracing slows the host: never in the timed process):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/lgnn_joint_perf.py --trace ROUTE --trace-steps N
    python scripts/lgnn_joint_perf.py --count DIR_OF_2_STEPS DIR_OF_6_STEPS        # (launches of 6 steps - launches of 2 steps) / 4
    python scripts/lgnn_joint_perf.py --merge-launches ROUTE COUNT_JSON --out FILE # the printed count of a route into FILE["launches_per_step"]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, A, T, LAYERS = 14, 3, 2, 3
CONFIGS = {'starter': dict(d=0, max_iteration=5), 'd32_k50': dict(d=32, max_iteration=50)}


def stack(config, mode, route):
    from gnnkeras_amd.Models.GNN import GNNgraphBased
    from gnnkeras_amd.Models.LGNN import LGNN
    from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
    from gnnkeras_amd.Models.training import Adam
    c = CONFIGS[config]
    gnns = []
    for i in range(LAYERS):
        inp, lay = get_inout_dims('state', L, A, T, 'g', c['d'], layer=i, get_state=True, get_output=True)
        ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=10 * i)
        inp, lay = get_inout_dims('output', L, A, T, 'g', c['d'], layer=i, get_state=True, get_output=True)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=10 * i + 1)
        gnns.append(GNNgraphBased(ns, no, c['d'], c['max_iteration'], 0.01))
    lg = LGNN(gnns, True, True)
    lg.compile(optimizer=Adam(0.001), loss='categorical_crossentropy', average_st_grads=True, metrics=['accuracy'], training_mode=mode, joint_step=route)
    return lg


def summary(values):
    import numpy as np
    v = np.asarray(values, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), values=[float(x) for x in v])


def time_steps(lg, data, steps, warmup=3):
    import torch
    for _ in range(warmup): lg.train_step(data, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps): lg.train_step(data, seed=1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def time_epoch(lg, seq, warm_data):
    import torch
    for _ in range(3): lg.train_step(warm_data, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lg.fit(seq, epochs=1, verbose=0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def count_rows(d):
    files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    if not files: raise SystemExit(f'no kernel trace under {d}')
    n = 0
    for f in files:
        with open(f, newline='') as fh: n += max(sum(1 for _ in csv.reader(fh)) - 1, 0)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=0, help='graphs of the fit() epoch (0: the 3 587 training graphs)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--skip-fit', action='store_true')
    ap.add_argument('--configs', default='starter,d32_k50')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lgnn_joint_step.json'))
    ap.add_argument('--trace', choices=['blocks', 'library'], help='run --trace-steps steps of the starter stack on this route and exit (under rocprofv3)')
    ap.add_argument('--trace-steps', type=int, default=2)
    ap.add_argument('--trace-config', default='starter')
    ap.add_argument('--count', nargs=2, metavar=('DIR2', 'DIR6'), help='launches per step from two trace directories (2 and 6 steps)')
    ap.add_argument('--merge-launches', nargs=2, metavar=('ROUTE', 'COUNT_JSON'), help='record the output of --count for a route in --out')
    args = ap.parse_args()
    if args.merge_launches:
        route, path = args.merge_launches
        with open(path) as fh: count = json.loads(fh.read().strip().splitlines()[-1])
        with open(args.out) as fh: out = json.load(fh)
        out.setdefault('launches_per_step', {})[route] = dict(count, config=args.trace_config, mode='parallel', source='rocprofv3 --kernel-trace, runs of their own')
        with open(args.out, 'w') as fh: json.dump(out, fh, indent=1)
        return
    if args.count:
        n2, n6 = count_rows(args.count[0]), count_rows(args.count[1])
        print(json.dumps(dict(launches_2_steps=n2, launches_6_steps=n6, launches_per_step=(n6 - n2) / 4.0)))
        return
    import numpy as np
    import torch
    from gnnkeras_amd import _native as nat
    from gnnkeras_amd.load_MUTAG import load_graphs
    from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer
    if not torch.cuda.is_available(): raise SystemExit('this measurement needs the GPU')
    graphs = load_graphs()
    for g in graphs: g.setAggregation('average')
    train = graphs[:-750]
    if args.graphs > 0: train = train[:args.graphs]
    batch = MultiGraphSequencer(list(train[:32]), 'g', 'average', 32, shuffle=False)[0]
    if args.trace:
        lg = stack(args.trace_config, 'parallel', args.trace)
        for _ in range(args.trace_steps): lg.train_step(batch, seed=1)
        torch.cuda.synchronize()
        print(args.trace, lg.last_joint_route, args.trace_steps, 'steps')
        return
    out = dict(sources=nat.source_hash(), device=torch.cuda.get_device_name(0), batch=dict(graphs=32, nodes=int(batch[0][0].shape[0]), arcs=int(batch[0][1].shape[0])),
               epoch_graphs=len(train), steps_per_timing=args.steps, pairs=args.pairs, results={})
    for config in args.configs.split(','):
        for mode in ('parallel', 'residual'):
            rec = dict(step_ms={'blocks': [], 'library': []}, epoch_s={'blocks': [], 'library': []}, k=None)
            for pair in range(args.pairs):
                for route in ('blocks', 'library'):
                    lg = stack(config, mode, route)                 # (fresh, identically seeded weights for every timing)
                    rec['step_ms'][route].append(time_steps(lg, batch, args.steps))
                    assert lg.last_joint_route == route, (lg.last_joint_route, route)
                    rec['k'] = [int(k) for k in lg.train_step(batch, seed=1)['k']]
                    if not args.skip_fit:
                        np.random.seed(pair)
                        seq = MultiGraphSequencer(list(train), 'g', 'average', 32, shuffle=False)
                        rec['epoch_s'][route].append(time_epoch(stack(config, mode, route), seq, batch))
            res = dict(k=rec['k'])
            for key in ('step_ms', 'epoch_s'):
                if not rec[key]['blocks']: continue
                res[key] = dict(blocks=summary(rec[key]['blocks']), library=summary(rec[key]['library']),
                                ratio_blocks_over_library=summary([b / l for b, l in zip(rec[key]['blocks'], rec[key]['library'])]))
            out['results'][f'{config}/{mode}'] = res
            print(config, mode, json.dumps({k: (v if k == 'k' else {kk: vv['median'] for kk, vv in v.items()}) for k, v in res.items()}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh: json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
