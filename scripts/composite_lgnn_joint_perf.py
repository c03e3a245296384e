#!/usr/bin/env python3
"""The joint CompositeLGNN step ('parallel' / 'residual') on both routes of `compile(composite_joint_step=...)` (docs/joint_lgnn_step.md,
"Composite stacks"): 'blocks' - the building blocks driven from Python, the only route such a stack had - against 'library' - two
`gnn_train_step_composite_ex` calls per layer.  One process, the routes alternating, five pairs, fresh identically seeded models, warm-up
excluded; medians, ranges and the ratio of every pair.  Composite MUTAG (`load_composite_graphs`: one node type, 14 label columns):

  * 'starter': the configuration of the reference's starter_composite.py - 5 layers, d = 10, max_iteration 5, threshold 0.01, selu /
    softmax, get_state and get_output, average_st_grads, batches of 500 graphs;
  * 'd32_k50': batches of 32 graphs, d = 32, max_iteration 50;
each in both training modes: one joint `train_step` (wall time of `--steps` steps ending in a synchronise, per step) and one `fit()`
epoch over `--graphs` graphs.  Before anything is timed, both routes run one step of the timed batch from the same weights and must
agree on k, on the loss (1e-5) and on every gradient within the bar of the parameter gradients (2e-5 of the larger of the tensor's and
the network's largest entry, twice for two float32 results).  Writes profiles/composite_lgnn_joint_step.json.

    python scripts/composite_lgnn_joint_perf.py [--graphs N] [--steps K] [--pairs P] [--skip-fit] [--configs a,b] [--out FILE]

Launches per step come from a kernel trace taken in runs of their own (tracing slows the host: never in the timed process):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/composite_lgnn_joint_perf.py --trace ROUTE --trace-steps N
    python scripts/composite_lgnn_joint_perf.py --count DIR_OF_2_STEPS DIR_OF_6_STEPS        # (launches of 6 steps - launches of 2 steps) / 4
    python scripts/composite_lgnn_joint_perf.py --merge-launches ROUTE COUNT_JSON --out FILE # the printed count of a route into FILE["launches_per_step"]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS, A, T, LAYERS = (14,), 3, 2, 5
CONFIGS = {'starter': dict(d=10, max_iteration=5, batch=500), 'd32_k50': dict(d=32, max_iteration=50, batch=32)}
BAR = 2e-5


def stack(config, mode, route):
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNgraphBased
    from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
    from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
    from gnnkeras_amd.Models.training import Adam
    c = CONFIGS[config]
    gnns = []
    for i in range(LAYERS):
        inp, lay = get_inout_dims('state', DIMS, A, T, 'g', c['d'], layer=i, get_state=True, get_output=True)
        ns = [MLP(k, lay, 'selu', 'lecun_normal', 'lecun_normal', rng=10 * i + t) for t, k in enumerate(inp)]
        no = MLP((c['d'],), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=10 * i + 5)      # (starter_composite.py: the state alone)
        gnns.append(CompositeGNNgraphBased(ns, no, c['d'], c['max_iteration'], 0.01))
    lg = CompositeLGNN(gnns, True, True)
    lg.compile(optimizer=Adam(0.001), loss='categorical_crossentropy', average_st_grads=True, metrics=['accuracy'], training_mode=mode,
               composite_joint_step=route)
    return lg


def summary(values):
    import numpy as np
    v = np.asarray(values, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), values=[float(x) for x in v])


def parity(config, mode, data):
    """One step of each route from the same weights on the timed batch: k, loss and every gradient."""
    import numpy as np
    got = {}
    for route in ('blocks', 'library'):
        lg = stack(config, mode, route)
        logs = lg.train_step(data, seed=1, apply=False)
        assert lg.last_joint_route == route, (lg.last_joint_route, route)
        got[route] = (logs['k'], float(logs['loss']),
                      [[g.detach().cpu().numpy().copy() for g in g_.gradients()] for tp in lg._last_tapes for g_ in list(tp.gs) + [tp.go]])
    (kb, lb, gb), (kl, ll, gl) = got['blocks'], got['library']
    worst = 0.0
    for net_b, net_l in zip(gb, gl):
        scale = max(max(float(np.max(np.abs(t))) for t in net_b), 1e-30)
        for u, v in zip(net_l, net_b): worst = max(worst, float(np.max(np.abs(u - v))) / max(float(np.max(np.abs(v))), scale))
    rec = dict(k_blocks=[int(k) for k in kb], k_library=[int(k) for k in kl], loss_blocks=lb, loss_library=ll, worst_gradient_error=worst, bar=2 * BAR)
    if kb != kl or abs(lb - ll) > 1e-5 * max(1.0, abs(lb)) or worst > 2 * BAR:
        raise SystemExit(f'{config}/{mode}: the routes disagree at the timed size: {json.dumps(rec)}')
    return rec


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
    ap.add_argument('--graphs', type=int, default=0, help='graphs of the fit() epoch (0: the training graphs of starter_composite.py, all but the last 1 500)')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--skip-fit', action='store_true')
    ap.add_argument('--configs', default='starter,d32_k50')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'composite_lgnn_joint_step.json'))
    ap.add_argument('--trace', choices=['blocks', 'library'], help='run --trace-steps steps of --trace-config on this route and exit (under rocprofv3)')
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
    from gnnkeras_amd.load_MUTAG import load_composite_graphs
    from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer
    if not torch.cuda.is_available(): raise SystemExit('this measurement needs the GPU')
    graphs = load_composite_graphs(aggregation_mode='average')
    train = graphs[:-1500]
    if args.graphs > 0: train = train[:args.graphs]
    batch_of = lambda config: CompositeMultiGraphSequencer(list(train[:CONFIGS[config]['batch']]), 'g', 'average', CONFIGS[config]['batch'], shuffle=False)[0]
    if args.trace:
        data = batch_of(args.trace_config)
        lg = stack(args.trace_config, 'parallel', args.trace)
        for _ in range(args.trace_steps): lg.train_step(data, seed=1)
        torch.cuda.synchronize()
        print(args.trace, lg.last_joint_route, args.trace_steps, 'steps')
        return
    out = dict(sources=nat.source_hash(), device=torch.cuda.get_device_name(0), layers=LAYERS, epoch_graphs=len(train), steps_per_timing=args.steps,
               pairs=args.pairs, batches={}, parity={}, results={})
    for config in args.configs.split(','):
        data = batch_of(config)
        out['batches'][config] = dict(graphs=CONFIGS[config]['batch'], nodes=int(data[0][0].shape[0]), arcs=int(data[0][1].shape[0]))
        for mode in ('parallel', 'residual'):
            out['parity'][f'{config}/{mode}'] = parity(config, mode, data)
            rec = dict(step_ms={'blocks': [], 'library': []}, epoch_s={'blocks': [], 'library': []}, k=None)
            for pair in range(args.pairs):
                for route in ('blocks', 'library'):
                    lg = stack(config, mode, route)                 # (fresh, identically seeded weights for every timing)
                    rec['step_ms'][route].append(time_steps(lg, data, args.steps))
                    assert lg.last_joint_route == route, (lg.last_joint_route, route)
                    rec['k'] = [int(k) for k in lg.train_step(data, seed=1)['k']]
                    if not args.skip_fit:
                        np.random.seed(pair)
                        seq = CompositeMultiGraphSequencer(list(train), 'g', 'average', CONFIGS[config]['batch'], shuffle=False)
                        rec['epoch_s'][route].append(time_epoch(stack(config, mode, route), seq, data))
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
