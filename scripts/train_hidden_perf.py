#!/usr/bin/env python3
"""Training steps of state networks with a hidden layer, with and without `FLAG_TRAIN_HIDDEN_SMALL` (include/gnnloop.h): the flag-off
route - the general kernels, one launch per layer and iteration, what such a network ran before the hidden-layer form of the persistent
small-graph kernels existed - against the flag-on route.  One process, the routes alternating, five pairs, warm-up excluded; medians,
ranges and the ratio of every pair.  The one-layer persistent step at the same state width is timed beside them for scale.

  * one `train_step` on a MUTAG batch of 32 graphs at (d, H, max_iteration) = (32, 32, 50) and on the starter shape with a hidden layer
    (d = 0: the state is the 14 label columns, H = 14, max_iteration 5);
  * one `fit()` epoch over `--graphs` MUTAG graphs (default: the 3 587 training graphs) in batches of 32, for each of the two;
  * one joint LGNN step (3 layers, d = 8, H = 12, BatchNormalization, 'parallel', `joint_step='library'`, the flag on every layer).
Writes profiles/train_hidden_small.json.

    python scripts/train_hidden_perf.py [--graphs N] [--steps K] [--pairs P] [--skip-fit] [--out FILE]

Launches per step come from a kernel trace taken in runs of their own (tracing slows the host: never in the timed process):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/train_hidden_perf.py --trace {off,on} --trace-steps N
    python scripts/train_hidden_perf.py --count DIR_OF_2_STEPS DIR_OF_6_STEPS        # (launches of 6 steps - launches of 2 steps) / 4
    python scripts/train_hidden_perf.py --merge-launches {off,on} COUNT_JSON --out FILE"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, A, T = 14, 3, 2
CONFIGS = {'d32_h32_k50': dict(d=32, H=32, max_iteration=50), 'starter_h14_k5': dict(d=0, H=14, max_iteration=5)}
NAMES = {'off': 'train_step: general kernels', 'on': 'train_step: persistent small-graph kernels (hidden layer)',
         'one_layer': 'train_step: persistent small-graph kernels'}


def model(config, route):
    """`route`: 'off' / 'on' (the hidden-layer network without / with the flag) or 'one_layer' (no hidden layer: the scale)."""
    from gnnkeras_amd import _native as nat
    from gnnkeras_amd.Models.GNN import GNNgraphBased
    from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
    from gnnkeras_amd.Models.training import Adam
    c = CONFIGS[config]
    inp, lay = get_inout_dims('state', L, A, T, 'g', c['d'], hidden_units=None if route == 'one_layer' else [c['H']])
    ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=0, batch_normalization=True)
    inp, lay = get_inout_dims('output', L, A, T, 'g', c['d'])
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=1, batch_normalization=True)
    m = GNNgraphBased(ns, no, c['d'], c['max_iteration'], 0.0 if c['max_iteration'] > 5 else 0.01)
    m.compile(optimizer=Adam(0.001), loss='categorical_crossentropy', average_st_grads=True, run_eagerly=True)
    m.native_flags = nat.FLAG_TRAIN_HIDDEN_SMALL if route == 'on' else 0
    return m


def lgnn(route):
    from gnnkeras_amd import _native as nat
    from gnnkeras_amd.Models.GNN import GNNgraphBased
    from gnnkeras_amd.Models.LGNN import LGNN
    from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
    from gnnkeras_amd.Models.training import Adam
    gnns = []
    for i in range(3):
        inp, lay = get_inout_dims('state', L, A, T, 'g', 8, hidden_units=[12], layer=i, get_state=True, get_output=True)
        ns = MLP(inp[0], lay, 'tanh', 'lecun_normal', 'lecun_normal', rng=10 + i, batch_normalization=True)
        inp, lay = get_inout_dims('output', L, A, T, 'g', 8, layer=i, get_state=True, get_output=True)
        no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=20 + i, batch_normalization=True)
        gnns.append(GNNgraphBased(ns, no, 8, 4, 0.0))
        gnns[-1].native_flags = nat.FLAG_TRAIN_HIDDEN_SMALL if route == 'on' else 0
    lg = LGNN(gnns, True, True)
    lg.compile(optimizer=Adam(0.001), loss='categorical_crossentropy', average_st_grads=True, training_mode='parallel', joint_step='library')
    return lg


def summary(values):
    import numpy as np
    v = np.asarray(values, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), values=[float(x) for x in v])


def step_of(m, data):
    from gnnkeras_amd.Models.LGNN import LGNN
    if isinstance(m, LGNN): return lambda: m.train_step(data, seed=1)
    from gnnkeras_amd.Models.training import LoopTrainer
    tr = m._trainer = getattr(m, '_trainer', None) or LoopTrainer(m)
    x, y, sw = data
    return lambda: tr.train_step(x, y, sw, seed=1)


def time_steps(m, data, steps, warmup=3):
    import torch
    step = step_of(m, data)
    for _ in range(warmup): step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps): step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def time_epoch(m, seq, warm_data):
    import torch
    step = step_of(m, warm_data)
    for _ in range(3): step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.fit(seq, epochs=1, verbose=0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def count_rows(d):
    files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
    if not files: raise SystemExit(f'no kernel trace under {d}')
    n = 0
    for f in files:
        with open(f, newline='') as fh: n += max(sum(1 for _ in csv.reader(fh)) - 1, 0)
    return n


def pairs_of(out, key, what, off, on):
    out['results'].setdefault(key, {})[what] = dict(flag_off=summary(off), flag_on=summary(on), ratio_off_over_on=summary([a / b for a, b in zip(off, on)]),
                                                   flag_on_won_every_pair=all(b < a for a, b in zip(off, on)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=0, help='graphs of the fit() epoch (0: the 3 587 training graphs)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--skip-fit', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_hidden_small.json'))
    ap.add_argument('--trace', choices=['off', 'on'], help='run --trace-steps steps of --trace-config on this route and exit (under rocprofv3)')
    ap.add_argument('--trace-steps', type=int, default=2)
    ap.add_argument('--trace-config', default='d32_h32_k50')
    ap.add_argument('--count', nargs=2, metavar=('DIR2', 'DIR6'), help='launches per step from two trace directories (2 and 6 steps)')
    ap.add_argument('--merge-launches', nargs=2, metavar=('ROUTE', 'COUNT_JSON'), help='record the output of --count for a route in --out')
    args = ap.parse_args()
    if args.merge_launches:
        route, path = args.merge_launches
        with open(path) as fh: count = json.loads(fh.read().strip().splitlines()[-1])
        with open(args.out) as fh: out = json.load(fh)
        out.setdefault('launches_per_step', {})[route] = dict(count, config=args.trace_config, source='rocprofv3 --kernel-trace, runs of their own')
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
    name = lambda: nat.lib().gnn_last_kernel_name().decode()
    graphs = [g for g in load_graphs() if g.nodes.shape[0] <= 64]      # (tiles are cut at graph boundaries: graphs of at most 64 nodes)
    for g in graphs: g.setAggregation('average')
    train = graphs[:-750]
    if args.graphs > 0: train = train[:args.graphs]
    batch = MultiGraphSequencer(list(train[:32]), 'g', 'average', 32, shuffle=False)[0]
    if args.trace:
        m = model(args.trace_config, args.trace)
        step = step_of(m, batch)
        for _ in range(args.trace_steps): step()
        torch.cuda.synchronize()
        print(args.trace, name(), args.trace_steps, 'steps')
        return
    out = dict(sources=nat.source_hash(), device=torch.cuda.get_device_name(0), batch=dict(graphs=32, nodes=int(batch[0][0].shape[0]), arcs=int(batch[0][1].shape[0])),
               epoch_graphs=len(train), steps_per_timing=args.steps, pairs=args.pairs, baseline='flag off: the general kernels of the same checkout', results={})
    for config in CONFIGS:
        step = {'off': [], 'on': [], 'one_layer': []}
        epoch = {'off': [], 'on': []}
        for pair in range(args.pairs):
            for route in ('off', 'on', 'one_layer'):
                m = model(config, route)                     # (fresh, identically seeded weights for every timing)
                step[route].append(time_steps(m, batch, args.steps))
                assert name() == NAMES[route], (route, name())
                if not args.skip_fit and route != 'one_layer':
                    np.random.seed(pair)
                    seq = MultiGraphSequencer(list(train), 'g', 'average', 32, shuffle=False)
                    epoch[route].append(time_epoch(model(config, route), seq, batch))
        pairs_of(out, config, 'step_ms', step['off'], step['on'])
        out['results'][config]['one_layer_step_ms'] = summary(step['one_layer'])
        if epoch['off']: pairs_of(out, config, 'epoch_s', epoch['off'], epoch['on'])
        print(config, json.dumps({k: (v['median'] if 'median' in v else {kk: vv['median'] for kk, vv in v.items() if isinstance(vv, dict)})
                                  for k, v in out['results'][config].items()}), flush=True)
    joint = {'off': [], 'on': []}
    for pair in range(args.pairs):
        for route in ('off', 'on'):
            lg = lgnn(route)
            joint[route].append(time_steps(lg, batch, args.steps))
            assert lg.last_joint_route == 'library'
    pairs_of(out, 'lgnn_joint_3x(d8,h12,k4)', 'step_ms', joint['off'], joint['on'])
    print('lgnn', json.dumps({k: v['median'] for k, v in out['results']['lgnn_joint_3x(d8,h12,k4)']['step_ms'].items() if isinstance(v, dict)}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh: json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
