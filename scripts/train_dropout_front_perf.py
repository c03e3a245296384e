#!/usr/bin/env python3
"""Training steps of a state network with a Dropout layer in FRONT of its first Dense (position 0), with and without
`FLAG_TRAIN_DROPOUT_FRONT` (include/gnnloop.h): the flag-off route - the Python building blocks (`LoopTrainer._mlp_forward` /
`_mlp_backward`, the `drop0` branches), what such a model runs without the flag and ran before it existed - against the in-library step
on the general kernels.  One process, the routes alternating, five pairs, warm-up excluded; medians, ranges and the ratio of every pair.
Before anything is timed, one step of both routes from the same weights and the same seed must agree by the route-agreement rule of
tests/test_gpu_train_dropout_front.py: the same k, every gradient tensor within 2 x BARS['kernel'] (tests/test_gpu_training.py).

  * one `train_step` on a MUTAG batch of 32 graphs at
      d32_k50      d = 32, one Dense, 50 iterations, threshold 0, BatchNormalization, Dropout 0.2 at position 0 of the state network
      starter_k5   the starter shape (d = 0: the state is the 14 label columns, 5 iterations) with the same layer
  * one `fit()` epoch over `--graphs` MUTAG graphs (default: the training graphs of at most 64 nodes) in batches of 32, for both.
Writes profiles/train_dropout_front.json.

    python scripts/train_dropout_front_perf.py [--graphs N] [--steps K] [--pairs P] [--skip-fit] [--out FILE]

Launches per step come from a kernel trace taken in runs of their own (tracing slows the host: never in the timed process):

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/train_dropout_front_perf.py --trace {off,on} --trace-steps N
    python scripts/train_dropout_front_perf.py --count DIR_OF_2_STEPS DIR_OF_6_STEPS        # (launches of 6 steps - launches of 2 steps) / 4
    python scripts/train_dropout_front_perf.py --merge-launches {off,on} COUNT_JSON --out FILE"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from train_hidden_perf import count_rows, pairs_of, summary, time_epoch, time_steps      # noqa: E402, F401  (the same timing loops)

L, A, T = 14, 3, 2
CONFIGS = {'d32_k50': dict(d=32, max_iteration=50, rate=0.2), 'starter_k5': dict(d=0, max_iteration=5, rate=0.2)}
ON = 'train_step: general kernels (dropout in front)'
GRADIENT_BAR = 2 * 2e-5                     # 2 x BARS['kernel'] of tests/test_gpu_training.py: two float32 routes that each keep the bar


def model(config, route):
    """`route`: 'off' / 'on' - the model without / with the flag."""
    from gnnkeras_amd import _native as nat
    from gnnkeras_amd.Models.GNN import GNNgraphBased
    from gnnkeras_amd.Models.MLP import MLP, get_inout_dims
    from gnnkeras_amd.Models.training import Adam
    c = CONFIGS[config]
    inp, lay = get_inout_dims('state', L, A, T, 'g', c['d'])
    ns = MLP(inp[0], lay, 'selu', 'lecun_normal', 'lecun_normal', rng=0, batch_normalization=True, dropout_rate=[c['rate']], dropout_pos=[0])
    inp, lay = get_inout_dims('output', L, A, T, 'g', c['d'])
    no = MLP(inp[0], lay, 'softmax', 'glorot_normal', 'glorot_normal', rng=1, batch_normalization=True)
    m = GNNgraphBased(ns, no, c['d'], c['max_iteration'], 0.0 if c['max_iteration'] > 5 else 0.01)
    m.compile(optimizer=Adam(0.001), loss='categorical_crossentropy', average_st_grads=True, run_eagerly=True)
    m.native_flags = nat.FLAG_TRAIN_DROPOUT_FRONT if route == 'on' else 0
    return m


def ran_as_asked(route, trainer, name):
    """The flag's route names itself; without the flag the trainer does not ask the library for a step at all (the building blocks)."""
    return name() == ON if route == 'on' else not trainer._native_step_applies(True)


def agreement(config, batch, name):
    """One step (not applied) of both routes from the same weights and seed: k, loss, the worst gradient entry relative to the larger of
    its tensor's and its network's largest entry."""
    import numpy as np
    import torch
    from gnnkeras_amd.Models.training import LoopTrainer
    x, y, sw = batch
    got = {}
    for route in ('off', 'on'):
        m = model(config, route)
        tr = LoopTrainer(m)
        res = tr.train_step(x, y, sw, apply=False, seed=1)
        torch.cuda.synchronize()
        assert ran_as_asked(route, tr, name), (route, name())
        got[route] = (int(res['k']), float(res['loss']), [[g.detach().cpu().numpy().copy() for g in h.gradients()] for h in (tr.gs, tr.go)])
    worst = 0.0
    for net_on, net_off in zip(got['on'][2], got['off'][2]):
        scale = max(float(np.max(np.abs(t))) for t in net_off)
        for u, v in zip(net_on, net_off): worst = max(worst, float(np.max(np.abs(u - v))) / max(float(np.max(np.abs(v))), scale, 1e-30))
    out = dict(k_off=got['off'][0], k_on=got['on'][0], loss_off=got['off'][1], loss_on=got['on'][1], worst_gradient_entry=worst, gradient_bar=GRADIENT_BAR)
    print(config, 'agreement', json.dumps(out), flush=True)
    if out['k_off'] != out['k_on'] or abs(out['loss_on'] - out['loss_off']) > 2e-5 * max(1.0, abs(out['loss_off'])) or worst > GRADIENT_BAR:
        raise SystemExit(f'{config}: the two routes disagree: {out}')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=0, help='graphs of the fit() epoch (0: the training graphs of at most 64 nodes)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--skip-fit', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_dropout_front.json'))
    ap.add_argument('--trace', choices=['off', 'on'], help='run --trace-steps steps of --trace-config on this route and exit (under rocprofv3)')
    ap.add_argument('--trace-steps', type=int, default=2)
    ap.add_argument('--trace-config', default='d32_k50')
    ap.add_argument('--count', nargs=2, metavar=('DIR2', 'DIR6'), help='launches per step from two trace directories (2 and 6 steps)')
    ap.add_argument('--merge-launches', nargs=2, metavar=('ROUTE', 'COUNT_JSON'), help='record the output of --count for a route in --out')
    args = ap.parse_args()
    if args.merge_launches:
        route, path = args.merge_launches
        with open(path) as fh: count = json.loads(fh.read().strip().splitlines()[-1])
        with open(args.out) as fh: out = json.load(fh)
        out.setdefault('launches_per_step', {}).setdefault(args.trace_config, {})[route] = dict(count, source='rocprofv3 --kernel-trace, runs of their own')
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
    from train_hidden_perf import step_of
    if not torch.cuda.is_available(): raise SystemExit('this measurement needs the GPU')
    name = lambda: nat.lib().gnn_last_kernel_name().decode()
    graphs = [g for g in load_graphs() if g.nodes.shape[0] <= 64]      # (the data of scripts/train_dropout_perf.py)
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
               epoch_graphs=len(train), steps_per_timing=args.steps, pairs=args.pairs,
               baseline='flag off: the building blocks of the same checkout (what a model with dropout_pos = 0 ran before the flag existed)', agreement={}, results={})
    for config in CONFIGS: out['agreement'][config] = agreement(config, batch, name)
    for config in CONFIGS:
        step = {'off': [], 'on': []}
        epoch = {'off': [], 'on': []}
        for pair in range(args.pairs):
            for route in ('off', 'on'):
                m = model(config, route)                     # (fresh, identically seeded weights for every timing)
                step[route].append(time_steps(m, batch, args.steps))
                assert ran_as_asked(route, m._trainer, name), (route, name())
                if not args.skip_fit:
                    np.random.seed(pair)
                    seq = MultiGraphSequencer(list(train), 'g', 'average', 32, shuffle=False)
                    epoch[route].append(time_epoch(model(config, route), seq, batch))
        pairs_of(out, config, 'step_ms', step['off'], step['on'])
        if epoch['off']: pairs_of(out, config, 'epoch_s', epoch['off'], epoch['on'])
        print(config, json.dumps({k: {kk: vv['median'] for kk, vv in v.items() if isinstance(vv, dict)} for k, v in out['results'][config].items()}), flush=True)
    out['flag_on_won_every_pair_of_every_configuration'] = all(w['flag_on_won_every_pair'] for r in out['results'].values() for w in r.values())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh: json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
