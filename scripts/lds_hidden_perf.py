#!/usr/bin/env python3
"""predict() / evaluate() over all of MUTAG (4 337 graphs, batches of 32) with a state network Dense(H) - Dense(state width): the
hidden-layer form of the one-CU-per-group kernels (`model.native_flags |= nat.FLAG_LDS_HIDDEN`) against the route the same model takes
without the flag - the spread form (k_state_small<.., L2>, runs of ~16 batches) for a homogeneous model, the batch-by-batch walk for a
composite one.  The baseline is the flag-off route of THIS checkout, which by construction is the route of the commit before the flag
existed (without the flag every answer of the library is unchanged: tests/test_lds_hidden_route_host.py).

  hom_d32       homogeneous, d = 32, H = 32, tanh, 50 iterations, threshold 0
  hom_starter   homogeneous, d = 0 (the 14 label columns are the state), H = 14, 5 iterations, threshold 0.01 (the starter shape + a hidden layer)
  comp_d32, comp_starter   the same two on composite MUTAG (`load_composite_graphs`: one node type)

One process; flag off and flag on ALTERNATE, `--repeat` pairs (at least five), `--walks` timed walks per call and turn after two warm-up
walks per route (merges, uploads, plans and kernels cached), wall time with a final synchronise.  Before timing: the kernel name of each
route, and both routes must agree on k (exactly), state and output (rel_err <= 1e-5) on the first four batches.  Writes
profiles/lds_hidden_groups.json: medians per route, the ratio on / off of every pair with its range, and whether the flag won every pair.

    python scripts/lds_hidden_perf.py [--repeat 5] [--walks 3] [--limit N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
L0, A, T = 14, 3, 2
CONFIGS = {'hom_d32': dict(composite=False, d=32, H=32, max_iteration=50, threshold=0.0),
           'hom_starter': dict(composite=False, d=0, H=14, max_iteration=5, threshold=0.01),
           'comp_d32': dict(composite=True, d=32, H=32, max_iteration=50, threshold=0.0),
           'comp_starter': dict(composite=True, d=0, H=14, max_iteration=5, threshold=0.01)}


def rel_err(a, b):
    import numpy as np
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30)) if a.size else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--walks', type=int, default=3)
    ap.add_argument('--limit', type=int, default=None)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'lds_hidden_groups.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from gnnkeras_amd import _native as nat
    from gnnkeras_amd import ops
    from gnnkeras_amd.load_MUTAG import load_composite_graphs, load_graphs
    from gnnkeras_amd.Models.CompositeGNN import CompositeGNNgraphBased
    from gnnkeras_amd.Models.GNN import GNNgraphBased
    from gnnkeras_amd.Models.MLP import MLP
    from gnnkeras_amd.Sequencers.GraphSequencers import CompositeMultiGraphSequencer, MultiGraphSequencer

    dev = torch.device('cuda', 0)
    last = lambda: nat.lib().gnn_last_kernel_name().decode()
    seqs = {}
    out = dict(device=torch.cuda.get_device_name(0), batch_size=32, repeat=args.repeat, walks=args.walks, sources=nat.source_hash(),
               unit='seconds per walk over the whole data set (median of the timed walks of a turn)',
               baseline='the flag-off route of the same checkout: the route of the commit before GNN_FLAG_LDS_HIDDEN existed', configurations={})
    for name, cfg in CONFIGS.items():
        comp, d, H = cfg['composite'], cfg['d'], cfg['H']
        if comp not in seqs:
            graphs = (load_composite_graphs if comp else load_graphs)(limit=args.limit)
            for g in graphs: g.setAggregation('average')
            seqs[comp] = (CompositeMultiGraphSequencer if comp else MultiGraphSequencer)(list(graphs), 'g', 'average', 32, shuffle=False)
            out.update(graphs=len(graphs), nodes=int(sum(g.nodes.shape[0] for g in graphs)), batches=len(seqs[comp]))
        seq = seqs[comp]
        S = d or L0
        in_dim = (L0 + 2 * S + L0 + A) if comp else (2 * S + 2 * L0 + A if d else 2 * S + A)
        ns = MLP((in_dim,), [H, S], ['tanh', 'tanh'], 'lecun_normal', 'lecun_normal', rng=0)
        ns.set_weights([w * 0.3 if w.ndim == 2 else w for w in ns.get_weights()])
        no = MLP((S if comp or not d else S + L0,), [T], 'softmax', 'glorot_normal', 'glorot_normal', rng=1)
        model = (CompositeGNNgraphBased([ns], no, d, cfg['max_iteration'], cfg['threshold']) if comp else
                 GNNgraphBased(ns, no, d, cfg['max_iteration'], cfg['threshold']))
        model.compile(optimizer='adam', loss='categorical_crossentropy', metrics=['accuracy'])
        routes = {'off': 0, 'on': nat.FLAG_LDS_HIDDEN}
        # ---- both routes agree: the flag's grouped launch over four batches against the flag-off call on each batch alone --------
        # (the first four batches that fit one CU whole: the planner cuts the larger ones into group sets)
        limit = ops.loop_group_max_nodes(L0, A, model.net_state, model.net_output, d, cfg['max_iteration'], nat.FOCUS['g'], [L0] if comp else None,
                                         flags=routes['on'])
        bs = [b for b in range(len(seq)) if seq[b][0][0].shape[0] <= limit][:4]
        x, begin = seq.merged_batches(bs)
        rng = np.random.default_rng(1)
        s0s = [torch.from_numpy(rng.normal(0, 0.1, (begin[j + 1] - begin[j], d)).astype(np.float32)).to(dev) if d else None for j in range(len(bs))]
        model.native_flags = routes['on']
        k, st, o = model.Loop(*model.process_inputs(x), state0=torch.cat(s0s) if d else None, groups=begin)
        name_on = last()
        assert name_on.startswith('k_state_lds_types<' if comp else 'k_state_lds<') and name_on.endswith(',hidden>'), name_on
        model.native_flags = routes['off']
        agree, r0 = dict(k=[], state=0.0, out=0.0), 0
        for j, b in enumerate(bs):
            kb, stb, ob = model.Loop(*model.process_inputs(seq[b][0]), state0=s0s[j])
            assert float(kb) == float(k[j]), (name, b, float(kb), float(k[j]))
            agree['k'].append(float(kb))
            agree['state'] = max(agree['state'], rel_err(st[begin[j]:begin[j + 1]].cpu().numpy(), stb.cpu().numpy()))
            agree['out'] = max(agree['out'], rel_err(o[r0:r0 + ob.shape[0]].cpu().numpy(), ob.cpu().numpy()))
            r0 += ob.shape[0]
        assert agree['state'] <= 1e-5 and agree['out'] <= 1e-5, (name, agree)
        # ---- plans and kernel names of the two walks ----------------------------------------------------------------------------------
        rec = dict(cfg, agreement=agree, routes={})
        calls = {'predict': lambda: model.predict(seq), 'evaluate': lambda: model.evaluate(seq)}
        for route, flags in routes.items():
            model.native_flags = flags
            plan = model._group_plan(seq, dev)
            for fn in calls.values():
                for _ in range(2): fn()
            torch.cuda.synchronize()
            rec['routes'][route] = dict(kernel=last(), plan=None if plan is None else
                                        [dict(batches=len(b_), resident=bool(getattr(b_, 'resident', False)), cut=len(getattr(b_, 'parts', {}) or {})) for b_ in plan])
        assert rec['routes']['on']['kernel'].endswith(',hidden>') and any(p_['resident'] for p_ in rec['routes']['on']['plan']), rec['routes']['on']
        assert not rec['routes']['off']['kernel'].startswith('k_state_lds'), rec['routes']['off']
        # ---- timing: off / on alternating -----------------------------------------------------------------------------------------------
        secs = {call: {route: [] for route in routes} for call in calls}
        for rep in range(args.repeat):
            for route, flags in routes.items():
                model.native_flags = flags
                for call, fn in calls.items():
                    ts = []
                    for _ in range(args.walks):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        ts.append(time.perf_counter() - t0)
                    secs[call][route].append(sorted(ts)[len(ts) // 2])
        for call in calls:
            med = {route: sorted(v)[len(v) // 2] for route, v in secs[call].items()}
            pairs = [on / off for on, off in zip(secs[call]['on'], secs[call]['off'])]
            rec[call] = dict(seconds_median=med, seconds=secs[call], on_over_off_pairs=pairs, on_over_off_min=min(pairs), on_over_off_max=max(pairs),
                             on_over_off_median=sorted(pairs)[len(pairs) // 2], flag_won_every_pair=all(p_ < 1.0 for p_ in pairs))
            print(name, call, {r_: round(v * 1e3, 3) for r_, v in med.items()}, 'on / off pairs', [round(p_, 3) for p_ in pairs], flush=True)
        out['configurations'][name] = rec
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh: json.dump(out, fh, indent=1)
    print(json.dumps({c: {call: r_[call]['on_over_off_median'] for call in ('predict', 'evaluate')} for c, r_ in out['configurations'].items()}))


if __name__ == '__main__':
    main()
