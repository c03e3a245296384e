"""Layered GNN (LGNN): a stack of GNNs, layer i+1 sees the original labels extended with the state and/or output of
layer i. Host-side orchestration over the device loop — mirror of the reference's `GNN/Models/LGNN.py`
(constructor, `compile(training_mode=...)`, `call`, `Loop`, `update_graph`, `train_step`, serial `fit`, save / load).

Every layer's message-passing loop is the native one (`gnn_loop_forward`, or the training tape of
`Models/training.py`); what this file adds is the label plumbing between layers and, for the joint training modes,
the chaining of gradients through `update_graph`:

    nodes_{i+1} = [ state_i (get_state) | out_i scattered on the mask (get_output, node / graph focus) | nodes_0 ]

so d loss / d nodes_{i+1} splits into an extra gradient on layer i's final state and on its per-node outputs
(reference: one eager GradientTape over all layers, `LGNN.py:252-287`).

Reference quirk kept on purpose (it defines the arithmetic): for arc-focused stacks with `get_output`, `update_graph`
concatenates the outputs *in front of the id columns* of `arcs` (`LGNN.py:210`), so the next layer's arc "labels"
`arcs[:, 2:]` are `[out[:, 2:] | src id | dst id | labels]`.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .GNN import GNNnodeBased, GNNarcBased, GNNgraphBased, _LoopModel, _metric_fn, _squeeze_last
from .training import LoopTrainer


SERIAL_PROPAGATION = ('per_graph', 'grouped')
JOINT_STEP = ('auto', 'library', 'blocks')
COMPOSITE_JOINT_STEP = ('blocks', 'auto', 'library')


def plan_runs(sizes, cap, max_nodes, max_graphs=1 << 20):
    """How the grouped serial propagation walks a sequencer's graphs (node counts `sizes`, in order): a list of ('run', i0, i1) -
    the consecutive graphs i0 .. i1 - 1 as the convergence groups of ONE library call, at most `max_nodes` nodes / `max_graphs` graphs
    per run (the workspace) - and ('single', i) - a graph of more than `cap` nodes, which takes the per-graph call between two runs.
    Every graph appears once, in order: the moving statistics are moved graph after graph whatever the cut."""
    plan, i0, nodes = [], None, 0
    for i, n in enumerate(int(v) for v in sizes):
        if n > cap:
            if i0 is not None: plan.append(('run', i0, i)); i0 = None
            plan.append(('single', i))
            continue
        if i0 is not None and (nodes + n > max_nodes or i - i0 >= max_graphs): plan.append(('run', i0, i)); i0 = None
        if i0 is None: i0, nodes = i, 0
        nodes += n
    if i0 is not None: plan.append(('run', i0, len(sizes)))
    return plan


def relabel_graphs(graphs, state, output, get_state: bool, get_output: bool, arc_focus: bool):
    """`LGNN.update_graph` for a whole list of graphs at once: `state` [sum of nodes, S] and `output` [sum of rows of
    set_mask & output_mask, T] are the per-graph results concatenated in list order; every graph's `nodes` / `arcs` / `DIM_NODE_LABEL`
    are replaced by what `update_graph(g.nodes, g.arcs, g.DIM_NODE_LABEL, g.set_mask, g.output_mask, state_g, output_g)` returns (the same
    bits, float32) - three array concatenations instead of one round of small tensor calls per graph."""
    if not graphs: return
    nodes0 = np.concatenate([np.asarray(g.nodes, dtype=np.float32) for g in graphs], axis=0)
    n_begin = np.concatenate([[0], np.cumsum([g.nodes.shape[0] for g in graphs])])
    a_begin = np.concatenate([[0], np.cumsum([g.arcs.shape[0] for g in graphs])])
    nodeplus, arcs_new = [], None
    if get_state: nodeplus.append(np.asarray(state, dtype=np.float32).reshape(nodes0.shape[0], -1))
    if get_output:
        mask = np.concatenate([np.logical_and(np.asarray(g.set_mask).reshape(-1).astype(bool), np.asarray(g.output_mask).reshape(-1).astype(bool))
                               for g in graphs])
        output = np.asarray(output, dtype=np.float32)
        out = np.zeros((len(mask), output.shape[1]), dtype=np.float32)
        out[mask] = output
        if arc_focus: arcs_new = np.concatenate([out, np.concatenate([np.asarray(g.arcs, dtype=np.float32) for g in graphs], axis=0)], axis=1)
        else: nodeplus.append(out)
    plus = sum(x.shape[1] for x in nodeplus)
    nodes_new = np.concatenate(nodeplus + [nodes0], axis=1)
    for i, g in enumerate(graphs):
        dnl = np.asarray(g.DIM_NODE_LABEL) + plus
        g.nodes = nodes_new[n_begin[i]:n_begin[i + 1]]
        g.arcs = arcs_new[a_begin[i]:a_begin[i + 1]] if arcs_new is not None else np.asarray(g.arcs, dtype=np.float32)
        g.DIM_NODE_LABEL = dnl


def split_label_gradient(d_nodes, d_arc_labels, prev, get_state: bool, get_output: bool, arc_based: bool):
    """`update_graph` backwards: the gradient w.r.t. layer i+1's labels - `d_nodes` [N, L] and, for arc focus with `get_output`,
    `d_arc_labels` [E, A] - cut into (d_state_extra [N, S], d_out_extra [M, T]) for layer i, None where nothing flows.  `prev`: layer i's
    tape or handle (`S`, `T`, `M`, `out_index`).  Pure slicing, gathering and zero-filling:
      * node / graph focus: nodes_{i+1} = [state_i | out_i scattered to `out_index` | nodes_0], so the state's gradient is the first S
        columns (with `get_state`) and the outputs' the next T, read at the rows of `out_index`;
      * arc focus: update_graph PREPENDS the T output columns to the arcs matrix (reference LGNN.py:209: `concat([arcplus, arcs])`), so
        the model's label view arcs[:, 2:] starts at output column 2: columns 0 and 1 sit where the arc ids used to be and are never
        read; output column 2 + j is arc-label column j."""
    d_state_extra = d_out_extra = None
    col = 0
    if get_state:
        d_state_extra = d_nodes[:, :prev.S].contiguous(); col = prev.S
    if get_output and not arc_based:
        d_out_extra = d_nodes[:, col:col + prev.T].index_select(0, prev.out_index.long()).contiguous()
    elif get_output:
        d_out_extra = torch.zeros((prev.M, prev.T), dtype=torch.float32, device=d_nodes.device)
        if prev.T > 2:
            d_out_extra[:, 2:] = d_arc_labels[:, :prev.T - 2].index_select(0, prev.out_index.long())
    return d_state_extra, d_out_extra


class LGNN(_LoopModel):
    """Layered GNN for node-, arc- or graph-focused problems (reference LGNN.py:11-362)."""
    _gnn_classes = {"node": GNNnodeBased, "arc": GNNarcBased, "graph": GNNgraphBased}

    def __init__(self, gnns: list, get_state: bool, get_output: bool) -> None:
        assert get_state or get_output
        assert len(set([type(i) for i in gnns])) == 1
        self.GNN_CLASS = type(gnns[0])
        self.gnns = gnns
        self.LAYERS = len(gnns)
        self.get_state = bool(get_state)
        self.get_output = bool(get_output)
        self.training_mode = None
        # how serial fit() hands a layer's results to the next one (`_propagate`): 'per_graph' = one training-mode call per graph,
        # 'grouped' = runs of consecutive graphs as convergence groups of one call (same results, same order of the moving statistics)
        self.serial_propagation = 'per_graph'
        self.serial_run_bytes = 512 << 20          # workspace a grouped run may ask for (bounds the graphs per run)
        # how a joint step ('parallel' / 'residual') runs: 'library' = every layer as two library calls (`gnn_train_step_ex` phases 1 and 2,
        # docs/joint_lgnn_step.md), 'blocks' = the building blocks driven from here, 'auto' = 'library' where it applies
        self.joint_step = 'auto'
        # ... of a stack of COMPOSITE layers: 'blocks' (the default) = as `joint_step` says, which keeps such stacks on the building blocks;
        # 'auto' / 'library' = every layer as two `gnn_train_step_composite_ex` calls where it applies / or an error
        self.composite_joint_step = 'blocks'
        self.last_joint_route = None
        self._engine_init()

    # the class <-> name maps of the reference (`__gnnClass__`, `__gnnClassLoader__`)
    @classmethod
    def _class_name(cls, klass):
        return {v: k for k, v in cls._gnn_classes.items()}[klass]

    @property
    def _focus(self):
        return self.gnns[0]._focus

    def copy(self, copy_weights: bool = True):
        config = self.get_config()
        config["gnns"] = [i.copy(copy_weights=copy_weights) for i in config["gnns"]]
        return self.from_config(config)

    def get_config(self):
        return {"gnns": self.gnns, "get_state": self.get_state, "get_output": self.get_output}

    @classmethod
    def from_config(cls, config, **kwargs):
        return cls(**config)

    def __repr__(self):
        return f"LGNN(type={self._class_name(self.GNN_CLASS)}, layers={self.LAYERS}, " \
               f"get_state={self.get_state}, get_output={self.get_output}, " \
               f"mode={self.training_mode}, avg={self.average_st_grads})"

    __str__ = __repr__

    def save(self, path: str, *args, **kwargs):
        """`<path>/GNN{i}/` per layer + `<path>/config.json` (reference LGNN.py:83-101)."""
        if path[-1] != '/': path += '/'
        config = self.get_config()
        config["gnn_class"] = self._class_name(self.GNN_CLASS)
        for i, gnn in enumerate(config.pop("gnns")): gnn.save(f'{path}GNN{i}/', **kwargs)
        with open(f'{path}config.json', 'w') as json_file: json.dump(config, json_file)

    @classmethod
    def load(cls, path: str):
        if path[-1] != '/': path += '/'
        with open(f'{path}config.json', 'r') as read_file: config = json.loads(read_file.read())
        gnn_class = cls._gnn_classes[config.pop('gnn_class')]
        dirs = sorted((d for d in os.listdir(path) if os.path.isdir(f'{path}{d}')), key=lambda d: int(d[3:]))
        return cls(gnns=[gnn_class.load(f'{path}{d}') for d in dirs], **config)

    def compile(self, *args, training_mode: str = 'parallel', average_st_grads: bool = False, serial_propagation: str = 'per_graph',
                joint_step: str = 'auto', composite_joint_step: str = 'blocks', **kwargs):
        """`training_mode` in 'serial' (layers trained one after another), 'parallel' (loss = mean of the layers' losses),
        'residual' (loss of the mean of the layers' outputs) — reference LGNN.py:133-152.  `serial_propagation` (additive; serial mode):
        'per_graph' - between two layers every graph runs alone through the trained layer, one library call each - or 'grouped' - the
        same arithmetic with the graphs as convergence groups of one call per run (docs/serial_propagation.md).  `joint_step` (additive;
        'parallel' / 'residual'): 'library' - every layer's forward and backward as one library call each, 'blocks' - the building blocks,
        'auto' - 'library' where it applies; `last_joint_route` records what a step took (docs/joint_lgnn_step.md).  `composite_joint_step`
        (additive; stacks of composite layers only): 'blocks' - everything as `joint_step` alone decides (composite stacks train through the
        building blocks, 'library' raises), 'auto' - the library route where it applies, else the building blocks, 'library' - the library
        route or NotImplementedError with the reason."""
        if training_mode not in ('serial', 'parallel', 'residual'): raise ValueError('unknown training_mode')
        if joint_step not in JOINT_STEP: raise ValueError(f'joint_step must be one of {JOINT_STEP}')
        self.joint_step = joint_step
        if composite_joint_step not in COMPOSITE_JOINT_STEP: raise ValueError(f'composite_joint_step must be one of {COMPOSITE_JOINT_STEP}')
        self.composite_joint_step = composite_joint_step
        if serial_propagation not in SERIAL_PROPAGATION: raise ValueError(f'serial_propagation must be one of {SERIAL_PROPAGATION}')
        self.serial_propagation = serial_propagation
        super().compile(*args, average_st_grads=average_st_grads, **kwargs)
        for gnn in self.gnns: gnn.compile(*args, average_st_grads=average_st_grads, **kwargs)
        self.training_mode = training_mode

    # ---- forward -----------------------------------------------------------------------------------------------------
    process_inputs = staticmethod(GNNnodeBased.process_inputs)

    def call(self, inputs, training: bool = False, mask=None):
        inputs = self.process_inputs(inputs)
        k, state, out = self.Loop(*inputs, training=training)
        if training: return k, state, out
        return out[-1]

    def update_graph(self, nodes, arcs, dim_node_label, set_mask, output_mask, state, output):
        """New (nodes, arcs, dim_node_label) with the state / output of a layer merged into the ORIGINAL labels
        (reference LGNN.py:175-214). Works on torch tensors (device) or numpy arrays (serial fit updates GraphObjects)."""
        as_np = not isinstance(nodes, torch.Tensor)
        t = (lambda x: torch.as_tensor(np.asarray(x))) if as_np else (lambda x: x)
        nodes, arcs, state, output = t(nodes).float(), t(arcs).float(), t(state).float(), t(output).float()
        set_mask, output_mask = _squeeze_last(t(set_mask)).bool(), _squeeze_last(t(output_mask)).bool()
        nodeplus, arcplus = [], []
        if self.get_state: nodeplus.append(state.to(nodes.device))
        if self.get_output:
            mask = torch.logical_and(set_mask, output_mask).to(nodes.device)
            out = torch.zeros((len(mask), output.shape[1]), dtype=torch.float32, device=nodes.device)
            out[mask] = output.to(nodes.device)
            (arcplus if self.GNN_CLASS is self._gnn_classes['arc'] else nodeplus).append(out)
        plus = sum(x.shape[1] for x in nodeplus)
        nodes = torch.cat(nodeplus + [nodes], dim=1)
        arcs = torch.cat(arcplus + [arcs], dim=1)
        dim_node_label = (np.asarray(dim_node_label) if as_np else dim_node_label) + plus
        if as_np: return nodes.numpy(), arcs.numpy(), dim_node_label
        return nodes, arcs, dim_node_label

    def _layer_inputs(self, nodes, arcs, dim_node_label, constant_inputs):
        return [nodes, arcs, dim_node_label] + list(constant_inputs)

    def Loop(self, nodes, arcs, dim_node_label, set_mask, output_mask, adjacency, arcnode, nodegraph,
             training: bool = False, *, state0=None, seed=None):
        """Lists (K, states, outs), one entry per layer (reference LGNN.py:217-249). `state0`: optional list of
        per-layer initial states."""
        constant_inputs = [set_mask, output_mask, adjacency, arcnode, nodegraph]
        nodes_0, arcs_0 = nodes, arcs
        s0 = state0 if state0 is not None else [None] * self.LAYERS
        K, states, outs = [], [], []
        graph_based = self.GNN_CLASS is self._gnn_classes['graph']
        for idx, gnn in enumerate(self.gnns[:-1]):
            k, state, out = gnn.Loop(nodes, arcs, dim_node_label, *constant_inputs, training=training, state0=s0[idx],
                                     seed=seed, node_level=True)
            K.append(k); states.append(state)
            outs.append(self._pool(nodegraph, out) if graph_based else out)
            nodes, arcs, dim_node_label = self.update_graph(nodes_0, arcs_0, dim_node_label, set_mask, output_mask, state, out)
        k, state, out = self.gnns[-1].Loop(nodes, arcs, dim_node_label, *constant_inputs, training=training,
                                           state0=s0[-1], seed=seed)
        return K + [k], states + [state], outs + [out]

    @staticmethod
    def _pool(nodegraph, out_nodes):
        """NodeGraph^T . out (per-graph mean of node outputs) on the device: `torch.ops.gnnkeras.pool`."""
        from .. import ops
        from ..sparse import SparseMatrix
        return ops.pool(SparseMatrix.from_triple(nodegraph).device_csr(out_nodes.device), out_nodes.to(torch.float32).contiguous())

    # ---- joint training (parallel / residual; docs/joint_lgnn_step.md) ---------------------------------------------------
    def _layer_x(self, x, nodes, arcs, dim_node_label):
        return [nodes, arcs, dim_node_label] + list(x[3:])

    def _joint_trainers(self):
        """One trainer per layer, kept across steps: its tape, gradient holders and the optimizer's pointer tables with it."""
        tr = getattr(self, '_joint_trs', None)
        if tr is None or len(tr) != self.LAYERS or any(t.model is not g for t, g in zip(tr, self.gnns)):
            tr = self._joint_trs = [LoopTrainer(g) for g in self.gnns]
        return tr

    def _joint_refusal(self, x, composite):
        """None when this batch can take the library route, else the reason (a joint step takes one route or the other, never a mix).
        `composite`: the question of `composite_joint_step` (a stack of composite layers) instead of `joint_step`'s; the two differ in the
        per-layer coverage query and in how the label widths grow from layer to layer."""
        from .loop_operands import type_widths
        is_composite = [isinstance(g.net_state, (list, tuple)) for g in self.gnns]
        if composite:
            if len(x) != 10 or not all(is_composite): return 'not a stack of composite layers'
        elif len(x) != 8 or any(is_composite): return 'composite layers train through the building blocks'
        if self.LAYERS > 16: return 'more than 16 layers'
        nodes, arcs = x[0], x[1]
        if not (isinstance(nodes, torch.Tensor) and nodes.is_cuda): return 'the batch is not on the device'
        arc_based = self.GNN_CLASS is self._gnn_classes['arc']
        if composite and arc_based:
            return 'arc-focused composite layers train through the building blocks (' + \
                ('get_output hands the outputs on through the arc labels, and there is no composite arc-label gradient' if self.get_output
                 else 'the phased composite step is wired for node and graph focus') + ')'
        N, E, L0, A0 = int(nodes.shape[0]), int(arcs.shape[0]), int(nodes.shape[1]), int(arcs.shape[1]) - 2
        L, A, dims = L0, A0, (type_widths(x[2]) if composite else None)
        for tr, g in zip(self._joint_trainers(), self.gnns):
            # (coverage depends on the dims and the networks, not on the rows of the mask)
            if not (tr._native_composite_phases_apply(N, E, dims, A, 1) if composite else tr._native_phases_apply(N, E, L, A, 1)):
                if composite:
                    return 'a layer is not covered by the phased in-library composite step (Dropout in front of a first Dense, a loss without a ' \
                           'device gradient, max_iteration < 1, a first state layer above 960 units, or a batch of the row-streaming size)'
                return 'a layer is not covered by the phased in-library step (Dropout in front of a first Dense, a loss without a device gradient, ' \
                       'max_iteration < 1, or a batch of the row-streaming size)'
            # what `update_graph` will add for the next layer
            S = g.state_vect_dim if g.state_vect_dim > 0 else L
            T = int(g.net_output.units[-1])
            plus = (S if self.get_state else 0) + (T if self.get_output and not arc_based else 0)
            L, A = L0 + plus, A0 + (T if self.get_output and arc_based else 0)
            if composite: dims = [min(dt + plus, L) for dt in dims]      # (it widens the widths it is handed, the labels it builds anew)
        return None

    def _joint_route(self, x):
        """The route of a joint step on the batch `x`: 'library' or 'blocks'.  A 10-element list (a stack of composite layers) that opted
        in through `composite_joint_step` is asked first; then `joint_step` decides.  A forced route that does not apply raises
        NotImplementedError with the reason."""
        if self.joint_step not in JOINT_STEP: raise ValueError(f'joint_step must be one of {JOINT_STEP}')
        if len(x) == 10 and self.composite_joint_step != 'blocks':
            why = self._joint_refusal(x, composite=True)
            if why is None: return 'library'
            if self.composite_joint_step == 'library': raise NotImplementedError(f"composite_joint_step='library' does not apply here: {why}")
        if self.joint_step == 'blocks': return 'blocks'
        why = self._joint_refusal(x, composite=False)
        if why is None: return 'library'
        if self.joint_step == 'library': raise NotImplementedError(f"joint_step='library' does not apply here: {why}")
        return 'blocks'

    def train_step(self, data, *, state0=None, seed=None, apply=True):
        """One joint optimisation step of all layers (reference LGNN.py:252-287): 'parallel' = mean of the per-layer
        losses, 'residual' = loss of the mean output. Gradients flow from layer i+1 into layer i through the labels
        built by `update_graph` (`split_label_gradient`).  One skeleton for both routes of `_joint_route`; where they differ - how a layer
        runs forward and backward, how the update is applied - the two stand side by side under `library`:
          'blocks'  - `LoopTrainer.forward` / `loss_and_grad` + `pool_backward` + `backward` on fresh trainers, a plain optimizer call;
          'library' - `forward_phase` / `backward_phase` on the cached trainers (LAYERS phase-1 calls, then LAYERS phase-2 calls, the label
                      gradients computed by the library), the update all or nothing behind one gate word (`_apply_gated`)."""
        if self.training_mode == 'serial':
            raise RuntimeError("training_mode 'serial' trains layer by layer: use fit()")
        if self.loss is None: raise RuntimeError('compile() the model with a loss before fit() / train_step()')
        x, y, sample_weight = data
        if y is None: raise TypeError('Target data is missing. Your model was compiled with `loss` '
                                      'argument and so expects targets to be passed in `fit()`.')
        x = list(x)
        composite = len(x) == 10                                   # composite lists carry type_mask at [3]
        i_set = 4 if composite else 3
        nodes_0, arcs_0, dnl, set_mask, output_mask = x[0], x[1], x[2], x[i_set], x[i_set + 1]
        s0 = state0 if state0 is not None else [None] * self.LAYERS
        for g in self.gnns: g.loss = self.loss
        self.last_joint_route = self._joint_route(x)
        library = self.last_joint_route == 'library'
        if library: trainers = self._joint_trainers()
        else:
            self.resolve_joint_pending()
            trainers = [LoopTrainer(g) for g in self.gnns]
        graph_based = self.GNN_CLASS is self._gnn_classes['graph']
        arc_based = self.GNN_CLASS is self._gnn_classes['arc']
        Lyr, residual = self.LAYERS, self.training_mode == 'residual'
        # forward sweep: layer i + 1 runs on the labels `update_graph` builds from layer i; `outs`: every layer's task-level output
        tapes, outs = [], []
        nodes, arcs = nodes_0, arcs_0
        for i, tr in enumerate(trainers):
            last = i == Lyr - 1
            lx = self._layer_x(x, nodes, arcs, dnl)
            if library:
                tp = tr.forward_phase(lx, state0=s0[i], seed=seed, composite_phases=composite)
                out = tp.y_pred
            else:
                tp = tr.forward(lx, state0=s0[i], seed=seed, node_level=not last)
                out = tp.y_pred if last else self._pool(x[-1], tp.out_nodes) if graph_based else tp.out_nodes
            tapes.append(tp); outs.append(out)
            if not last: nodes, arcs, dnl = self.update_graph(nodes_0, arcs_0, dnl, set_mask, output_mask, tp.state, tp.out_nodes)
        if library:
            # the previous applied joint step: every phase 1 above fetched its layer's word for free at its synchronisation; a layer whose tape
            # was reallocated in between fetched nothing, and the gate word itself is read then (before this step overwrites it)
            fetched = [h.prev_ok for h in tapes if h.prev_ok is not None]
            self.resolve_joint_pending(failed=(any(ok is False for ok in fetched) if len(fetched) == Lyr else None))
        # the loss and its gradient w.r.t. every layer's task-level output ('parallel' on the library route: inside `backward_phase`)
        loss, dpreds = None, [None] * Lyr
        if residual:
            loss, dmean = trainers[-1].loss_and_grad(tapes[-1], sum(outs) / Lyr, y, sample_weight)
            dpreds = [dmean / Lyr] * Lyr if library else [dmean / Lyr for _ in range(Lyr)]      # ('blocks' keeps its one division per layer)
        elif not library:
            parts = [trainers[i].loss_and_grad(tapes[i], outs[i], y, sample_weight) for i in range(Lyr)]
            loss = sum(pl[0] for pl in parts) / Lyr
            dpreds = [pl[1] / Lyr for pl in parts]
        # backward sweep, last layer first; the label gradient of layer i+1 feeds layer i
        d_state_extra, d_out_extra = None, None
        for i in range(Lyr - 1, -1, -1):
            tp, tr = tapes[i], trainers[i]
            arc_out = arc_based and self.get_output and i > 0        # the layer below wrote its output into the ARC labels
            if library:
                own = dict(y=None, sample_weight=None, d_pred_extra=dpreds[i]) if residual else \
                    dict(y=y, sample_weight=sample_weight, loss_scale=1.0 / Lyr)
                tr.backward_phase(tp, d_out_extra=d_out_extra, d_state_extra=d_state_extra, want_label_grads=i > 0,
                                  want_arc_label_grads=arc_out, **own)
                d_nodes = tp.d_nodes
            else:
                G = tr.pool_backward(tp, dpreds[i]) if graph_based else dpreds[i].clone()      # every layer's task output is pooled for graph focus
                if d_out_extra is not None: G = G + d_out_extra
                d_nodes = tr.backward(tp, G.contiguous(), d_state_extra=d_state_extra, want_label_grads=i > 0,
                                      want_arc_label_grads=arc_out)
            d_state_extra = d_out_extra = None
            if i > 0:
                # (`d_arc_labels`: there where `arc_out` asked for it; a composite layer on 'blocks' has none, and T <= 2 reads none)
                d_state_extra, d_out_extra = split_label_gradient(d_nodes, getattr(tp, 'd_arc_labels', None), tapes[i - 1],
                                                                  self.get_state, self.get_output, arc_based)
        if library and not residual: loss = sum(h.loss[0] for h in tapes) / Lyr
        for tp, tr in zip(tapes, trainers): tr.finish(tp, apply=False)
        if apply:
            gv = [pair for tp in tapes for pair in LoopTrainer.grads_and_vars(tp)]
            if library: self._apply_gated(tapes, trainers, gv)
            else: self._optimizer_obj().apply_gradients(gv)
        self._last_tapes = tapes
        logs = {'loss': loss, 'k': [tp.k for tp in tapes]}
        yd = y.to(outs[-1].device)
        sw = torch.ones(yd.shape[0], device=yd.device) if sample_weight is None else sample_weight.to(yd.device)
        for mtr in self.metrics_spec:
            n, f = _metric_fn(mtr, yd.shape[-1])
            logs[n] = (f(yd, outs[-1]) * sw).sum() / sw.sum()
        return logs

    def _apply_gated(self, hs, trainers, gv):
        """The optimizer update of a library-route step, all or nothing: one gate word over every layer's validity word (the moving
        statistics of a layer are gated by that layer's own word).  A foreign optimizer knows nothing of the gate: the words are read."""
        import ctypes as C
        from .. import _native as nat
        from .training import Adam, SGD
        opt = self._optimizer_obj()
        if not isinstance(opt, (Adam, SGD)):
            if all(LoopTrainer._read_word(h.grads_ok_view) for h in hs): opt.apply_gradients(gv)
            return
        dev = hs[0].dev
        gate = getattr(self, '_joint_gate', None)
        if gate is None or gate.device != dev: gate = self._joint_gate = torch.zeros(1, dtype=torch.int32, device=dev)
        words = (C.c_void_p * len(hs))(*[h.grads_ok for h in hs])
        nat.check(nat.lib().gnn_gate_all(words, len(hs), nat.ptr(gate), nat.current_stream(dev)))
        opt.apply_gradients(gv, gate=gate.data_ptr())
        for h, tr in zip(hs, trainers): tr._joint_word_tape = h.tape      # the next phase 1 on this tape reads the word for free
        self._joint_pending = True

    def resolve_joint_pending(self, failed=None):
        """Settle the last applied joint step of the library route: was its update gated off on the device (a barrier wait of a persistent
        backward launch expired)?  `failed` None: read the gate word (one synchronisation) - what `fit()` does behind its last step and
        `train_step` when a tape was reallocated; else what the layers' phase-1 calls fetched for free.  A discarded update had been
        counted on the host: the count is taken back, with a RuntimeWarning.  The batch is not trained again."""
        import warnings
        pending, self._joint_pending = getattr(self, '_joint_pending', False), False
        if not pending: return
        if failed is None:
            gate = getattr(self, '_joint_gate', None)
            failed = gate is not None and int(gate.item()) == 0
        if failed:
            warnings.warn('the previous joint LGNN step was discarded on the device (a persistent backward kernel could not keep its workgroups '
                          'resident): weights and optimizer slots untouched', RuntimeWarning, stacklevel=3)
            opt = self._optimizer_obj()
            if isinstance(getattr(opt, 'iterations', None), int) and opt.iterations > 0: opt.iterations -= 1

    # ---- fit: serial mode trains the layers one after another (reference LGNN.py:290-362) -----------------------------------
    def _propagate(self, gnn, seq_now, seq_t0, state0s=None):
        """What serial fit() hands from a trained layer to the next (reference LGNN.py:325-354): the states / outputs of every single
        graph of `seq_now` (batch size 1, in order, training-mode forward: BatchNormalization on that graph's own statistics, the
        moving averages moved per call) merged into copies of the t0 graphs of `seq_t0` (`update_graph`).  `state0s`: optional
        per-graph initial states for state_vect_dim > 0 (drawn otherwise).  Returns (the relabelled sequencer, per-graph k).
        `self.serial_propagation` selects the route: 'per_graph' (below) or 'grouped' (`_propagate_grouped`)."""
        if self.serial_propagation not in SERIAL_PROPAGATION: raise ValueError(f'serial_propagation must be one of {SERIAL_PROPAGATION}')
        if self.serial_propagation == 'grouped':
            done = self._propagate_grouped(gnn, seq_now, seq_t0, state0s)
            if done is not None: return done
        self.last_propagate = dict(route='per_graph', library_calls=len(seq_now.data), runs=0, fallback_graphs=len(seq_now.data))
        seq_now.shuffle = False
        seq_now.set_batch_size(1)
        s0 = state0s if state0s is not None else [None] * len(seq_now)
        results = [gnn.Loop(*gnn.process_inputs(seq_now[i][0]), training=True, state0=s0[i], node_level=True)
                   for i in range(len(seq_now))]
        new_seq = seq_t0.copy()
        for g, (_, s, o) in zip(new_seq.data, results):
            n, a, l = self.update_graph(g.nodes, g.arcs, g.DIM_NODE_LABEL, g.set_mask, g.output_mask,
                                        s.cpu().numpy(), o.cpu().numpy())
            g.nodes, g.arcs, g.DIM_NODE_LABEL = n, a, l
        return new_seq, [int(float(k)) for k, _, _ in results]

    def _grouped_applies(self, gnn, seq_now):
        """May this layer's propagation merge graphs into runs?  (a plain multi-graph sequencer whose merge leaves every graph's operators as
        they are - 'normalized' divides by the arc count of the merge - with a homogeneous layer, or the composite multi-graph sequencer
        with a composite layer; the library has the last word per run)"""
        from ..Sequencers.GraphSequencers import MultiGraphSequencer, CompositeMultiGraphSequencer
        composite = isinstance(gnn.net_state, (list, tuple))
        return type(seq_now) is (CompositeMultiGraphSequencer if composite else MultiGraphSequencer) and \
            seq_now.aggregation_mode != 'normalized' and len(seq_now.data) > 0

    def _propagate_grouped(self, gnn, seq_now, seq_t0, state0s=None):
        """`_propagate` with runs of consecutive graphs as the convergence groups of one `gnn_train_step(forward_only)` call each
        (include/gnnloop.h ABI 10): per run one batch assembly, one library call, one copy of k / state / output rows to the host; all graphs
        relabelled from the concatenated arrays at the end.  A graph above the library's group size takes the per-graph call between two runs;
        a layer the grouped kernels do not cover returns None before anything ran (the caller takes the per-graph route for that layer)."""
        from .training import LoopTrainer
        from .. import _native as nat
        if not self._grouped_applies(gnn, seq_now): return None
        graphs = list(seq_now.data)
        seq_now.shuffle = False
        focus = gnn._focus
        arc = focus == 'a'
        d = gnn.state_vect_dim
        L, A = int(graphs[0].nodes.shape[1]), int(graphs[0].arcs.shape[1]) - 2
        S = d if d > 0 else L
        SP = 16 if S <= 16 else 32 if S <= 32 else 64
        in_o = int(gnn.net_output.input_dim)
        sizes = [int(g.nodes.shape[0]) for g in graphs]
        if isinstance(gnn.net_state, (list, tuple)):
            # one state network per node type over [labels[:, :d_t] | state | Adj^T state | aggregated_component]; the statistics slots are per type
            dims = [int(v) for v in np.asarray(graphs[0].DIM_NODE_LABEL).reshape(-1)]
            w_comp = sum(dims) + A
            in_s = sum(d_t + 2 * S + w_comp for d_t in dims)
            per_node = 4 * (2 * SP + w_comp + 2) + 16
            per_graph = 4 * (max(gnn.max_iteration, 1) * 2 * in_s + 2 * in_o) + 64 + 4 * len(dims)
        else:
            in_s = 2 * S + (2 * L if d > 0 else 0) + A
            per_node = 4 * (2 * SP + L + A + 2) + 16
            per_graph = 4 * (max(gnn.max_iteration, 1) * 2 * in_s + 2 * in_o) + 64
        max_nodes = max(nat.TRAIN_GROUP_MAX_NODES, int(self.serial_run_bytes // (per_node + per_graph)))
        plan = plan_runs(sizes, nat.TRAIN_GROUP_MAX_NODES, max_nodes)
        if getattr(gnn, '_trainer', None) is None: gnn._trainer = LoopTrainer(gnn)
        rows_of = lambda g: int(np.count_nonzero(np.logical_and(np.asarray(g.set_mask).reshape(-1), np.asarray(g.output_mask).reshape(-1))))
        # (the sequencer's device-resident data set is looked up once: `_assemble_graphs` re-validates it against every graph per call)
        ds = seq_now._device_dataset()
        index = seq_now._dataset[2] if ds is not None else None
        assemble = (lambda part: ds.assemble([index[id(g_)] for g_ in part])) if ds is not None else seq_now._assemble_graphs
        states, outs, ks = [], [], []
        calls = fallback = runs = 0
        import time
        sec = dict(assemble=0.0, library_calls=0.0, d2h=0.0, copy_graphs=0.0, relabel=0.0, new_sequencer=0.0)      # host wall time (the calls are asynchronous: d2h waits for them)
        for entry in plan:
            if entry[0] == 'run':
                t0 = time.perf_counter()
                part = graphs[entry[1]:entry[2]]
                x = seq_now._x_list(assemble(part))
                node_begin = np.concatenate([[0], np.cumsum(sizes[entry[1]:entry[2]])]).astype(np.int32)
                out_begin = np.concatenate([[0], np.cumsum([rows_of(g) for g in part])]).astype(np.int32)
                s0 = None
                if d > 0 and state0s is not None:
                    s0 = torch.cat([torch.as_tensor(state0s[i]).to(x[0].device, torch.float32) for i in range(entry[1], entry[2])], dim=0)
                t1 = time.perf_counter()
                try:
                    k, state, out = gnn._trainer.forward_native(x, state0=s0, node_level=True, groups=node_begin, group_out_begin=out_begin)
                except NotImplementedError:
                    if calls: raise                  # (coverage is a property of the layer: it cannot change between two runs)
                    return None
                calls += 1; runs += 1
                t2 = time.perf_counter()
                k_h = k.cpu().numpy()                # one synchronisation per run
                if (k_h < 0).any():
                    raise nat.NativeError(f'grouped serial propagation: an arc leaves its graph (graphs {np.flatnonzero(k_h < 0)[:8] + entry[1]})')
                ks += [int(v) for v in k_h]
                if self.get_state: states.append(state.cpu().numpy())
                if self.get_output: outs.append(out.cpu().numpy())
                t3 = time.perf_counter()
                sec['assemble'] += t1 - t0; sec['library_calls'] += t2 - t1; sec['d2h'] += t3 - t2
            else:
                i = entry[1]
                x = seq_now._x_list(assemble([graphs[i]]))
                k, state, out = gnn.Loop(*gnn.process_inputs(x), training=True, state0=None if state0s is None else state0s[i], node_level=True)
                calls += 1; fallback += 1
                ks.append(int(float(k)))
                if self.get_state: states.append(state.cpu().numpy())
                if self.get_output: outs.append(out.cpu().numpy())
        # what `seq_t0.copy()` does, with the relabelling in front of the new sequencer's constructor: its batches are built once, from
        # the relabelled graphs (the per-graph route builds them from the t0 labels and leaves them stale)
        t0 = time.perf_counter()
        config = seq_t0.get_config()
        config['graphs'] = [g.copy() for g in config['graphs']]
        t1 = time.perf_counter()
        relabel_graphs(config['graphs'], np.concatenate(states, axis=0) if states else None, np.concatenate(outs, axis=0) if outs else None,
                       self.get_state, self.get_output, arc)
        t2 = time.perf_counter()
        new_seq = seq_t0.from_config(config)
        sec['copy_graphs'], sec['relabel'], sec['new_sequencer'] = t1 - t0, t2 - t1, time.perf_counter() - t2
        self.last_propagate = dict(route='grouped', library_calls=calls, runs=runs, fallback_graphs=fallback)
        self.last_propagate_seconds = sec
        return new_seq, ks

    def fit(self, sequencer, epochs: int = 1, validation_data=None, verbose: int = 1, **kwargs):
        """'parallel' / 'residual': the usual loop.  'serial' (reference LGNN.py:290-362): the layers are trained one after
        another, each on the graphs relabelled with its predecessor's states / outputs; `callbacks`, when given, is a list of
        LAYERS callback lists - entry i goes to layer i's fit (reference :299-303)."""
        if self.training_mode != 'serial':
            try: return super().fit(sequencer, epochs=epochs, validation_data=validation_data, verbose=verbose, **kwargs)
            finally: self.resolve_joint_pending()          # (the last step's gate word: nothing follows it that would fetch it)
        from ..Sequencers.GraphSequencers import SingleGraphSequencer
        if any(isinstance(s, SingleGraphSequencer) for s in (sequencer, validation_data)):
            # (the reference cannot either: it zips the layer's results with `sequencer.data`, LGNN.py:330-331, one graph object there)
            raise TypeError("serial LGNN fit() relabels a list of graphs one by one: a SingleGraphSequencer is not supported "
                            "(use a MultiGraphSequencer, or training_mode 'parallel' / 'residual')")
        callbacks = kwargs.pop('callbacks', None)
        if callbacks is None: callbacks = [[] for _ in range(self.LAYERS)]
        assert len(callbacks) == self.LAYERS
        histories = []
        # (the reference copies a sequencer wherever it hands one on, LGNN.py:303-313; a layer's fit() and the propagation below re-batch and
        # shuffle but never edit a graph, so a second sequencer over the same graph objects does - only the relabelled graphs are copies)
        view = lambda s: s._view() if hasattr(s, '_view') else s.copy()
        train_t0, valid_t0 = sequencer, validation_data
        training_sequence = view(train_t0)
        valid_sequence = view(valid_t0) if valid_t0 is not None else None
        for idx, gnn in enumerate(self.gnns[:-1]):
            if verbose: print(f'\\n\\n --- GNN {idx + 1}/{self.LAYERS} ---')
            histories.append(gnn.fit(view(training_sequence), epochs=epochs, verbose=verbose, callbacks=callbacks[idx],
                                     validation_data=view(valid_sequence) if valid_sequence is not None else None, **kwargs))
            training_sequence = self._propagate(gnn, training_sequence, train_t0)[0]
            if valid_sequence is not None: valid_sequence = self._propagate(gnn, valid_sequence, valid_t0)[0]
        if verbose: print(f'\\n\\n --- GNN {self.LAYERS}/{self.LAYERS} ---')
        histories.append(self.gnns[-1].fit(view(training_sequence), epochs=epochs, verbose=verbose, callbacks=callbacks[-1],
                                           validation_data=view(valid_sequence) if valid_sequence is not None else None, **kwargs))
        self.history = histories
        return histories
