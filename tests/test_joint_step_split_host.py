"""Host side of the joint LGNN step's skeleton (docs/joint_lgnn_step.md) - no GPU: `split_label_gradient` against float64 autograd through
a literal restatement of `update_graph`, and the route decision `LGNN._joint_route` on a batch that is not on the device."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.MLP import MLP
from gnnkeras_amd.Models.GNN import GNNnodeBased
from gnnkeras_amd.Models.CompositeGNN import CompositeGNNnodeBased
from gnnkeras_amd.Models.CompositeLGNN import CompositeLGNN
from gnnkeras_amd.Models.LGNN import LGNN, split_label_gradient
from gnnkeras_amd.Models.training import SGD

N, E, S, L0, A = 5, 4, 3, 2, 3
OUT_ROWS = [0, 2, 3]                 # a strict subset of the rows, not the identity


def _update_graph(nodes0, arcs0, mask, state, output, get_state, get_output, arc_based):
    """`LGNN.update_graph`, restated: [state | outputs scattered on the mask | nodes_0] for node / graph focus; arc focus puts the
    scattered outputs IN FRONT of the whole arcs matrix, id columns included."""
    nodeplus, arcplus = [], []
    if get_state: nodeplus.append(state)
    if get_output:
        out = torch.zeros((len(mask), output.shape[1]), dtype=output.dtype).index_copy(0, torch.nonzero(mask).reshape(-1), output)
        (arcplus if arc_based else nodeplus).append(out)
    return torch.cat(nodeplus + [nodes0], dim=1), torch.cat(arcplus + [arcs0], dim=1)


@pytest.mark.parametrize('arc_based,get_state,get_output,T', [
    (False, True, True, 4),          # node focus, state + output
    (False, False, True, 4),         # node focus, output only: the column offset is 0
    (False, True, False, 4),         # node focus, state only
    (True, True, True, 4),           # arc focus with output: output column 2 + j is arc-label column j
    (True, False, True, 4),
    (True, True, True, 2),           # arc focus, T <= 2: nothing reaches the outputs
    (True, True, True, 1),
])
def test_split_label_gradient_is_update_graph_backwards(arc_based, get_state, get_output, T):
    g = torch.Generator().manual_seed(7)
    f32 = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)
    rows = N if not arc_based else E
    mask = torch.zeros(rows, dtype=torch.bool); mask[OUT_ROWS] = True
    M = len(OUT_ROWS)
    nodes0, arcs0 = f32(N, L0).double(), torch.cat([torch.randint(0, N, (E, 2), generator=g).double(), f32(E, A).double()], dim=1)
    state, output = f32(N, S).double().requires_grad_(), f32(M, T).double().requires_grad_()
    nodes, arcs = _update_graph(nodes0, arcs0, mask, state, output, get_state, get_output, arc_based)
    # a random linear functional of the next layer's label views: its gradients w.r.t. them are the weights themselves
    w_nodes, w_arcs = f32(*nodes.shape), f32(arcs.shape[0], arcs.shape[1] - 2)
    loss = (w_nodes.double() * nodes).sum() + (w_arcs.double() * arcs[:, 2:]).sum()
    want_state, want_out = torch.autograd.grad(loss, [state, output], allow_unused=True)

    prev = SimpleNamespace(S=S, T=T, M=M, out_index=torch.tensor(OUT_ROWS, dtype=torch.int32))
    d_state, d_out = split_label_gradient(w_nodes, w_arcs if arc_based and get_output else None, prev, get_state, get_output, arc_based)
    if get_state:
        assert d_state.dtype == torch.float32 and d_state.shape == (N, S) and d_state.is_contiguous()
        assert torch.equal(d_state, want_state.float())
    else: assert d_state is None
    if get_output:
        assert d_out.dtype == torch.float32 and d_out.shape == (M, T) and d_out.is_contiguous()
        assert torch.equal(d_out, want_out.float())
        if arc_based and T <= 2: assert not d_out.any()
        else: assert d_out.any()
    else: assert d_out is None


def _mlp(inp, units, rng):
    return MLP(inp, [units], 'tanh', 'lecun_normal', 'lecun_normal', rng=rng, batch_normalization=False)


def _host_stack(composite, **keywords):
    """A two-layer node-focused stack and a batch of the right length whose tensors live on the HOST (the route decision looks at the
    length of the list, at the layers' kind and at where `nodes` / `arcs` are - nothing else, before it answers for such a batch)."""
    if composite:
        gnns = [CompositeGNNnodeBased([_mlp(16, S, 10 * i + t) for t in range(2)], _mlp(S, 2, 10 * i + 5), S, 3, 0.01) for i in range(2)]
        lg = CompositeLGNN(gnns, True, True)
    else:
        gnns = [GNNnodeBased(_mlp(16, S, 10 * i), _mlp(S, 2, 10 * i + 5), S, 3, 0.01) for i in range(2)]
        lg = LGNN(gnns, True, True)
    lg.compile(optimizer=SGD(0.0), loss='categorical_crossentropy', training_mode='parallel', **keywords)
    rng = np.random.default_rng(0)
    nodes = torch.from_numpy(rng.normal(size=(N, L0)).astype(np.float32))
    arcs = torch.from_numpy(np.concatenate([rng.integers(0, N, (E, 2)), rng.normal(size=(E, A))], axis=1).astype(np.float32))
    ones = torch.ones(N, dtype=torch.bool)
    dnl = np.array([L0, L0]) if composite else np.array([L0])
    x = [nodes, arcs, dnl] + ([torch.ones(2, N, dtype=torch.bool)] if composite else []) + [ones, ones] + [None] * (4 if composite else 3)
    assert len(x) == (10 if composite else 8)
    return lg, x, torch.from_numpy(np.eye(2, dtype=np.float32)[rng.integers(0, 2, N)])


@pytest.fixture
def no_native_library(monkeypatch):
    def touched(): raise AssertionError('the native library was touched before the route was decided')
    monkeypatch.setattr(nat, 'lib', touched)


def test_a_forced_library_route_refuses_a_host_batch_by_name(no_native_library):
    lg, x, y = _host_stack(False, joint_step='library')
    with pytest.raises(NotImplementedError, match="joint_step='library' does not apply here: the batch is not on the device") as err:
        lg.train_step((x, y, None))
    assert 'composite_joint_step' not in str(err.value)


def test_auto_sends_a_host_batch_to_the_blocks_without_asking_the_library(no_native_library):
    lg, x, _ = _host_stack(False, joint_step='auto')
    assert lg._joint_route(x) == 'blocks'
    lg, x, _ = _host_stack(True, joint_step='auto', composite_joint_step='auto')
    assert lg._joint_route(x) == 'blocks'


def test_a_forced_composite_route_names_its_own_keyword(no_native_library):
    lg, x, y = _host_stack(True, composite_joint_step='library')
    with pytest.raises(NotImplementedError, match="composite_joint_step='library' does not apply here: the batch is not on the device"):
        lg.train_step((x, y, None))
    with pytest.raises(NotImplementedError, match="composite_joint_step='library' does not apply here"):
        lg._joint_route(x)
