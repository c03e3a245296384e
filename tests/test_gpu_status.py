"""The library's failure status (`gnn_last_status`, include/gnnloop.h "Conventions") through both bindings, end to end on the device: the
ctypes binding raises it as a class of `_native` (`NotResident` here), the custom op as `NotImplementedError` (`NOT_COVERED`).  The
refusals that need no device: tests/test_status_host.py."""
import numpy as np
import pytest
import torch

from gnnkeras_amd import _native as nat
from gnnkeras_amd.Models.GNN import GNNgraphBased
from gnnkeras_amd.Models.training import LoopTrainer
from gnnkeras_amd.Sequencers.GraphSequencers import MultiGraphSequencer

pytestmark = pytest.mark.gpu


def test_both_bindings_raise_the_status_as_a_type(mutag_graphs, monkeypatch):
    """32 MUTAG graphs in one batch, d = 32, 4 iterations (the shapes of the fall-back test in tests/test_gpu_round6.py): with every barrier
    wait of the persistent forward launch expiring at once (GNN_DEBUG_FAIL_FWD=1, one call) `forward_native` raises `NotResident`, and the
    next call runs.  State width 100 (tests/test_gpu_parity.py: no whole-loop kernel, so no convergence groups): the custom op raises
    `NotImplementedError`."""
    from test_gpu_training import nets
    from test_gpu_parity import starter_nets
    x = MultiGraphSequencer([g.copy() for g in mutag_graphs[:32]], 'g', 'average', 32, shuffle=False)[0][0]
    d = 32
    model = GNNgraphBased(*nets('g', d, True), d, 4, 0.0)
    trainer = LoopTrainer(model)
    x_list = list(model.process_inputs(x))
    s0 = torch.from_numpy(np.random.default_rng(5).normal(0, 0.1, (x[0].shape[0], d)).astype(np.float32)).cuda()
    monkeypatch.setenv('GNN_DEBUG_FAIL_FWD', '1')
    with pytest.raises(nat.NotResident, match='grid barrier'):
        trainer.forward_native(x_list, state0=s0, seed=3)
    assert nat.lib().gnn_last_status() == nat.STATUS_NOT_RESIDENT
    monkeypatch.delenv('GNN_DEBUG_FAIL_FWD')
    k, state, out = trainer.forward_native(x_list, state0=s0, seed=3)
    assert k == 4 and bool(torch.isfinite(state).all()) and tuple(out.shape) == (32, 2)
    assert nat.lib().gnn_last_kernel_name().decode() == 'train_step: persistent small-graph kernels'

    seq = MultiGraphSequencer(mutag_graphs[:64], 'g', 'average', 32, shuffle=False)
    wide = GNNgraphBased(*starter_nets('g', 100), 100, 5, 0.01)
    xm, begin = seq.merged_batches(0, 2)
    with pytest.raises(NotImplementedError, match='convergence groups need the whole-loop kernel'):
        wide.call(xm, groups=begin)
