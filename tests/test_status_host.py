"""What KIND of failure a refused call was (`gnn_last_status`, include/gnnloop.h "Conventions") - no GPU: arguments with fake device
addresses, every call refused on host data before a launch.  The callers that fall back (gnnkeras_amd/Models/training.py, GNN.py) decide
on this status and never on the wording of `gnn_last_error`, so the table of who answers what is pinned here, next to the texts."""
import ctypes as C
import json

import pytest

from gnnkeras_amd import _native as nat
import test_loop_route_host as routes
from test_train_plan_host import make_args, malformed, lib      # noqa: F401  (lib: the fixture)


def dropout_at_0(spec):
    spec.n, spec.pos[0], spec.rate[0] = 1, 0, 0.5


def phase_forward(keep):
    px, ps = nat.TrainPhaseArgs(), nat.TrainPhaseState()
    px.phase, px.phase_state = nat.TRAIN_PHASE_FORWARD, C.pointer(ps)
    keep += [px, ps]
    return px


def not_covered_cases():
    """{name: (args, phase args or None, keep-alive, gnn_last_error text)}: well-formed calls the training entry points have no kernel form for."""
    out = {}
    def case(name, text, change=lambda ta: None, phase=False, **kw):
        ta, keep = make_args(**kw)
        change(ta)
        out[name] = (ta, phase_forward(keep) if phase else None, keep, text)
    dropout = '%s: Dropout in front of the first Dense layer (position 0): such networks train through the building blocks'
    case('Dropout at position 0, state network', dropout % 'net_state', lambda ta: dropout_at_0(ta.drop_state[0]), d=16, n=200)
    case('Dropout at position 0, output network', dropout % 'net_output', lambda ta: dropout_at_0(ta.drop_output), d=16, n=200)
    for comp in (False, True):
        case(f'no nodes, composite={comp}', 'gnn_train_step: empty graph', lambda ta: setattr(ta.loop, 'n_nodes', 0), d=16, n=200, composite=comp)
    case('composite, max_iteration 0', 'composite GNN requires max_iteration > 0', d=16, n=200, composite=True, K=0)
    case('a phase of a composite model', 'gnn_train_step_ex: phases, upstream gradients and label gradients cover whole steps of homogeneous models only '
         '(gnn_train_phases_supported)', phase=True, d=16, n=200, composite=True)
    case('a phase on the row-streaming path', 'gnn_train_step_ex: the row-streaming path (>= GNN_TRAIN_BIG_MIN_NODES nodes) has no phases / upstream '
         'gradients / label gradients: such steps train through the building blocks', phase=True, d=16, n=32768)
    return out


def test_malformed_training_calls_are_errors(lib):
    for key, (ta, keep) in malformed().items():
        assert lib.gnn_train_step(C.byref(ta)) == 1, key
        assert lib.gnn_last_status() == nat.STATUS_ERROR, (key, lib.gnn_last_error())


@pytest.mark.parametrize('name', list(not_covered_cases()))
def test_training_refusals_that_are_not_covered(lib, name):
    ta, px, keep, text = not_covered_cases()[name]
    before = bytes(ta)
    rc = lib.gnn_train_step_ex(C.byref(ta), C.byref(px)) if px is not None else lib.gnn_train_step(C.byref(ta))
    assert rc != 0
    assert lib.gnn_last_status() == nat.STATUS_NOT_COVERED and lib.gnn_last_error().decode() == text
    assert bytes(ta) == before and keep[0].value == -7          # nothing written back, k_host included
    with pytest.raises(nat.NotCovered) as raised: nat.check(rc)          # the binding: the status as the exception's type, the same message
    assert str(raised.value) == text


# every text with which loop_route.hpp refuses a forward call, and its status: the merges a caller reruns batch by batch are NOT_COVERED;
# group sets on the spread form stay an error (no caller has ever fallen back on them)
ROUTE_STATUS = {
    'convergence groups of a composite graph need the one-CU-per-group kernel (gnn_loop_groups_supported() != 2 for these args)': nat.STATUS_NOT_COVERED,
    "more than 32 convergence groups need every group to fit one CU's LDS (gnn_loop_groups_supported() != 2)": nat.STATUS_NOT_COVERED,
    'convergence groups need the whole-loop kernel (gnn_loop_groups_supported() == 0 for these args)': nat.STATUS_NOT_COVERED,
    'convergence group sets need the one-CU-per-group form (gnn_loop_groups_supported() != 2 for these args)': nat.STATUS_ERROR,
}


def test_every_refused_route_of_the_table_has_its_status(lib):
    """Every case of tests/golden/loop_routes.json whose route is "refused: ..": gnn_loop_forward fails with that text (before its first
    launch - nothing here touches a device) and with the status of the table above.  All four texts occur.  The two refusals of
    gnn_loop_forward behind its set-up launches (a one-CU-per-group launcher that declines) cannot be reached without a device."""
    with open(routes.TABLE) as fh: named = routes.decode(json.load(fh))
    seen = set()
    for s, lines in routes.sections().items():
        for key, cases in lines.items():
            for v, kw in cases:
                name = named[(s, key, str(v))]
                if not name.startswith('refused: '): continue
                text = name[len('refused: '):]
                a, keep = routes.make_args(**kw)
                assert lib.gnn_loop_forward(C.byref(a)) == 1 and lib.gnn_last_error().decode() == text, (s, key, v)
                assert lib.gnn_last_status() == ROUTE_STATUS[text], (s, key, v, text)
                seen.add(text)
    assert seen == set(ROUTE_STATUS)
    a, keep = routes.malformed()['composite, max_iteration 0']      # (the plan's twin of the training refusal)
    assert lib.gnn_loop_forward(C.byref(a)) == 1 and lib.gnn_last_status() == nat.STATUS_NOT_COVERED
    a, keep = routes.malformed()['abi_version 9']
    assert lib.gnn_loop_forward(C.byref(a)) == 1 and lib.gnn_last_status() == nat.STATUS_ERROR


def test_the_exception_classes():
    assert issubclass(nat.NotCovered, NotImplementedError) and issubclass(nat.NotCovered, nat.NativeError)
    assert issubclass(nat.NotResident, nat.NativeError) and not issubclass(nat.NotResident, NotImplementedError)
