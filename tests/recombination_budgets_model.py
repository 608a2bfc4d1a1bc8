"""Recombination margins for every listed budget from one joint pass -- numpy, TEST INFRASTRUCTURE, on top of
recombination_margins_model.recombination_margins_np and phase_margins_model.joint_states_fb.

Written from the definition in include/dipgenie_hip.h (dg_dp_recombination_margins_budgets), not from any implementation of it.  Both
states mean "at most r", so plane p of F_l and of B_{l+1} computed at bmax = max(budgets) is plane p at any b <= bmax: the states are
computed ONCE at bmax, query q reads the planes 0 .. budgets[q] of them, and V_b is plane b of the sink's cell of the last level.
tests/test_recombination_budgets_model.py pins every such slice to the one-budget model at that budget."""
import numpy as np

from phase_margins_model import joint_states_fb
from recombination_margins_model import recombination_margins_np


def sliced_states(states, b):
    """the states of joint_states_fb(m, bmax) as those of budget b <= bmax: planes 0 .. b, V from the sink's cell"""
    F, B, _, edges = states
    return [f[:, :, :b + 1] for f in F], [x[:, :, :b + 1] for x in B], int(F[-1][-1, -1, b]), edges


def recombination_margins_budgets_np(m, budgets, called=None, states=None):
    """-> (records int32 [n, L - 1, 16], called_out int32 [n, L - 1, 2] or None, V int64 [n]).  budgets: n integers >= 0;
    called: int [n, 2, L] or None; states: joint_states_fb(m, bmax) with bmax >= max(budgets), computed here if absent"""
    budgets = [int(b) for b in budgets]
    if states is None:
        states = joint_states_fb(m, max(budgets))
    rec, out, V = [], [], []
    for q, b in enumerate(budgets):
        r, o, v = recombination_margins_np(m, b, None if called is None else np.asarray(called)[q:q + 1], sliced_states(states, b))
        rec.append(r)
        out.append(None if o is None else o[0])
        V.append(v)
    return np.stack(rec), (None if called is None else np.stack(out)), np.array(V, np.int64)
