"""GroupSort through the rk4 train_ode solve, the parts that need no GPU: the float64 reference
(tests/_groupsort_odetrain_ref.py) against the numpy oracle and against itself, the second opt-in
switch ``ops.GROUPSORT_TRAIN_ODE``, the ``fiode_odetrain_*_act`` C ABI, and the near-tie census of
the GPU cases (tests/test_gpu_groupsort_odetrain.py)."""
import ctypes as ct
import pathlib
import re

import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from oracle import torch_ref as T
from tests import _groupsort_odetrain_ref as G
from tests import _groupsort_train_ref as R

ROOT = pathlib.Path(__file__).resolve().parents[1]
ACT_SYMBOLS = ("fiode_odetrain_workspace_bytes_act", "fiode_odetrain_forward_act", "fiode_odetrain_backward_act",
               "fiode_odetrain_backward_x_act")


# ---- the reference against the oracle and against itself -----------------------------------------

@pytest.mark.parametrize("B,step,scale_nominal,p,seed", G.CASES)
def test_torch_reference_matches_numpy_oracle(B, step, scale_nominal, p, seed, monkeypatch):
    """The unpinned float64 torch solve = O.rk4_train with the GroupSort MLP monkeypatched in, within
    the state tolerance of tests/test_gpu_odetrain.py (2e-4: the oracle rounds to float32 per op).
    And a condition on the GPU cases: the two references agree on every stage input within
    MAX_REFERENCE_SPREAD, so the device's 2e-4 bound on them is one either reference can hold."""
    P, x, h0, labels, masks = G.make_case(B, step, p, seed)
    _, yy, _, rec = G.solve_with_grads(monkeypatch, P, x, h0, labels, masks, step, scale_nominal, p)
    monkeypatch.setattr(O, "mlp_forward", R.mlp_forward)
    ref, recs = O.rk4_train(x, h0, P, O.DynConfig(scale_nominal=scale_nominal), 0.0, 1.0, step, masks, p)
    assert len(recs) == len(rec) == G.n_evals(step)
    err = float(np.abs(yy.numpy() - ref).max())
    herr = max(float(np.abs(rec[e][4].numpy() - recs[e][0]).max()) for e in range(len(recs)))
    print(f"B={B} step={step}: |y_torch64 - y_oracle| = {err:.3e}, stage inputs {herr:.3e}")
    assert err <= 2e-4
    assert herr <= G.MAX_REFERENCE_SPREAD


@pytest.mark.parametrize("B,step,scale_nominal,p,seed", [G.CASES[0], G.CASES[4]])
def test_pinning_own_codes_changes_nothing(B, step, scale_nominal, p, seed, monkeypatch):
    P, x, h0, labels, masks = G.make_case(B, step, p, seed)
    l0, y0, g0, rec = G.solve_with_grads(monkeypatch, P, x, h0, labels, masks, step, scale_nominal, p)
    order, tie, live, _ = G.pair_codes(rec)
    if p > 0:
        assert bool(tie[~live].all()) and int((~live).sum()) > 0        # two dropped members: a tie of zeros
    l1, y1, g1, _ = G.solve_with_grads(monkeypatch, P, x, h0, labels, masks, step, scale_nominal, p,
                                       order=order, tie=tie)
    assert abs(float(l0 - l1)) <= 1e-12 and float((y0 - y1).abs().max()) <= 1e-12
    for k in g0:
        assert float((g0[k] - g1[k]).abs().max()) <= 1e-12, k


def test_tie_gives_the_half_sum_rule():
    """Autograd through maximum / minimum on an exact tie gives both members g_max / 2 + g_min / 2,
    and so does the pinned routing with the tie code."""
    d = torch.tensor([[1.5] * 64 + [1.5] * 64], dtype=torch.float64)
    d[0, 3], d[0, 67] = 2.0, -1.0                     # one ordered pair among the ties
    g = torch.arange(128, dtype=torch.float64)[None] + 1.0
    want = torch.cat([g[:, :64] / 2 + g[:, 64:] / 2] * 2, dim=1)
    want[0, 3], want[0, 67] = g[0, 3], g[0, 67]
    for pinned in (False, True):
        dd = d.clone().requires_grad_(True)
        a, b = d[:, :64], d[:, 64:]
        out = G._sort(dd, a > b, a == b) if pinned else G._sort(dd)
        out.backward(g)
        assert torch.equal(dd.grad, want), pinned


# ---- the switch ----------------------------------------------------------------------------------

def test_switch_defaults_off_and_restores():
    from fiode_amd import ops
    assert ops.GROUPSORT_TRAIN_ODE is False and ops.GROUPSORT_TRAINING is False
    with ops.groupsort_train_ode():
        assert ops.GROUPSORT_TRAIN_ODE is True and ops.GROUPSORT_TRAINING is True     # implies the first switch
        with ops.groupsort_train_ode(False):
            assert ops.GROUPSORT_TRAIN_ODE is False and ops.GROUPSORT_TRAINING is True
        assert ops.GROUPSORT_TRAIN_ODE is True
    assert ops.GROUPSORT_TRAIN_ODE is False and ops.GROUPSORT_TRAINING is False
    with pytest.raises(KeyError):
        with ops.groupsort_train_ode():
            raise KeyError("inside")
    assert ops.GROUPSORT_TRAIN_ODE is False and ops.GROUPSORT_TRAINING is False
    with ops.groupsort_training():
        with ops.groupsort_train_ode():
            pass
        assert ops.GROUPSORT_TRAINING is True and ops.GROUPSORT_TRAIN_ODE is False


def _solve_calls(ops, gs, cfg):
    x = torch.zeros(4, 10)
    return ((ops.odetrain_forward, (x, torch.full((4, 10), 0.1), {}, gs, cfg)),
            (ops.odetrain_backward, (x, x, {}, gs, cfg, None)),
            (ops.odetrain_backward_x, (x, x, {}, gs, cfg, None)),
            (ops.odetrain_backward_weights, (x, {}, gs, cfg, None)))


def test_first_switch_alone_still_refuses_the_solve():
    from fiode_amd import ops, _lib as L
    from tests.test_groupsort_dyn import build_module
    gs = ops.DynCfg(activation="GroupSort")
    cfg = ops.odetrain_config(4, 0.0, 1.0, 0.1, L.FIODE_DROPOUT_OFF)
    mod = build_module("GroupSort").train()
    mod.train_ode, mod.train_ode_solver, mod.train_ode_tol = True, "rk4", 0.25
    x, y = torch.rand(2, 3, 32, 32), torch.tensor([1, 4])
    for ctx in (ops.groupsort_training(), ops.groupsort_train_ode(False)):
        with ctx:
            for fn, args in _solve_calls(ops, gs, cfg):
                with pytest.raises(NotImplementedError, match="training"):
                    fn(*args)
            with pytest.raises(NotImplementedError, match="training"):
                mod.ode_plan(2)
            with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
                mod.compute_loss(x, y)


def test_second_switch_opens_the_rk4_solve_only():
    from fiode_amd import ops, _lib as L
    gs = ops.DynCfg(activation="GroupSort")
    rk4 = ops.odetrain_config(4, 0.0, 1.0, 0.1, L.FIODE_DROPOUT_OFF)
    dp = ops.odetrain_config(4, 0.0, 1.0, 0.0, L.FIODE_DROPOUT_OFF, method="dopri5")
    with ops.groupsort_train_ode():
        # past the activation gate: the next check is the device check of the tensors
        for fn, args in _solve_calls(ops, gs, rk4):
            with pytest.raises(ValueError, match="ROCm device"):
                fn(*args)
        for fn, args in _solve_calls(ops, gs, dp):
            with pytest.raises(NotImplementedError, match="training"):
                fn(*args)
        with pytest.raises(NotImplementedError):      # an activation no kernel implements
            ops.odetrain_forward(torch.zeros(4, 10), torch.zeros(4, 10), {}, ops.DynCfg(activation="Tanh"), rk4)
    for fn, args in _solve_calls(ops, gs, rk4):
        with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
            fn(*args)


def test_module_gate_follows_the_solver():
    from fiode_amd import ops, _lib as L
    from tests.test_groupsort_dyn import build_module
    mod = build_module("GroupSort").train()
    mod.train_ode = True                                            # current_epoch 20 > train_ode_epoch 10
    x, y = torch.rand(2, 3, 32, 32), torch.tensor([1, 4])
    with ops.groupsort_train_ode():
        assert mod.train_ode_solver == "dopri5"                     # the builder's solver: refused untouched
        with pytest.raises(NotImplementedError, match="training"):
            mod.ode_plan(2)
        with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
            mod.compute_loss(x, y)
        mod.train_ode_solver, mod.train_ode_tol = "rk4", 0.25
        mod.require_trainable_dynamics("step", step=True)
        mod.require_trainable_dynamics("solve")
        plan = mod.ode_plan(2)
        assert plan["dyn"].activation == "GroupSort" and plan["cfg"].method == L.FIODE_ODE_RK4
        assert ops.odetrain_evals(plan["cfg"]) == 16
        mod.current_epoch = 5                                       # before the branch: the Lyapunov step alone
        mod.require_trainable_dynamics("step", step=True)
    with pytest.raises(NotImplementedError):
        mod.ode_plan(2)


# ---- C ABI ---------------------------------------------------------------------------------------

def test_header_and_library_have_the_act_symbols():
    from fiode_amd import _lib
    hdr = (ROOT / "include" / "fiode.h").read_text()
    declared = re.findall(r"FIODE_API\s+[\w\s\*]+?\b(fiode_\w+)\s*\(", hdr)
    lib = _lib.lib()
    for s in ACT_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
    assert lib.fiode_abi_version() == _lib.ABI_VERSION == 5
    assert _lib.FIODE_ODETRAIN_NSAVED == 14


@pytest.mark.parametrize("B", [1, 16, 37])
def test_workspace_bytes_act(B):
    """RELU is the base size; GroupSort appends the code region, 32 bytes per (row, eval) rounded up
    to the layout's 256-byte granule; dopri5 has no GroupSort workspace."""
    from fiode_amd import ops, _lib as L
    lib = L.lib()
    for step in (0.5, 0.25, 0.1):
        cfg = ops.odetrain_config(B, 0.0, 1.0, step, L.FIODE_DROPOUT_GIVEN)
        E = ops.odetrain_evals(cfg)
        base = lib.fiode_odetrain_workspace_bytes(ct.byref(cfg))
        assert base > 0 and lib.fiode_odetrain_workspace_bytes_act(ct.byref(cfg), L.FIODE_ACT_RELU) == base
        gs = lib.fiode_odetrain_workspace_bytes_act(ct.byref(cfg), L.FIODE_ACT_GROUPSORT)
        assert gs - base == (B * E * 32 + 255) // 256 * 256
    dp = ops.odetrain_config(B, 0.0, 1.0, 0.0, L.FIODE_DROPOUT_OFF, method="dopri5")
    assert lib.fiode_odetrain_workspace_bytes_act(ct.byref(dp), L.FIODE_ACT_RELU) == \
        lib.fiode_odetrain_workspace_bytes(ct.byref(dp)) > 0
    assert lib.fiode_odetrain_workspace_bytes_act(ct.byref(dp), L.FIODE_ACT_GROUPSORT) == 0
    assert lib.fiode_odetrain_workspace_bytes_act(ct.byref(cfg), 2) == 0


def _act_calls(lib, L, cfg, ws, nbytes, activation):
    p = ct.c_void_p(1)
    dyn = L.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
    w = L.DynWeights(*[1] * 8)
    gr = L.LyapGrads(*[1] * 9)
    c, d, ww = ct.byref(cfg), ct.byref(dyn), ct.byref(w)
    return dict(
        forward=lib.fiode_odetrain_forward_act(None, c, d, ww, p, p, p, None, p, p, ws, nbytes, activation),
        backward=lib.fiode_odetrain_backward_act(None, c, d, ww, p, p, ct.byref(gr), None, ws, nbytes, activation),
        backward_x=lib.fiode_odetrain_backward_x_act(None, c, d, ww, p, p, p, None, None, None, ws, nbytes,
                                                     activation))


@pytest.mark.parametrize("activation,method,expect", [(0, "rk4", 3), (1, "rk4", 3), (0, "dopri5", 3),
                                                      (1, "dopri5", 2), (2, "rk4", 1), (-1, "dopri5", 1)])
def test_act_entry_points_check_arguments_before_workspace(activation, method, expect):
    """Valid configs and dummy non-NULL pointers.  With a zero-byte workspace a solve the library
    implements reaches the workspace-size check (FIODE_EWORKSPACE = 3); an unknown activation is
    FIODE_EINVAL (1) and GroupSort with dopri5 FIODE_ESHAPE (2), both also with a NULL workspace (the
    activation's checks come first); nothing is launched either way."""
    from fiode_amd import ops, _lib as L
    lib = L.lib()
    cfg = ops.odetrain_config(4, 0.0, 1.0, 0.25, L.FIODE_DROPOUT_GIVEN, method=method)
    for name, rc in _act_calls(lib, L, cfg, ct.c_void_p(1), 0, activation).items():
        assert rc == expect, name
    if expect != 3:
        for name, rc in _act_calls(lib, L, cfg, None, 0, activation).items():
            assert rc == expect, name
    else:
        # a NULL argument behind the workspace in the base entry point's order is still caught first
        p = ct.c_void_p(1)
        dyn = L.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
        w = L.DynWeights(*[1] * 8)
        assert lib.fiode_odetrain_forward_act(None, ct.byref(cfg), ct.byref(dyn), ct.byref(w), p, None, p, None, p, p,
                                              p, 0, activation) == 1


# ---- near-tie census of the GPU cases ------------------------------------------------------------

@pytest.mark.parametrize("B,step,scale_nominal,p,seed", G.CASES)
def test_gpu_cases_have_few_near_ties(B, step, scale_nominal, p, seed, monkeypatch):
    """A condition on the inputs of the GPU cases, not a tolerance: on the unpinned float64 reference,
    over all evals and both layers, at most 1e-3 of the live pairs (not both dropped) are closer than
    MIN_SEPARATION = 2e-5 -- the pairs a float32 device may order differently."""
    P, x, h0, labels, masks = G.make_case(B, step, p, seed)
    _, _, grads, rec = G.solve_with_grads(monkeypatch, P, x, h0, labels, masks, step, scale_nominal, p)
    _, _, live, sep = G.pair_codes(rec)
    n_live = int(live.sum())
    near = int((sep[live] < R.MIN_SEPARATION).sum())
    print(f"B={B} step={step} seed={seed}: {near} near ties of {n_live} live pairs, smallest {float(sep[live].min()):.3e}")
    assert n_live > 0 and near <= 1e-3 * n_live
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads.values())
