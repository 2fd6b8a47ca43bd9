"""Training GroupSort dynamics through the fused Lyapunov step: CPU checks of the float64 reference
(tests/_groupsort_train_ref.py) against autograd, of the inputs the GPU parity cases use, of the
additive C-ABI (fiode_lyap_step_act) and of the opt-in switch (ops.GROUPSORT_TRAINING)."""
import ctypes as ct
import pathlib
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fiode_oracle as O
from tests import _groupsort_ref as R0
from tests import _groupsort_train_ref as R
from tests._util import make_params, make_step_inputs

ROOT = pathlib.Path(__file__).resolve().parents[1]
KEYS = ("Q1", "b1", "Qx", "bx", "Q2", "b2", "Q3", "b3")


def _round32(t):
    """Value rounded to float32, gradient of the identity (the reference rounds its activations)."""
    return t + (t.float().double() - t).detach()


def _torch_mlp(h, x, w, mask1, mask2, p, S):
    """The op-for-op composition of classification.py:96-102 in float64 (F.linear, mask multiply,
    cat(maximum, minimum)), rounded where the reference rounds."""
    scale = float(np.float32(1.0 / (1.0 - p)))

    def act(z, m):
        d = _round32(z * (torch.from_numpy(m.astype(np.float64)) * scale))
        return torch.cat([torch.maximum(d[:, :64], d[:, 64:]), torch.minimum(d[:, :64], d[:, 64:])], 1)
    u = _round32(F.linear(x, w["Qx"], w["bx"]))
    z1 = _round32(_round32(F.linear(h, w["Q1"], w["b1"])) + u.repeat_interleave(S, 0))
    a1 = act(z1, mask1)
    z2 = _round32(F.linear(a1, w["Q2"], w["b2"]))
    a2 = act(z2, mask2)
    return _round32(F.linear(a2, w["Q3"], w["b3"])), a1, a2


def test_reference_matches_autograd():
    B, S, p = 2, 3, 0.5
    P = make_params(seed=21)
    inp = make_step_inputs(B=B, S=S, seed=22)
    rng = np.random.default_rng(23)
    g_ft = rng.normal(size=(B * S, 10)).astype(np.float32)
    u_rows = np.repeat(O.static_projection(inp.x_feat, P), S, 0)
    m = R.mlp_forward(inp.h, u_rows, P, inp.mask1, inp.mask2, p)
    g = R.mlp_backward(g_ft, inp.h, inp.x_feat, S, P, m, inp.mask1, inp.mask2, p)
    # some pairs have one member dropped, some both (an exact tie of two zeros), some none
    k1 = inp.mask1[:, :64].astype(int) + inp.mask1[:, 64:]
    assert {0, 1, 2} <= set(np.unique(k1))

    w = {k: torch.from_numpy(getattr(P, k).astype(np.float64)).requires_grad_(True) for k in KEYS}
    x = torch.from_numpy(inp.x_feat.astype(np.float64)).requires_grad_(True)
    ft, a1, a2 = _torch_mlp(torch.from_numpy(inp.h.astype(np.float64)), x, w, inp.mask1, inp.mask2, p, S)
    for name, t in (("ftilde", ft), ("a1", a1), ("a2", a2)):
        ref = m[name].astype(np.float64)
        assert np.abs(t.detach().numpy() - ref).max() <= 1e-10 * np.abs(ref).max(), name
    (ft * torch.from_numpy(g_ft.astype(np.float64))).sum().backward()
    for k in KEYS + ("x_feat",):
        auto = (x if k == "x_feat" else w[k]).grad.numpy()
        # (the reference returns float32: compare with autograd's value rounded the same way)
        err = np.abs(g[k].astype(np.float64) - auto.astype(np.float32)).max()
        assert err <= 1e-10 * np.abs(auto).max(), (k, err)
        assert np.abs(auto).max() > 0, k


def test_reference_without_masks_is_the_eval_reference():
    P = make_params(seed=9)
    rng = np.random.default_rng(10)
    h = O.uniform_simplex(rng.exponential(1, (6, 10)).astype(np.float32))
    u = np.repeat(O.static_projection(rng.normal(size=(2, 10)).astype(np.float32), P), 3, 0)
    a, b = R.mlp_forward(h, u, P, None, None, 0.0), R0.mlp_forward(h, u, P, None, None, 0.0)
    for k in b:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("B,S,seed,scale_nominal", R.PARITY_CASES)
def test_parity_inputs_have_no_near_tie(B, S, seed, scale_nominal, monkeypatch):
    """Order-flip census of the GPU parity cases: no loss-pass pair of the reference is closer than
    2e-5 (so a float32 device orders every pair as the reference does), every row has a positive
    hinge (every row carries gradient), and the ReLU oracle's loss is far from the GroupSort one."""
    P = make_params(seed=seed)
    inp = make_step_inputs(B=B, S=S, seed=seed + 1)
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    relu = O.lyapunov_step(inp, P, cfg)
    monkeypatch.setattr(O, "mlp_forward", R.mlp_forward)
    monkeypatch.setattr(O, "mlp_backward", R.mlp_backward)
    u_rows = np.repeat(O.static_projection(inp.x_feat, P), S, 0)
    m = R.mlp_forward(inp.h, u_rows, P, inp.mask1, inp.mask2, cfg.dropout)
    sep = R.pair_separation(m, inp.mask1, inp.mask2)
    print(f"B={B} S={S} seed={seed}: smallest loss-pass separation {sep:.3e}")
    assert sep >= R.MIN_SEPARATION
    assert R.near_ties(m, inp.mask1, inp.mask2, R.MIN_SEPARATION) == 0
    out = O.lyapunov_step(inp, P, cfg)
    assert out.eff == B * S
    assert abs(out.loss - relu.loss) > 1e-3
    assert all(np.isfinite(v).all() for v in out.grads.values())


def test_existing_relu_seed_has_near_ties(monkeypatch):
    """Why (16, 64) does not reuse the ReLU test's seed 1664: two pairs under 1e-5 there."""
    P = make_params(seed=1664)
    inp = make_step_inputs(B=16, S=64, seed=1665)
    u_rows = np.repeat(O.static_projection(inp.x_feat, P), 64, 0)
    m = R.mlp_forward(inp.h, u_rows, P, inp.mask1, inp.mask2, 0.5)
    assert R.near_ties(m, inp.mask1, inp.mask2, 1e-5) == 2


# ---- C ABI ---------------------------------------------------------------------------------------

def test_header_and_library_have_lyap_step_act():
    from fiode_amd import _lib
    hdr = (ROOT / "include" / "fiode.h").read_text()
    declared = re.findall(r"FIODE_API\s+[\w\s\*]+?\b(fiode_\w+)\s*\(", hdr)
    lib = _lib.lib()
    assert "fiode_lyap_step_act" in declared and hasattr(lib, "fiode_lyap_step_act")
    assert lib.fiode_abi_version() == _lib.ABI_VERSION == 5


@pytest.mark.parametrize("activation,expect", [(0, 3), (1, 3), (2, 1), (-1, 1)])
def test_lyap_step_act_checks_arguments_before_workspace(activation, expect):
    """Valid configs, dummy non-NULL pointers, a zero-byte workspace: a known activation reaches the
    workspace-size check (FIODE_EWORKSPACE = 3), an unknown one is FIODE_EINVAL (1); nothing is
    launched either way."""
    from fiode_amd import _lib
    lib = _lib.lib()
    p = ct.c_void_p(1)
    dyn = _lib.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
    w = _lib.DynWeights(*[1] * 8)
    cfg = _lib.LyapConfig(4, 8, 8, _lib.FIODE_SAMPLER_GIVEN, _lib.FIODE_DROPOUT_GIVEN, 2.0, 0, 0)
    io = _lib.LyapIO(*([1] * 5 + [None] * 9), 0, None, None, None, None, None)
    gr = _lib.LyapGrads(*[1] * 9)
    rc = lib.fiode_lyap_step_act(None, ct.byref(cfg), ct.byref(dyn), ct.byref(w), ct.byref(io), ct.byref(gr), p, 0,
                                 activation)
    assert rc == expect
    if activation == 0:
        assert lib.fiode_lyap_step(None, ct.byref(cfg), ct.byref(dyn), ct.byref(w), ct.byref(io), ct.byref(gr),
                                   p, 0) == expect


# ---- the switch ----------------------------------------------------------------------------------

def test_switch_defaults_off_and_restores():
    from fiode_amd import ops
    assert ops.GROUPSORT_TRAINING is False
    with ops.groupsort_training():
        assert ops.GROUPSORT_TRAINING is True
        with ops.groupsort_training(False):
            assert ops.GROUPSORT_TRAINING is False
        assert ops.GROUPSORT_TRAINING is True
    assert ops.GROUPSORT_TRAINING is False
    with pytest.raises(KeyError):
        with ops.groupsort_training():
            raise KeyError("inside")
    assert ops.GROUPSORT_TRAINING is False


def test_switch_opens_the_lyapunov_step_only():
    from fiode_amd import ops, _lib as L
    gs = ops.DynCfg(activation="GroupSort")
    x, y = torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64)
    with ops.groupsort_training():
        # past the activation gate: the next check is the device check of the tensors
        with pytest.raises(ValueError, match="ROCm device"):
            ops.lyap_step(x, y, {}, gs, sample_size=8, n_uniform=8)
        cfg = ops.odetrain_config(4, 0.0, 1.0, 0.1, L.FIODE_DROPOUT_OFF)
        with pytest.raises(NotImplementedError, match="training"):
            ops.odetrain_forward(x, torch.full((4, 10), 0.1), {}, gs, cfg)
        for fn, args in ((ops.odetrain_backward, (x, x, {}, gs, cfg, None)),
                         (ops.odetrain_backward_x, (x, x, {}, gs, cfg, None)),
                         (ops.odetrain_backward_weights, (x, {}, gs, cfg, None))):
            with pytest.raises(NotImplementedError):
                fn(*args)
        with pytest.raises(NotImplementedError):      # an activation no kernel implements
            ops.lyap_step(x, y, {}, ops.DynCfg(activation="Tanh"), sample_size=8, n_uniform=8)
    with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
        ops.lyap_step(x, y, {}, gs, sample_size=8, n_uniform=8)


def test_module_gate_follows_the_train_ode_branch():
    from fiode_amd import ops
    from tests.test_groupsort_dyn import build_module
    mod = build_module("GroupSort").train()
    x, y = torch.rand(2, 3, 32, 32), torch.tensor([1, 4])
    with ops.groupsort_training():
        mod.require_trainable_dynamics("step", step=True)          # train_ode False: the step may run
        with pytest.raises(NotImplementedError, match="training"):
            mod.ode_plan(2)
        with pytest.raises(NotImplementedError, match="training"):
            mod.require_trainable_dynamics("solve")
        mod.train_ode = True                                        # current_epoch 20 > train_ode_epoch 10
        assert mod.ode_branch_active()
        with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
            mod.compute_loss(x, y)
        mod.current_epoch = 5                                       # before the branch: Lyapunov-only again
        assert not mod.ode_branch_active()
        mod.require_trainable_dynamics("step", step=True)
    with pytest.raises(NotImplementedError):
        mod.require_trainable_dynamics("step", step=True)
    relu = build_module("ReLU")
    relu.train_ode = True
    relu.require_trainable_dynamics("step", step=True)
    relu.require_trainable_dynamics("solve")
