"""GroupSort as the dynamics MLP's activation (the reference's config default, ExpConfig.py:83,
classification.py:44-48): CPU checks of the module surface, the additive C-ABI (fiode_*_act) and
the guards that keep GroupSort dynamics out of the ReLU-only training kernels."""
import ctypes as ct
import pathlib
import re

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
ACT_SYMBOLS = ("fiode_dyn_eval_act", "fiode_odeint_act", "fiode_certify_act")


def _dyn(activation, **kw):
    from fiode_amd.dynamics import OrthoClassDynProjectSimplexLips
    args = dict(n_hidden=10, activation=activation, dropout=0.5, mlp_size=128, kappa=2.0, kappa_length=0,
                alpha_1=100.0, alpha_2=20.0, sigma_1=0.02, scale_nominal=True, x_dim=10, cayley=True)
    args.update(kw)
    return OrthoClassDynProjectSimplexLips(**args)


def build_module(activation="GroupSort", seed=0):
    """bench.build_module with the dynamics' activation as a parameter (host tensors)."""
    from fiode_amd.lyapunov import LyapunovLearning, UniformInitFun, DecisionBoundary
    from fiode_amd.models import make_ortho_KWLarge_Concat
    from fiode_amd.sampling import (CompositeSampler, CompositeSamplerScheduler, CorrectConeSampling,
                                    LinearScheduler, UniformSimplexSampling)
    torch.manual_seed(seed)
    dyn = _dyn(activation)
    backbone = make_ortho_KWLarge_Concat(out_dim=10, act="GroupSort")
    sampler = CompositeSampler((10,), [UniformSimplexSampling(), CorrectConeSampling()])
    sched = CompositeSamplerScheduler([LinearScheduler(-0.02, 1.0, "min", 0.02, 10),
                                       LinearScheduler(0.02, 0.0, "max", 0.98, 10)], [1.0, 1.0])
    mod = LyapunovLearning(order=1, h_sample_size=256, h_dist_lim=15.0, sampler=sampler,
                           sampler_scheduler=sched, dynamics=dyn, init_fun=UniformInitFun((10,), backbone),
                           lya_cand=DecisionBoundary(on_simplex=True), t_max=1.0, opt_name="Adam", lr=5e-3,
                           train_ode=False, train_ode_epoch=10, train_ode_solver="dopri5", train_ode_tol=1e-3,
                           val_ode_solver="dopri5", val_ode_tol=1e-3, weight_decay=0.0, warmup=-1, max_epochs=300,
                           simplex=True, act="relu", val_adv=False, seed=seed)
    mod.current_epoch = 20
    mod.dyn_fun.scale_nominal = False
    return mod


def test_constructor_accepts_groupsort():
    from fiode_amd.cayley import GroupSort
    gs, relu = _dyn("GroupSort"), _dyn("ReLU")
    assert isinstance(gs.activation, GroupSort)
    assert list(gs.state_dict().keys()) == list(relu.state_dict().keys())
    assert gs.dyn_cfg().activation == "GroupSort" and relu.dyn_cfg().activation == "ReLU"
    with pytest.raises(NotImplementedError):
        _dyn("Tanh")


def test_dyncfg_activation_is_last_and_defaults_to_relu():
    from fiode_amd import ops
    assert ops.DynCfg().activation == "ReLU"
    assert ops.DynCfg(100.0, 20.0, 0.02, True, 0.5, 30, 1e-4).activation == "ReLU"      # positional use
    c = ops.DynCfg(activation="GroupSort").to_c()
    assert (c.n_hidden, c.mlp_size, c.x_dim, c.qp_max_iter) == (10, 128, 10, 30)         # to_c unchanged
    with pytest.raises(ValueError):
        ops._act(ops.DynCfg(activation="Tanh"))


def test_h_dot_raw_matches_float64_restatement():
    torch.manual_seed(3)
    dyn = _dyn("GroupSort", cayley=False).eval()      # plain linear layers: the Cayley maps need the device
    with torch.no_grad():
        for lin in (dyn.hidden_to_mlp, dyn.mlp_to_mlp, dyn.mlp_to_hidden, dyn.U_x):
            lin.bias.uniform_(-0.1, 0.1)
    h = torch.rand(6, 10)
    h = h / h.sum(-1, keepdim=True)
    x = torch.randn(6, 10)
    with torch.no_grad():
        out = dyn._h_dot_raw(h, x).numpy()
        w = {k: v.double().numpy() for k, v in dyn.effective_weights().items()}
    def gs(z):
        return np.concatenate([np.maximum(z[:, :64], z[:, 64:]), np.minimum(z[:, :64], z[:, 64:])], 1)
    z = gs(h.double().numpy() @ w["Q1"].T + w["b1"] + x.double().numpy() @ w["Qx"].T + w["bx"])
    z = gs(z @ w["Q2"].T + w["b2"])
    ref = z @ w["Q3"].T + w["b3"]
    assert np.abs(out - ref).max() <= 1e-5


def test_header_and_library_have_act_entry_points():
    from fiode_amd import _lib
    hdr = (ROOT / "include" / "fiode.h").read_text()
    declared = re.findall(r"FIODE_API\s+[\w\s\*]+?\b(fiode_\w+)\s*\(", hdr)
    lib = _lib.lib()
    for s in ACT_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
    assert re.search(r"FIODE_ACT_RELU = 0, FIODE_ACT_GROUPSORT = 1", hdr)
    assert (_lib.FIODE_ACT_RELU, _lib.FIODE_ACT_GROUPSORT) == (0, 1)
    assert lib.fiode_abi_version() == _lib.ABI_VERSION == 5


@pytest.mark.parametrize("activation,expect", [(0, 3), (1, 3), (2, 1), (-1, 1)])
def test_act_entry_points_check_arguments_before_workspace(activation, expect):
    """Valid configs, dummy non-NULL pointers, a zero-byte workspace: a known activation reaches the
    workspace-size check (FIODE_EWORKSPACE = 3), an unknown one is FIODE_EINVAL (1); nothing is
    launched either way."""
    from fiode_amd import _lib
    lib = _lib.lib()
    p = ct.c_void_p(1)
    dyn = _lib.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
    w = _lib.DynWeights(*[1] * 8)
    assert lib.fiode_dyn_eval_act(None, ct.byref(dyn), ct.byref(w), 4, 2, p, p, p, p, p, 0, activation) == expect
    ode = _lib.OdeConfig(_lib.FIODE_ODE_DOPRI5, 32, 2, 0, 1e-3, 1e-3, 0.0)
    assert lib.fiode_odeint_act(None, ct.byref(ode), ct.byref(dyn), ct.byref(w), p, p, p, p, p, p, p, 0,
                                activation) == expect
    cert = _lib.CertifyConfig(10, 8, 10, 3, 0.141, 0.225)
    G = lib.fiode_certify_grid_rows(10, 8)
    assert lib.fiode_certify_act(None, ct.byref(cert), ct.byref(dyn), ct.byref(w), p, p, G, p, p, p, 0,
                                 activation) == expect


def test_training_wrappers_refuse_groupsort():
    """The guards run before any tensor is looked at (host tensors here, no library call)."""
    from fiode_amd import ops, _lib as L
    gs = ops.DynCfg(activation="GroupSort")
    x, y = torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
        ops.lyap_step(x, y, {}, gs, sample_size=8, n_uniform=8)
    cfg = ops.odetrain_config(4, 0.0, 1.0, 0.1, L.FIODE_DROPOUT_OFF)
    with pytest.raises(NotImplementedError, match="training"):
        ops.odetrain_forward(x, torch.full((4, 10), 0.1), {}, gs, cfg)
    for fn, args in ((ops.odetrain_backward, (x, x, {}, gs, cfg, None)),
                     (ops.odetrain_backward_x, (x, x, {}, gs, cfg, None)),
                     (ops.odetrain_backward_weights, (x, {}, gs, cfg, None))):
        with pytest.raises(NotImplementedError):
            fn(*args)


def test_compute_loss_refuses_groupsort_on_host_tensors():
    mod = build_module("GroupSort").train()
    x, y = torch.rand(2, 3, 32, 32), torch.tensor([1, 4])
    with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
        mod.compute_loss(x, y)
    with pytest.raises(NotImplementedError, match="training"):
        mod.ode_plan(2)


def test_groupsort_reference_differs_from_relu(monkeypatch):
    """The float64 GroupSort reference runs through the oracle's eval_dot and differs from the ReLU
    oracle by far more than any tolerance of the GPU tests (a kernel still applying ReLU cannot pass)."""
    from oracle import fiode_oracle as O
    from tests._util import make_params
    from tests import _groupsort_ref as R
    P = make_params(seed=9)
    rng = np.random.default_rng(10)
    x = rng.normal(size=(50, 10)).astype(np.float32)
    h = O.uniform_simplex(rng.exponential(1, (150, 10)).astype(np.float32))
    u = np.repeat(O.static_projection(x, P), 3, 0)
    relu = O.eval_dot(h, u, P, O.DynConfig(scale_nominal=False)).f
    monkeypatch.setattr(O, "mlp_forward", R.mlp_forward)
    gs = O.eval_dot(h, u, P, O.DynConfig(scale_nominal=False)).f
    assert np.abs(gs - relu).max() > 0.1
    # the dyadic case: exact in float32, every pair of both layers at least 1/4 apart
    Pd, hd = R.dyadic_params(), R.dyadic_rows(150)
    for k in ("Q1", "Q2", "Q3"):
        assert np.array_equal(getattr(Pd, k) * 4, np.round(getattr(Pd, k) * 4))
    for k in ("b1", "b2", "b3"):
        assert np.array_equal(getattr(Pd, k) * 8, np.round(getattr(Pd, k) * 8))
    assert not Pd.Qx.any() and np.array_equal(np.abs(Pd.Q2).sum(0), np.ones(128))
    assert np.array_equal(np.abs(Pd.Q3).sum(0), np.ones(128))
    m = R.mlp_forward(hd, np.zeros((150, 128), np.float32), Pd, None, None, 0.0)
    assert R.pair_separation(m) >= 0.25
