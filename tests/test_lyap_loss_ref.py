"""CPU checks of the loss reference of the fused Lyapunov step (tests/_lyap_loss_ref.py): the closed
forms of every candidate against float64 torch autograd of the package's candidate modules, the hinges
against torch, the default config against the oracle's step bit for bit, and the input conditions that
the GPU parity cases (test_gpu_lyap_loss.py) rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fiode_oracle as O
from tests import _groupsort_train_ref as G
from tests import _lyap_loss_ref as R
from tests._util import make_params, make_step_inputs

NC = 10


def _module(name):
    from fiode_amd import lyapunov as ly
    return {"DecisionBoundary": lambda: ly.DecisionBoundary(on_simplex=True),
            "DecisionBoundaryLog": lambda: ly.DecisionBoundary(on_simplex=True, log_mode=True),
            "DynCrossEntropy": lambda: ly.DynCrossEntropy(on_simplex=True),
            "OnemEtay": lambda: ly.OnemEtay(on_simplex=True),
            "CompositeL1": lambda: ly.CompositeDynCrossEntropy(on_simplex=True, norm_type="L1"),
            "CompositeL2": lambda: ly.CompositeDynCrossEntropy(on_simplex=True, norm_type="L2")}[name]()


def _autograd(name, h, y):
    ht = torch.from_numpy(np.asarray(h, np.float64)).requires_grad_(True)
    V = _module(name)(ht, torch.from_numpy(np.asarray(y, np.int64)))
    g, = torch.autograd.grad(V.sum(), ht)
    return V.detach().numpy(), g.numpy()


def _dirichlet(n=96, seed=0):
    rng = np.random.default_rng(seed)
    h = O.uniform_simplex(rng.exponential(1.0, (n, NC)).astype(np.float32))
    return h, rng.integers(0, NC, n)


@pytest.mark.parametrize("name", R.CANDIDATES)
def test_closed_forms_equal_autograd_on_dirichlet_rows(name):
    h, y = _dirichlet()
    Va, ga = _autograd(name, h, y)
    V, g = R.cand_f64(name, h, y)
    np.testing.assert_allclose(V, Va, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g, ga, rtol=1e-12, atol=1e-14)
    # the float32-per-op form: the rounding of ~30 float32 operations on values of the arrays' scale
    V32, g32 = R.cand_f32(name, h, y)
    for a, b, what in ((V32, V, "V"), (g32, g, "grad")):
        err, mx = float(np.abs(a - b).max()), float(np.abs(b).max())
        print(f"{name} {what}: float32 form off by {err:.3e} of max {mx:.3e}")
        assert err <= 1e-6 * max(1.0, mx), (what, err, mx)


def _edge_rows():
    """h = e_y, h = e_j (j != y), h_y = 0 with the rest spread, for a few labels."""
    rows, ys = [], []
    for y in (0, 3, 9):
        e = np.zeros(NC, np.float32)
        e[y] = 1.0
        rows.append(e); ys.append(y)
        j = (y + 4) % NC
        e = np.zeros(NC, np.float32)
        e[j] = 1.0
        rows.append(e); ys.append(y)
        e = np.arange(1, NC + 1, dtype=np.float32)
        e[y] = 0.0
        rows.append((e / e.sum()).astype(np.float32)); ys.append(y)
    return np.stack(rows), np.array(ys), np.array([0, 1, 2] * 3)     # kind: 0 = e_y, 1 = e_j, 2 = h_y = 0


@pytest.mark.parametrize("name", R.CANDIDATES)
def test_closed_forms_equal_autograd_on_edge_rows(name):
    """The clamp's zero gradient is part of the check (lc' = 0 below 1e-12: h_y = 0, 1 - h_j = 0)."""
    h, y, kind = _edge_rows()
    keep = np.ones(len(y), bool)
    if name == "DecisionBoundaryLog":
        keep = kind != 0          # V_lin = 0 at h = e_y: log(0), in the reference too
    h, y, kind = h[keep], y[keep], kind[keep]
    Va, ga = _autograd(name, h, y)
    for form in (R.cand_f64, R.cand_f32):
        V, g = form(name, h, y)
        assert np.isfinite(V).all() and np.isfinite(g).all()
        tol = 1e-12 if form is R.cand_f64 else 1e-6 * max(1.0, float(np.abs(Va).max()))
        np.testing.assert_allclose(V, Va, rtol=0, atol=tol)
        gt = 1e-12 if form is R.cand_f64 else 1e-6 * max(1.0, float(np.abs(ga).max()))
        if name == "DecisionBoundary":
            # at h = e_y the nine wrong classes tie: autograd sends the +1 to one of them, the closed
            # form to the first; the label's entry and the sum over the wrong classes are compared
            r = np.arange(len(y))
            np.testing.assert_allclose(g[r, y], ga[r, y], rtol=0, atol=gt)
            np.testing.assert_allclose(g.sum(1), ga.sum(1), rtol=0, atol=gt)
            tie = kind == 0
            np.testing.assert_allclose(g[~tie], ga[~tie], rtol=0, atol=gt)
            first = np.where(y[tie] == 0, 1, 0)
            assert (g[tie][np.arange(tie.sum()), first] == 1).all()
        else:
            np.testing.assert_allclose(g, ga, rtol=0, atol=gt)
    if name in ("DynCrossEntropy", "CompositeL1", "CompositeL2"):
        g = R.cand_f64(name, h, y)[1]
        r = np.arange(len(y))
        assert (g[r, y][kind == 2] == 0).all()                       # h_y = 0: the clamp passes no gradient
    if name in ("CompositeL1", "CompositeL2"):
        j = (y + 4) % NC
        assert (g[r, j][kind == 1] == 0).all()                       # 1 - h_j = 0 likewise


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hinges_equal_torch(dtype):
    pre = np.concatenate([np.linspace(-30, 30, 241), [0.0, -0.0, 1e-8, -1e-8, -100.0]]).astype(dtype)
    ref = {"relu": torch.relu, "elu": F.elu, "identity": lambda t: t * 1.0}
    for name in R.HINGES:
        t = torch.from_numpy(pre.copy()).requires_grad_(True)
        out = ref[name](t)
        d, = torch.autograd.grad(out.sum(), t)
        viol, dv = R.hinge(name, pre)
        assert viol.dtype == dtype and dv.dtype == dtype
        tol = 4 * np.finfo(dtype).eps
        np.testing.assert_allclose(viol, out.detach().numpy(), rtol=tol, atol=0)
        np.testing.assert_allclose(dv, d.numpy(), rtol=tol, atol=0)


@pytest.mark.parametrize("B,S,sn", R.RELU_CASES)
def test_default_config_is_the_oracle_step(B, S, sn):
    P = make_params(seed=0)
    inp = make_step_inputs(B=B, S=S, seed=1)
    cfg = O.DynConfig(scale_nominal=sn)
    a, b = O.lyapunov_step(inp, P, cfg), R.lyapunov_step(inp, P, cfg, R.Loss())
    assert a.loss == b.loss and a.eff == b.eff and a.mean_active == b.mean_active
    assert (a.qp_iters, a.qp_iters_log) == (b.qp_iters, b.qp_iters_log)
    for k in ("V", "Vdot", "viol", "f", "f_log"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert set(a.grads) == set(b.grads)
    for k in a.grads:
        assert np.array_equal(a.grads[k], b.grads[k]), k


@pytest.mark.parametrize("loss", [R.Loss()] + R.RELU_LOSSES, ids=R.loss_id)
@pytest.mark.parametrize("B,S,sn", R.RELU_CASES)
def test_relu_parity_inputs_meet_the_conditions(B, S, sn, loss):
    """No row near pre = 0 or near the cap, both hinge branches present, the capped share inside
    10-90 %: what lets the GPU test compare signs, eff and the capped rows exactly."""
    P = make_params(seed=0)
    inp = make_step_inputs(B=B, S=S, seed=1, kappa=R.KAPPA)
    out = R.lyapunov_step(inp, P, O.DynConfig(scale_nominal=sn), loss)
    print(R.loss_id(loss), R.check_input_conditions(out, loss))
    for a, b in ((out.V, out.V64), (out.Vdot, out.Vdot64)):
        if np.isfinite(b).all():
            assert np.abs(a - b).max() <= 1e-6 * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("loss", R.GROUPSORT_LOSSES, ids=R.loss_id)
@pytest.mark.parametrize("B,S,seed,sn", R.GROUPSORT_CASES)
def test_groupsort_parity_inputs_meet_the_conditions(B, S, seed, sn, loss, monkeypatch):
    assert (B, S, seed, sn) in G.PARITY_CASES
    monkeypatch.setattr(O, "mlp_forward", G.mlp_forward)
    monkeypatch.setattr(O, "mlp_backward", G.mlp_backward)
    P = make_params(seed=seed)
    inp = make_step_inputs(B=B, S=S, seed=seed + 1, kappa=R.KAPPA)
    cfg = O.DynConfig(scale_nominal=sn)
    ev = O.eval_dot(inp.h, np.repeat(O.static_projection(inp.x_feat, P), S, 0), P, cfg, inp.mask1, inp.mask2)
    assert G.pair_separation(ev.mlp, inp.mask1, inp.mask2) >= G.MIN_SEPARATION
    out = R.lyapunov_step(inp, P, cfg, loss)
    print(R.loss_id(loss), R.check_input_conditions(out, loss))


def test_a_wrong_candidate_moves_the_loss():
    """The mutant bound of the GPU test, on the reference: every non-default loss is > 1e-3 from the default."""
    P = make_params(seed=0)
    for B, S, sn in R.RELU_CASES:
        inp = make_step_inputs(B=B, S=S, seed=1, kappa=R.KAPPA)
        cfg = O.DynConfig(scale_nominal=sn)
        base = R.lyapunov_step(inp, P, cfg, R.Loss()).loss
        for loss in R.RELU_LOSSES:
            assert abs(R.lyapunov_step(inp, P, cfg, loss).loss - base) > 1e-3, (B, S, R.loss_id(loss))
