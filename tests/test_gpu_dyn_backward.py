"""GPU parity of the differentiable eval_dot (fiode_dyn_eval_backward, ops.dyn_eval_backward and the
autograd path of OrthoClassDynProjectSimplexLips) against tests/_dyn_grad_ref.py, for ReLU and
GroupSort dynamics.

Tolerance: every gradient array within 2e-4 of the reference's max |entry| (the project's gradient
tolerance, tests/test_gpu_lyap.py:87-90: different but equally valid fp32 summation orders), with the
QP inputs pinned to the device's (DESIGN.md "Parity").  Rows on which a ReLU unit or a GroupSort
pair is within 1e-4 of its kink in the reference get a zero upstream gradient on both sides: float32
and float64 may order such a unit differently, which is a discrete difference, not an error.
"""
import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _dyn_grad_ref as G
from tests import _groupsort_ref as R
from tests._util import make_params

pytestmark = pytest.mark.gpu

TOL = 2e-4
ACTS = ["ReLU", "GroupSort"]
# seeds chosen on the CPU so that at most 15 % of the rows are within 1e-4 of a kink (none of the 5
# rows of the one-tile case), for both activations
SEEDS = {(1, 5): 25, (3, 37): 22, (50, 1): 23, (16, 64): 24}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


def _wt(P, dev):
    from fiode_amd import ops
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}


def _dyn(activation, scale_nominal):
    from fiode_amd import ops
    return ops.DynCfg(scale_nominal=scale_nominal, dropout=0.0, activation=activation)


def make_case(B, S, seed, activation, P=None, ignore_ties=False):
    """Inputs of one parity case: weights, x [B, X], simplex rows h [N, C], and an upstream gradient
    g_f that is zero on the rows within 1e-4 of a kink of the reference.  Returns the zeroed fraction
    too.  ``ignore_ties``: exact ties (weights with duplicated rows) are no kink of the comparison."""
    P = make_params(seed=seed) if P is None else P
    rng = np.random.default_rng(seed + 1)
    x = rng.normal(size=(B, 10)).astype(np.float32)
    h = O.uniform_simplex(rng.exponential(1, (B * S, 10)).astype(np.float32))
    g_f = rng.normal(size=(B * S, 10)).astype(np.float32)
    u_rows = np.repeat(O.static_projection(x, P), S, 0)
    mlp = (R.mlp_forward if activation == "GroupSort" else O.mlp_forward)(h, u_rows, P, None, None, 0.0)
    if ignore_ties:
        m = 64
        mlp = dict(mlp)
        for k in ("z1", "z2"):
            z = mlp[k].astype(np.float64).copy()
            tie = z[:, :m] == z[:, m:]
            z[:, :m][tie] += 1.0
            mlp[k] = z
    near = G.preact_margin(mlp, activation) < 1e-4
    g_f[near] = 0.0
    return P, x, h, g_f, float(near.mean())


def _run(dev, P, x, h, g_f, S, activation, scale_nominal, exit_iter=None):
    from fiode_amd import ops
    dyn = _dyn(activation, scale_nominal)
    w = _wt(P, dev)
    hd, xd, gd = (torch.from_numpy(a).to(dev) for a in (h, x, g_f))
    f, it = ops.dyn_eval(hd, xd, w, dyn, rows_per_image=S)
    g_h, grads, dbg = ops.dyn_eval_backward(gd, hd, xd, w, dyn, rows_per_image=S,
                                            exit_iter=it if exit_iter is None else exit_iter, debug=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in grads.items()}
    out["g_h"] = g_h.cpu().numpy()
    return f.cpu().numpy(), int(it.item()), out, {k: v.cpu().numpy() for k, v in dbg.items()}


def _assert_close(dev_out, ref, what=""):
    for k in G.KEYS + ("g_h",):
        a, b = dev_out[k], ref[k]
        tol = TOL * max(1e-6, float(np.abs(b).max()))
        err = float(np.abs(a - b).max())
        print(f"{what}{k}: err {err:.3e} tol {tol:.3e} max|ref| {float(np.abs(b).max()):.3e}")
        assert err <= tol, (k, err, tol)


# ---- 1. parity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(1, 5), (3, 37), (50, 1), (16, 64)])
@pytest.mark.parametrize("scale_nominal", [True, False])
@pytest.mark.parametrize("activation", ACTS)
def test_backward_matches_reference(activation, scale_nominal, B, S):
    """(1, 5): one partial tile; (3, 37): N = 111, tiles span image boundaries, plus a tail tile;
    (50, 1): the ODE function's shape; (16, 64): N = 1024, 8 workgroups."""
    dev = _dev()
    P, x, h, g_f, zeroed = make_case(B, S, SEEDS[(B, S)], activation)
    assert zeroed <= 0.15, zeroed
    f, K, out, dbg = _run(dev, P, x, h, g_f, S, activation, scale_nominal)
    # the recomputed forward is the forward's, and the QP is the reference's on the device's inputs
    assert np.array_equal(dbg["f"], f)
    v, mu = O.qp_run_fixed(dbg["qp_lower"], dbg["qp_nominal"], K)
    assert np.array_equal(dbg["f"], v) and np.array_equal(dbg["mu"], mu)
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    ref = G.eval_dot_backward(g_f, h, x, S, P, cfg, activation, qp_inputs=(dbg["qp_lower"], dbg["qp_nominal"]), K=K)
    assert float(np.abs(ref["g_h"]).max()) > 0
    tol = TOL * float(np.abs(ref["g_ft"]).max())
    assert float(np.abs(dbg["g_ftilde"] - ref["g_ft"]).max()) <= max(tol, 1e-10)
    _assert_close(out, ref)


# ---- 2. the exit iteration is honoured ------------------------------------------------------------
@pytest.mark.parametrize("activation", ACTS)
def test_exit_iteration_is_read_from_the_argument(activation):
    dev = _dev()
    P, x, h, g_f, _ = make_case(3, 37, 22, activation)
    f, K, out, dbg = _run(dev, P, x, h, g_f, 37, activation, True, exit_iter=3)
    assert K > 3
    v, mu = O.qp_run_fixed(dbg["qp_lower"], dbg["qp_nominal"], 3)
    assert np.array_equal(dbg["f"], v) and np.array_equal(dbg["mu"], mu)
    assert not np.array_equal(dbg["f"], f)


# ---- 3. GroupSort ties split the gradient ---------------------------------------------------------
@pytest.mark.parametrize("layer", [1, 2])
def test_groupsort_ties_split_in_half(layer):
    """Rows u and u + 64 of a layer's weights duplicated for eight units: the pair's pre-activations
    are bit-identical on the device and in the reference, and both members get (g_max + g_min) / 2."""
    dev = _dev()
    P = make_params(seed=31)
    units = np.array([0, 5, 17, 31, 32, 40, 55, 63])
    if layer == 1:
        for k in ("Q1", "b1", "Qx", "bx"):
            getattr(P, k)[units + 64] = getattr(P, k)[units]
    else:
        for k in ("Q2", "b2"):
            getattr(P, k)[units + 64] = getattr(P, k)[units]
    B, S = 5, 9
    P, x, h, g_f, zeroed = make_case(B, S, 32, "GroupSort", P=P, ignore_ties=True)
    assert zeroed <= 0.15, zeroed
    f, K, out, dbg = _run(dev, P, x, h, g_f, S, "GroupSort", True)
    ref = G.eval_dot_backward(g_f, h, x, S, P, O.DynConfig(scale_nominal=True), "GroupSort",
                              qp_inputs=(dbg["qp_lower"], dbg["qp_nominal"]), K=K)
    z = ref["mlp"]["z1" if layer == 1 else "z2"]
    assert np.array_equal(z[:, units], z[:, units + 64])            # the reference sees the ties
    _assert_close(out, ref)
    # both members of a tied pair receive the same gradient: equal rows of the layer's weight gradient
    key = "Q1" if layer == 1 else "Q2"
    gq = out[key]
    assert float(np.abs(gq[units]).max()) > 0
    assert np.abs(gq[units] - gq[units + 64]).max() <= TOL * float(np.abs(ref[key]).max())


# ---- 4. rows past N contribute nothing ------------------------------------------------------------
@pytest.mark.parametrize("activation", ACTS)
def test_rows_past_n_contribute_nothing(activation):
    dev = _dev()
    P, x, h, g_f, _ = make_case(1, 64, 41, activation)
    g_f[33:] = 0.0
    _, K, small, _ = _run(dev, P, x, h[:33].copy(), g_f[:33].copy(), 33, activation, True)
    _, _, big, _ = _run(dev, P, x, h, g_f, 64, activation, True, exit_iter=K)
    assert np.array_equal(big["g_h"][:33], small["g_h"])
    assert not np.any(big["g_h"][33:])
    for k in G.KEYS:
        a, b = big[k], small[k]
        assert np.allclose(a, b, rtol=1e-5, atol=1e-7 * float(np.abs(b).max())), (k, float(np.abs(a - b).max()))


# ---- 5. repeated calls ----------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ACTS)
def test_repeated_calls_are_bit_identical(activation):
    from fiode_amd import ops
    dev = _dev()
    P, x, h, g_f, _ = make_case(16, 64, 24, activation)
    dyn, w = _dyn(activation, True), _wt(P, dev)
    hd, xd, gd = (torch.from_numpy(a).to(dev) for a in (h, x, g_f))
    _, it = ops.dyn_eval(hd, xd, w, dyn, rows_per_image=64)
    runs = [ops.dyn_eval_backward(gd, hd, xd, w, dyn, rows_per_image=64, exit_iter=it, debug=True) for _ in range(3)]
    for g_h, grads, dbg in runs[1:]:
        assert torch.equal(g_h, runs[0][0])
        for k in grads:
            assert torch.equal(grads[k], runs[0][1][k]), k
        for k in dbg:
            assert torch.equal(dbg[k], runs[0][2][k]), k


# ---- 6. autograd through the module ---------------------------------------------------------------
def _module(dev, activation, scale_nominal=True):
    from fiode_amd.dynamics import OrthoClassDynProjectSimplexLips
    torch.manual_seed(5)
    return OrthoClassDynProjectSimplexLips(n_hidden=10, activation=activation, dropout=0.5, mlp_size=128, kappa=2.0,
                                           kappa_length=0, alpha_1=100.0, alpha_2=20.0, sigma_1=0.02,
                                           scale_nominal=scale_nominal, x_dim=10, cayley=True).to(dev).eval()


@pytest.mark.parametrize("activation", ACTS)
def test_autograd_through_the_module(activation):
    from fiode_amd import ops
    dev = _dev()
    dyn = _module(dev, activation)
    B, S = 6, 7
    rng = np.random.default_rng(51)
    x = torch.from_numpy(rng.normal(size=(B, 10)).astype(np.float32)).to(dev).requires_grad_(True)
    h = torch.from_numpy(O.uniform_simplex(rng.exponential(1, (B * S, 10)).astype(np.float32))).to(dev).requires_grad_(True)
    g = torch.from_numpy(rng.normal(size=(B * S, 10)).astype(np.float32)).to(dev)
    f = dyn.eval_dot(0.0, (h,), x)
    assert f.requires_grad
    gh, gx = torch.autograd.grad(f, (h, x), g, retain_graph=True)
    # the ops-level call on the detached effective weights
    w_eff = dyn.effective_weights()
    w = {k: v.detach().contiguous().float() for k, v in w_eff.items()}
    f0, it = ops.dyn_eval(h.detach(), x.detach(), w, dyn.dyn_cfg(), rows_per_image=S)
    g_h, grads = ops.dyn_eval_backward(g, h.detach(), x.detach(), w, dyn.dyn_cfg(), rows_per_image=S, exit_iter=it)
    assert torch.equal(f.detach(), f0)
    assert torch.equal(gh, g_h) and torch.equal(gx, grads["x_feat"])
    # parameters: finite, non-zero, and the effective-weight gradients pushed through the Cayley maps
    f.backward(g)
    params = dict(dyn.named_parameters())
    assert len(params) == 12
    expect = torch.autograd.grad([w_eff[k] for k in ops.WEIGHT_KEYS], list(params.values()),
                                 [grads[k] for k in ops.WEIGHT_KEYS], allow_unused=True)
    for (name, p), e in zip(params.items(), expect):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name
        assert torch.equal(p.grad, e), (name, float((p.grad - e).abs().max()))
    # no grad: the plain path, same values
    with torch.no_grad():
        f1 = dyn.eval_dot(0.0, (h,), x)
    assert not f1.requires_grad and torch.equal(f1, f0)
    assert torch.equal(dyn.eval_dot_light(h.detach(), x.detach()).detach(), f0)
    # one derivative only
    f2 = dyn.eval_dot(0.0, (h,), x)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(f2, h, g, create_graph=True)
    # training mode with dropout still refuses
    dyn.train()
    with pytest.raises(NotImplementedError):
        dyn.eval_dot(0.0, (h,), x)


# ---- 7. a differentiable solve through the public odeint ------------------------------------------
# d loss / d x of the torch-stepped RK4 solve over the autograd eval_dot against the native
# differentiable solve (fiode_odetrain_* with dropout off: 4-row train tiles, an independent
# implementation).  The two differ by float32 summation order only; the bound is the larger of 2e-4
# and 4 x the relative difference measured on an MI355X (DESIGN.md section 7c:
# 2.3e-6 on these inputs, 1.8e-5 at most over three seeds).
# scale_nominal is True here: with False the reference's active-set test in the QP backward is the
# rounding residue of nominal - mu, so two implementations whose MLP outputs
# differ in the last bit pick different active sets and their gradients differ by 0.14 to 0.35 of
# the max (measured, three seeds) while y(1) agrees to 4e-6; each of them matches the reference on
# its own pinned inputs (the parity tests above run both settings).
ODE_MEASURED = 2.3e-6
ODE_BOUND = max(2e-4, 4 * ODE_MEASURED)
assert ODE_BOUND <= 2e-3


def _solve_grad(dev, dyn, x0, h0, c):
    from fiode_amd.odeint import odeint
    x = x0.clone().requires_grad_(True)
    t = torch.tensor([0.0, 1.0], device=dev)
    y = odeint(lambda tt, hh: dyn.eval_dot(tt, (hh,), x), h0, t, method="rk4", options={"step_size": 0.25})
    (y[-1] * c).sum().backward()
    return y[-1].detach(), x.grad


def _ode_inputs(dev):
    rng = np.random.default_rng(61)
    x0 = torch.from_numpy(rng.normal(size=(8, 10)).astype(np.float32)).to(dev)
    h0 = torch.from_numpy(O.uniform_simplex(rng.exponential(1, (8, 10)).astype(np.float32))).to(dev)
    c = torch.from_numpy(rng.normal(size=(8, 10)).astype(np.float32)).to(dev)
    return x0, h0, c


def test_differentiable_solve_matches_native_train_solve():
    from fiode_amd import ops, _lib as L
    dev = _dev()
    dyn = _module(dev, "ReLU", scale_nominal=True)
    for p in dyn.parameters():
        p.requires_grad_(False)
    x0, h0, c = _ode_inputs(dev)
    y, gx = _solve_grad(dev, dyn, x0, h0, c)
    w = {k: v.detach().contiguous().float() for k, v in dyn.effective_weights().items()}
    cfg = ops.odetrain_config(8, 0.0, 1.0, 0.25, L.FIODE_DROPOUT_OFF)
    y_n, stats, ws = ops.odetrain_forward(x0, h0, w, dyn.dyn_cfg(), cfg)
    grads, _ = ops.odetrain_backward(c, x0, w, dyn.dyn_cfg(), cfg, ws)
    torch.cuda.synchronize()
    assert int(stats[3]) == 0
    b = grads["x_feat"]
    rel = float((gx - b).abs().max() / b.abs().max())
    print(f"differentiable solve vs native train solve: y diff {float((y - y_n).abs().max()):.3e}, "
          f"d loss / d x relative difference {rel:.3e} (bound {ODE_BOUND:.1e})")
    assert float(b.abs().max()) > 0
    assert rel <= ODE_BOUND, rel


def test_differentiable_solve_groupsort():
    """No native counterpart (the train solves are ReLU only): finite, non-zero, reproducible."""
    dev = _dev()
    dyn = _module(dev, "GroupSort", scale_nominal=True)
    for p in dyn.parameters():
        p.requires_grad_(False)
    x0, h0, c = _ode_inputs(dev)
    y1, g1 = _solve_grad(dev, dyn, x0, h0, c)
    y2, g2 = _solve_grad(dev, dyn, x0, h0, c)
    assert torch.isfinite(g1).all() and g1.abs().sum() > 0
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
