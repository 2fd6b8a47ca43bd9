"""GPU checks of the differentiable inference solve (fiode_odeint_backward_x, ops.odeint_backward_x,
the autograd routing of fiode_amd.odeint) and of the PGD validation on the native path.

The reference of the gradients is the torch-stepped differentiable solve on the device: ``odeint``
with a user function over ``_EvalDotFn`` (the differentiable eval_dot), code that is merged and tested
on its own (tests/test_gpu_dyn_backward.py).  With scale_nominal=True every array is within 2e-4 of
its max |entry| (the project's gradient tolerance).  Rows that pass within 1e-4 of a kink (QP
active-set change, ReLU zero, GroupSort tie) in the float64 solve of tests/_ode_grad_ref.py get a
zero upstream gradient on both sides, as in test_gpu_dyn_backward.py: which side of a kink a unit
falls on is a discrete difference, not an error.  The margin is that test's: the device projection
stops at |sum v| < 1e-4, which puts the device trajectories up to 3e-5 from the float64 solve with the
exact projection and the two float32 routes up to 1e-5 from each other (measured: a row 3.3e-5 from a
GroupSort tie in float64 sat 2e-7 from it on the device, and the routes then differed by 1e-2 on that
row alone).  A row meets 16 x 256 hidden units on its way, so about a third of the ReLU rows and two
thirds of the GroupSort rows are kept; the seeds are chosen on the CPU so that at least 10 rows are.
With scale_nominal=False the reference's active-set test is rounding noise (0.14-0.35
between two valid implementations), so no parity bound is fixed there.
"""
import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _groupsort_ref as GR
from tests import _ode_grad_ref as R
from tests._util import make_params

pytestmark = pytest.mark.gpu

TOL = 2e-4
ACTS = ["ReLU", "GroupSort"]
BATCHES = [1, 33, 37]          # a partial tile, a full tile plus one row, two tiles (the second partial)
STEPS = [0.25, 0.3]            # 4 steps / 16 evaluations; 0.3: the last step is shorter
SEEDS = {1: 77, 33: 40, 37: 46}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


def _wt(P, dev):
    from fiode_amd import ops
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}


def _dyn(activation, scale_nominal=True):
    from fiode_amd import ops
    return ops.DynCfg(scale_nominal=scale_nominal, dropout=0.0, activation=activation)


def make_case(B, seed, activation, step, P=None, h0=None, t1=1.0):
    """Weights, x [B, X], simplex rows h0 [B, C] and an upstream gradient g_y that is zero on the rows
    within 1e-4 of a kink of the float64 solve.  Returns the kept fraction too."""
    P = make_params(seed=seed) if P is None else P
    rng = np.random.default_rng(seed + 1)
    x = rng.normal(size=(B, 10)).astype(np.float32)
    if h0 is None:
        h0 = O.uniform_simplex(rng.exponential(1, (B, 10)).astype(np.float32))
    g_y = rng.normal(size=(B, 10)).astype(np.float32)
    margin = R.solve(h0, x, P, O.DynConfig(scale_nominal=True), activation, 0.0, t1, step)[3]
    keep = margin >= 1e-4
    g_y[~keep] = 0.0
    return P, x, h0, g_y, float(keep.mean())


def torch_route(dev, P, x, h0, g_y, dyn, step, t1=1.0):
    """(y, g_h0, g_x) of the torch-stepped rk4 solve over the differentiable eval_dot."""
    from fiode_amd import ops
    from fiode_amd.dynamics import _EvalDotFn
    from fiode_amd.odeint import odeint
    w = _wt(P, dev)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    hd = torch.from_numpy(h0).to(dev).requires_grad_(True)
    ws = [w[k] for k in ops.WEIGHT_KEYS]
    sol = odeint(lambda t, y: _EvalDotFn.apply(dyn, 1, y, xd, *ws), hd, torch.tensor([0.0, t1], device=dev),
                 method="rk4", options=dict(step_size=step))
    (sol[-1] * torch.from_numpy(g_y).to(dev)).sum().backward()
    return sol[-1].detach(), hd.grad, xd.grad


def native(dev, P, x, h0, g_y, dyn, step, debug=False, t1=1.0):
    from fiode_amd import ops
    w = _wt(P, dev)
    xd, hd, gd = (torch.from_numpy(a).to(dev) for a in (x, h0, g_y))
    out = ops.odeint_backward_x(gd, xd, hd, w, dyn, t0=0.0, t1=t1, step_size=step, debug=debug)
    torch.cuda.synchronize()
    return out


def rel_err(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("activation", ACTS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("B", BATCHES)
def test_gradients_match_the_torch_stepped_route(B, step, activation):
    dev = _dev()
    P, x, h0, g_y, kept = make_case(B, SEEDS[B], activation, step)
    assert kept * B >= 10 or B == 1, kept
    dyn = _dyn(activation)
    _, gh_ref, gx_ref = torch_route(dev, P, x, h0, g_y, dyn, step)
    g_h0, g_x = native(dev, P, x, h0, g_y, dyn, step)
    assert g_h0.shape == (B, 10) and g_x.shape == (B, 10)
    eh, ex = rel_err(g_h0, gh_ref), rel_err(g_x, gx_ref)
    print(f"B={B} step={step} {activation}: kept {kept:.2f}, g_h0 err {eh:.2e} of max {float(gh_ref.abs().max()):.3f}, "
          f"g_x err {ex:.2e} of max {float(gx_ref.abs().max()):.3f}")
    if kept > 0:
        assert float(gh_ref.abs().max()) > 1e-3 and float(gx_ref.abs().max()) > 1e-4
        assert eh <= TOL, eh
        assert ex <= TOL, ex
    else:
        assert float(g_h0.abs().max()) == 0.0 and float(g_x.abs().max()) == 0.0


@pytest.mark.parametrize("activation", ACTS)
def test_single_row_with_gradient(activation):
    """B = 1 with a seed whose row is away from every kink (the parametrised B = 1 cases may fall on a
    masked row): one lane of one tile carries the whole gradient."""
    dev = _dev()
    for seed in range(60, 80):
        P, x, h0, g_y, kept = make_case(1, seed, activation, 0.25)
        if kept == 1.0:
            break
    assert kept == 1.0
    dyn = _dyn(activation)
    _, gh_ref, gx_ref = torch_route(dev, P, x, h0, g_y, dyn, 0.25)
    g_h0, g_x = native(dev, P, x, h0, g_y, dyn, 0.25)
    assert float(gh_ref.abs().max()) > 1e-3
    assert rel_err(g_h0, gh_ref) <= TOL and rel_err(g_x, gx_ref) <= TOL


@pytest.mark.parametrize("activation", ACTS)
@pytest.mark.parametrize("scale_nominal", [True, False])
def test_autograd_forward_is_the_no_grad_solve(activation, scale_nominal):
    """The differentiable route's y is torch.equal to the no-grad native solve's (both settings of
    scale_nominal); its gradients have the right shapes and are finite.  scale_nominal=False: no
    parity bound (module docstring), the measured distance to the torch-stepped route is printed."""
    from fiode_amd import ops
    from fiode_amd.odeint import _OdeintRk4XFn
    dev = _dev()
    B, step = 37, 0.3
    P, x, h0, g_y, _ = make_case(B, 90, activation, step)
    dyn = _dyn(activation, scale_nominal)
    w = _wt(P, dev)
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    hd = torch.from_numpy(h0).to(dev).requires_grad_(True)

    class _Mod:                     # the Function records the solve's stats on the dynamics module
        last_solve_stats = None
    plan = dict(dyn=dyn, t0=0.0, t1=1.0, step_size=step)
    y = _OdeintRk4XFn.apply(_Mod, plan, hd, xd, *[w[k] for k in ops.WEIGHT_KEYS])
    sol, stats, _ = ops.odeint_dyn(xd.detach(), hd.detach(), torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev),
                                   w, dyn, method="rk4", step_size=step)
    assert int(stats[3]) == 0 and int(stats[1]) == 4
    assert y.grad_fn is not None and torch.equal(y.detach(), sol[-1])
    gd = torch.from_numpy(g_y).to(dev)
    (y * gd).sum().backward()
    assert hd.grad.shape == (B, 10) and xd.grad.shape == (B, 10)
    assert bool(torch.isfinite(hd.grad).all()) and bool(torch.isfinite(xd.grad).all())
    _, gh_ref, gx_ref = torch_route(dev, P, x, h0, g_y, dyn, step)
    print(f"{activation} scale_nominal={scale_nominal}: g_h0 {rel_err(hd.grad, gh_ref):.2e}, g_x {rel_err(xd.grad, gx_ref):.2e}")
    # once differentiable, with eval_dot's error
    xd2 = xd.detach().clone().requires_grad_(True)
    y2 = _OdeintRk4XFn.apply(_Mod, plan, hd.detach(), xd2, *[w[k] for k in ops.WEIGHT_KEYS])
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad((y2 * gd).sum(), xd2, create_graph=True)


@pytest.mark.parametrize("activation", ACTS)
def test_replay_exit_iterations_and_stage_derivatives(activation):
    """K[n][s] of the replay lies within +-1 of a per-evaluation ops.dyn_eval at the same stage inputs
    (rebuilt here from the returned states and stage derivatives with the solve's float32
    expressions), for B = 33 (tiles that straddle steps) and B = 1 (the four steps' rows in one
    tile, one exit word per row).  Both sides see the same input bits, so equal
    K is the rule and then the stage derivatives agree to rounding (1e-6); +-1 is the allowance for a
    row whose |eps| sits at the tolerance."""
    from fiode_amd import ops
    dev = _dev()
    for B, step in ((33, 0.3), (1, 0.25)):
        P, x, h0, g_y, _ = make_case(B, 100 + B, activation, step)
        dyn = _dyn(activation)
        w = _wt(P, dev)
        _, _, dbg = native(dev, P, x, h0, g_y, dyn, step, debug=True)
        Kx, ks, states = dbg["exit_iters"].cpu().numpy(), dbg["stage_k"], dbg["states"]
        grid = ops.rk4_grid(0.0, 1.0, step).astype(np.float32)
        assert Kx.shape == (4, 4) and ks.shape == (4, 4, B, 10) and states.shape == (5, B, 10)
        xd = torch.from_numpy(x).to(dev)
        third = 1.0 / 3.0
        worst = 0
        for n in range(4):
            dt = float(grid[n + 1] - grid[n])
            y, k = states[n], ks[n]
            hin = [y, y + (dt * k[0]) * third, y + dt * (k[1] - k[0] * third), y + dt * ((k[0] - k[1]) + k[2])]
            for s in range(4):
                f, it = ops.dyn_eval(hin[s].contiguous(), xd, w, dyn)
                d = abs(int(it.item()) - int(Kx[n, s]))
                worst = max(worst, d)
                assert d <= 1, (n, s, int(it.item()), int(Kx[n, s]))
                if d == 0:
                    assert float((f - k[s]).abs().max()) <= 1e-6, (n, s)
        print(f"{activation} B={B}: exit iterations {Kx.tolist()}, largest distance {worst}")
        # and the states are the no-grad solve's: the last one is its y(t1)
        sol, _, _ = ops.odeint_dyn(xd, torch.from_numpy(h0).to(dev),
                                   torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev), w, dyn, method="rk4",
                                   step_size=step)
        assert torch.equal(states[-1], sol[-1]) and torch.equal(states[0], sol[0])


def test_dyadic_groupsort_pairs():
    """The dyadic weights of tests/_groupsort_ref.py (Q2 a signed permutation across the halves and the
    16- / 32-unit blocks, pairs at least 1/4 apart on dyadic states): a mis-routed GroupSort pair moves
    the gradient by O(1).  One step of 1/16 from dyadic rows: these dynamics expand state differences
    about 100-fold per unit of time (a 3e-6 change of h0 flips a unit within [0, 0.25], and over [0, 1]
    the two routes, 1e-5 apart in their states, measured 9e-4 of a gradient of 482), so a longer solve
    would test the conditioning of the weights, not the routing of the pairs.  One step is also the
    smallest grid the sweep takes."""
    dev = _dev()
    B, step = 33, 0.0625
    P = GR.dyadic_params()
    P, x, h0, g_y, kept = make_case(B, 120, "GroupSort", step, P=P, h0=GR.dyadic_rows(B), t1=step)
    assert kept == 1.0, kept
    dyn = _dyn("GroupSort")
    _, gh_ref, gx_ref = torch_route(dev, P, x, h0, g_y, dyn, step, t1=step)
    g_h0, g_x = native(dev, P, x, h0, g_y, dyn, step, t1=step)
    # the step's Jacobian, not the identity, carries the gradient: |g_h0 - g_y| is O(|g_y|)
    gy = torch.from_numpy(g_y).to(dev)
    assert float((gh_ref - gy).abs().max()) > 0.25 * float(gy.abs().max())
    print(f"dyadic: kept {kept:.2f}, g_h0 err {rel_err(g_h0, gh_ref):.2e} of max {float(gh_ref.abs().max()):.3f}, "
          f"|g_h0 - g_y| max {float((gh_ref - gy).abs().max()):.3f}")
    assert rel_err(g_h0, gh_ref) <= TOL
    assert float(g_x.abs().max()) == 0.0 and float(gx_ref.abs().max()) == 0.0       # Qx = 0 in these weights


# ---- routing through the module ---------------------------------------------------------------------
def _module(dev, activation, solver, tol, seed=0):
    from tests.test_groupsort_dyn import build_module
    mod = build_module(activation, seed=seed).to(dev)
    mod.dyn_fun.scale_nominal = True
    mod.val_ode_solver, mod.val_ode_tol = solver, tol
    mod.eval()
    return mod


def _images(dev, B, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, 32, 32, generator=g).to(dev)


def _rows_off_kinks(mod, static, activation):
    """Rows of the module's rk4 solve (h0 = 1/C, its own effective weights) that stay 1e-4 away from
    every kink in the float64 solve (module docstring)."""
    import types
    with torch.no_grad():
        w = {k: v.detach().double().cpu().numpy() for k, v in mod.dyn_fun.effective_weights().items()}
    d = mod.dyn_fun
    cfg = O.DynConfig(alpha_1=d.alpha_1, alpha_2=d.alpha_2, sigma_1=d.sigma_1, scale_nominal=True)
    xs = static.detach().double().cpu().numpy()
    h0 = np.full((xs.shape[0], 10), 0.1)
    return R.solve(h0, xs, types.SimpleNamespace(**w), cfg, activation, 0.0, 1.0, 0.25)[3] >= 1e-4


@pytest.mark.parametrize("activation", ACTS)
def test_module_forward_routes_rk4_to_the_native_backward(activation):
    """B = 8 images; the upstream gradient is zero on the rows near a kink, and the image seed is the
    first of ten that keeps at least three rows."""
    from fiode_amd.lyapunov import no_param_grad
    from fiode_amd.odeint import odeint
    dev = _dev()
    B = 8
    mod = _module(dev, activation, "rk4", 0.25)
    for seed in range(5, 15):
        x = _images(dev, B, seed)
        with torch.no_grad():
            keep = _rows_off_kinks(mod, mod.init_coordinates(x, mod.dyn_fun)[0], activation)
        if keep.sum() >= 3:
            break
    assert keep.sum() >= 3, keep
    gout = torch.randn(B, 10, generator=torch.Generator().manual_seed(6))
    gout[torch.from_numpy(~keep)] = 0.0
    gout = gout.to(dev)
    # as today: parameters require grad, the solve runs without grad
    xa = x.clone().requires_grad_(True)
    out = mod(xa)
    assert out.grad_fn is None and not out.requires_grad
    with torch.no_grad():
        clean = mod(x)
    with no_param_grad(mod):
        xb = x.clone().requires_grad_(True)
        out = mod(xb)
        assert out.grad_fn is not None and torch.equal(out.detach(), clean)
        gx, = torch.autograd.grad((out * gout).sum(), xb)
        # the torch-stepped route from the same backbone features
        xc = x.clone().requires_grad_(True)
        static, (h0,) = mod.init_coordinates(xc, mod.dyn_fun)
        sol = odeint(lambda t, y: mod.dyn_fun._eval(y, static), h0.contiguous(), torch.tensor([0.0, 1.0], device=dev),
                     method="rk4", options=dict(step_size=0.25))
        gref, = torch.autograd.grad((sol[-1] * gout).sum(), xc)
    assert all(p.requires_grad for p in mod.parameters())
    assert gx.shape == x.shape and bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    print(f"{activation}: kept {int(keep.sum())} of {B}, image gradient max {float(gref.abs().max()):.3e}, "
          f"err {rel_err(gx, gref):.2e}")
    assert rel_err(gx, gref) <= TOL


@pytest.mark.parametrize("activation", ACTS)
def test_module_forward_dopri5_routes_give_an_image_gradient(activation):
    """dopri5: ReLU through the train_ode solve with dropout off and its backward_x, GroupSort through
    the torch stepper over the differentiable eval_dot; B = 4."""
    from fiode_amd.lyapunov import no_param_grad
    dev = _dev()
    mod = _module(dev, activation, "dopri5", 1e-3)
    x = _images(dev, 4)
    with torch.no_grad():
        clean = mod(x)
    with no_param_grad(mod):
        xb = x.clone().requires_grad_(True)
        out = mod(xb)
        assert out.grad_fn is not None
        gx, = torch.autograd.grad(torch.nn.functional.cross_entropy(out, clean.argmax(-1)), xb)
    assert float((out.detach() - clean).abs().max()) <= 1e-3        # the solver's own tolerance
    assert gx.shape == x.shape and bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0


def test_validation_step_attacks_on_the_native_path():
    dev = _dev()
    mod = _module(dev, "GroupSort", "rk4", 0.25)
    mod.val_adv, mod.norm, mod.eps = True, "L2", 36 / 255
    mod.val_adv_generator = torch.Generator(device=dev).manual_seed(7)
    x = _images(dev, 8)
    with torch.no_grad():
        y = mod(x).argmax(-1)
    seen = {}
    attack = mod.validation_attack
    def record(xx, yy):
        seen["adv"] = attack(xx, yy)
        return seen["adv"]
    mod.validation_attack = record
    mod.validation_step((x, y))
    adv = seen["adv"]
    norms = (adv - x).flatten(1).norm(dim=1)
    assert float(norms.min()) > 0 and float(norms.max()) <= mod.eps * (1 + 1e-5)
    assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
    err, err_adv = float(mod.logged["validation_error"]), float(mod.logged["validation_adv_error"])
    print(f"validation_error {err}, validation_adv_error {err_adv}, |delta| {float(norms.min()):.4f}..{float(norms.max()):.4f}")
    assert err == 0.0 and err_adv >= err
    assert all(p.requires_grad for p in mod.parameters()) and not mod.training
