"""GPU checks of the native input gradients of the dopri5 inference solve: the step log of
fiode_odeint_act_log, fiode_odeint_dopri5_backward_x (ops.odeint_dopri5_backward_x), the autograd routing
of fiode_amd.odeint and the PGD validation of a GroupSort module with its own validation solver.

The reference of the gradients is a frozen-step torch replay on the device: given the device's log it
runs the dopri5 steps and the dense output at t1 in torch over ``_EvalDotFn`` (the differentiable
eval_dot, merged and tested on its own; the tableau constants of fiode_amd.odeint) and calls
``.backward()`` -- what the torch stepper differentiates, whose step sizes are Python floats.  The
tolerance and the masking are those of test_gpu_ode_backward_x.py: every array within TOL = 2e-4 of its
max |entry|, and rows within 1e-4 of a kink (QP active-set change, ReLU zero, GroupSort tie) of the
float64 ``solve_on_log`` on the DEVICE's log get a zero upstream gradient on both sides.  The kept-row
counts of the cases were chosen with the float64 controller (tests/_dopri5_grad_ref.controller_solve)
and are asserted again on the device's log.

Largest distances measured on an MI355X over the cases below: g_h0 6.8e-5, g_x 2.4e-5 of the array's
max, next to TOL = 2e-4 (the table is in DESIGN.md 7d.2).
"""
import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _dopri5_grad_ref as D
from tests._util import make_params

pytestmark = pytest.mark.gpu

TOL = 2e-4
CAP = 64
# (activation, B, seed, t1, tol): accepted steps and kept rows of the float64 controller
CASES = {
    ("GroupSort", 33, 40, 1.0, 1e-3): (7, 11),
    ("GroupSort", 37, 46, 1.0, 1e-3): (6, 14),
    ("GroupSort", 97, 46, 1.0, 1e-5): (12, 35),
    ("GroupSort", 1, 65, 1.0, 1e-3): (6, 1),
    ("ReLU", 97, 47, 0.25, 1e-4): (3, 32),
    ("ReLU", 97, 46, 0.5, 1e-3): (4, 12),
    ("ReLU", 1, 64, 1.0, 1e-3): (6, 1),
}
_CACHE = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


def _wt(P, dev):
    from fiode_amd import ops
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}


def _dyn(activation):
    from fiode_amd import ops
    return ops.DynCfg(scale_nominal=True, dropout=0.0, activation=activation)


def make_inputs(B, seed):
    """Weights, x [B, X], simplex rows h0 [B, C] and an upstream gradient, as make_case of
    test_gpu_ode_backward_x.py draws them."""
    P = make_params(seed=seed)
    rng = np.random.default_rng(seed + 1)
    x = rng.normal(size=(B, 10)).astype(np.float32)
    h0 = O.uniform_simplex(rng.exponential(1, (B, 10)).astype(np.float32))
    g_y = rng.normal(size=(B, 10)).astype(np.float32)
    return P, x, h0, g_y


def solve_case(dev, activation, B, seed, t1, tol):
    """The logged solve of a case on the device, its float64 solve on that log and the masked upstream
    gradient; computed once per case and shared (nothing in it is modified afterwards)."""
    from fiode_amd import ops
    key = (activation, B, seed, t1, tol)
    if key in _CACHE:
        return _CACHE[key]
    P, x, h0, g_y = make_inputs(B, seed)
    w, dyn = _wt(P, dev), _dyn(activation)
    xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(h0).to(dev)
    tt = torch.tensor([0.0, t1], dtype=torch.float64, device=dev)
    sol, stats, dstats, times, states = ops.odeint_dyn(xd, hd, tt, w, dyn, method="dopri5", rtol=tol, atol=tol,
                                                       log_steps=CAP)
    st = stats.cpu().numpy()
    assert st[3] == 0 and 1 <= st[1] <= CAP, st
    n = int(st[1])
    tn = times.cpu().numpy()
    y64, _, _, margin = D.solve_on_log(h0, x, P, O.DynConfig(scale_nominal=True), activation, tn[:n, 0], tn[:n, 1], t1)
    keep = margin >= 1e-4
    g_y = g_y.copy()
    g_y[~keep] = 0.0
    c = dict(P=P, x=x, h0=h0, g_y=g_y, w=w, dyn=dyn, xd=xd, hd=hd, tt=tt, sol=sol, stats=st, dstats=dstats,
             times=times, states=states, tn=tn, n=n, y64=y64, keep=keep, t1=t1, tol=tol, activation=activation)
    _CACHE[key] = c
    return c


def frozen_replay(dev, c, need_grad=True):
    """(y(t1), g_h0, g_x) of the torch replay of the logged steps over the differentiable eval_dot."""
    from fiode_amd import ops
    from fiode_amd.dynamics import _EvalDotFn
    from fiode_amd.odeint import _BETA, _CMID
    xd = c["xd"].clone().requires_grad_(need_grad)
    hd = c["hd"].clone().requires_grad_(need_grad)
    ws = [c["w"][k] for k in ops.WEIGHT_KEYS]
    F = lambda yy: _EvalDotFn.apply(c["dyn"], 1, yy, xd, *ws)
    y = hd
    n = c["n"]
    for i in range(n):
        tn, dtn = float(c["tn"][i, 0]), float(c["tn"][i, 1])
        dt = float(np.float32(dtn))
        k = [F(y)]
        for s in range(6):
            k.append(F(y + sum(k[j] * (_BETA[s][j] * dt) for j in range(s + 1))) if s < 5 or i == n - 1 else None)
        ynew = y + sum(k[j] * (_BETA[5][j] * dt) for j in range(6))
        if i == n - 1:
            ym = y + sum(k[j] * (_CMID[j] * dt) for j in range(7))
            fa, fb = k[0], k[6]
            interp = [y, dt * fa, dt * (fb - 4 * fa) - 11 * y - 5 * ynew + 16 * ym,
                      dt * (5 * fa - 3 * fb) + 18 * y + 14 * ynew - 32 * ym, 2 * dt * (fb - fa) - 8 * (ynew + y) + 16 * ym]
            x = float(np.float32((c["t1"] - tn) / ((tn + dtn) - tn)))
            out, xp = interp[0] + x * interp[1], x
            for cf in interp[2:]:
                xp = xp * x
                out = out + xp * cf
        y = ynew
    if not need_grad:
        return out.detach(), None, None
    (out * torch.from_numpy(c["g_y"]).to(dev)).sum().backward()
    return out.detach(), hd.grad, xd.grad


def native(dev, c, debug=False):
    from fiode_amd import ops
    out = ops.odeint_dopri5_backward_x(torch.from_numpy(c["g_y"]).to(dev), c["xd"], c["w"], c["dyn"], t1=c["t1"],
                                       step_times=c["times"], step_states=c["states"], n_steps=c["n"], debug=debug)
    torch.cuda.synchronize()
    return out


def rel_err(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# ---- 1. the log -------------------------------------------------------------------------------------
def _check_log(dev, c):
    from fiode_amd import ops
    sol0, stats0, dstats0 = ops.odeint_dyn(c["xd"], c["hd"], c["tt"], c["w"], c["dyn"], method="dopri5", rtol=c["tol"],
                                           atol=c["tol"])
    assert torch.equal(sol0, c["sol"]) and torch.equal(stats0.cpu(), torch.from_numpy(c["stats"]))
    assert torch.equal(dstats0, c["dstats"])
    n, tn, t1 = c["n"], c["tn"], c["t1"]
    assert n == c["stats"][1]
    assert tn[0, 0] == 0.0 and np.all(tn[:n, 1] > 0)
    assert np.all(tn[1:n, 0] == tn[:n - 1, 0] + tn[:n - 1, 1])            # exact, in float64
    assert np.all(tn[n:] == 0.0)                                         # nothing past the accepted steps
    assert tn[n - 1, 0] < t1 <= tn[n - 1, 0] + tn[n - 1, 1]
    assert torch.equal(c["states"][0], c["hd"])
    d = float(np.abs(c["y64"] - c["sol"][-1].cpu().numpy().astype(np.float64)).max())
    print(f"{c['activation']} B={c['hd'].shape[0]} tol={c['tol']}: {n} accepted, {c['stats'][2]} rejected, "
          f"|y(t1) - float64 solve on the log| max {d:.2e}")
    # the solve's own tolerance; never below 1e-3: the device projection stops at |sum v| < 1e-4, the float64
    # one is exact (test_gpu_ode_backward_x.py measures 3e-5 between such trajectories at these horizons)
    assert d <= max(c["tol"], 1e-3), d
    return int(c["stats"][2])


@pytest.mark.parametrize("case", [("GroupSort", 1, 65, 1.0, 1e-3), ("ReLU", 1, 60, 1.0, 1e-3)])
def test_log_skips_a_rejected_attempt(case):
    """B = 1 solves whose controller rejects an attempt (in float64: once, 6 accepted): the log holds
    the accepted steps only and the solution and stats are the plain call's, bit for bit."""
    dev = _dev()
    c = solve_case(dev, *case)
    rejected = _check_log(dev, c)
    assert rejected >= 1, c["stats"]
    assert c["stats"][5] == c["n"] + rejected                            # attempts = accepted + rejected


@pytest.mark.parametrize("case", [k for k in CASES if k[1] > 1])
def test_log_is_the_solves_accepted_steps(case):
    dev = _dev()
    _check_log(dev, solve_case(dev, *case))


def test_log_past_the_capacity_is_not_written():
    """Capacity 2 on a 6-7 step solve: stats[1] counts every accepted step, the two logged ones are the
    full log's first two and the solution is unchanged."""
    from fiode_amd import ops
    dev = _dev()
    c = solve_case(dev, "GroupSort", 33, 40, 1.0, 1e-3)
    sol, stats, _, times, states = ops.odeint_dyn(c["xd"], c["hd"], c["tt"], c["w"], c["dyn"], method="dopri5",
                                                  rtol=1e-3, atol=1e-3, log_steps=2)
    assert int(stats[1]) == c["n"] > 2 and torch.equal(sol, c["sol"])
    assert times.shape == (2, 2) and states.shape == (2, 33, 10)
    assert torch.equal(times, c["times"][:2]) and torch.equal(states, c["states"][:2])


# ---- 2. gradients -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_gradients_match_the_frozen_step_torch_replay(case):
    dev = _dev()
    activation, B = case[0], case[1]
    c = solve_case(dev, *case)
    kept = int(c["keep"].sum())
    print(f"{case}: {c['n']} accepted steps (float64 controller {CASES[case][0]}), kept {kept} rows "
          f"(float64 controller {CASES[case][1]})")
    assert kept >= 10 or (B == 1 and kept == 1), kept
    y_ref, gh_ref, gx_ref = frozen_replay(dev, c)
    g_h0, g_x = native(dev, c)
    assert g_h0.shape == (B, 10) and g_x.shape == (B, 10)
    eh, ex = rel_err(g_h0, gh_ref), rel_err(g_x, gx_ref)
    print(f"{case}: |y replay - y solve| {float((y_ref - c['sol'][-1]).abs().max()):.2e}, g_h0 err {eh:.2e} of max "
          f"{float(gh_ref.abs().max()):.3f}, g_x err {ex:.2e} of max {float(gx_ref.abs().max()):.3f}")
    assert float(gh_ref.abs().max()) > 1e-3 and float(gx_ref.abs().max()) > 1e-3
    assert eh <= TOL, eh
    assert ex <= TOL, ex


# ---- 3. the replay ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("GroupSort", 33, 40, 1.0, 1e-3), ("GroupSort", 1, 65, 1.0, 1e-3),
                                  ("ReLU", 1, 64, 1.0, 1e-3)])
def test_replay_exit_iterations_and_stage_derivatives(case):
    """K[n][s] of the replay lies within +-1 of a per-evaluation ops.dyn_eval at the same stage inputs
    (rebuilt here from the log and the returned stage derivatives with the solve's float32 expressions);
    with equal K the stage derivatives agree to rounding (1e-6).  k7 exists for the last step only."""
    from fiode_amd import ops
    from fiode_amd.odeint import _BETA
    dev = _dev()
    c = solve_case(dev, *case)
    B, n = case[1], c["n"]
    _, _, dbg = native(dev, c, debug=True)
    Kx, ks = dbg["exit_iters"].cpu().numpy(), dbg["stage_k"]
    assert Kx.shape == (n, 7) and ks.shape == (n, 7, B, 10)
    assert np.all(Kx[:n - 1, 6] == -1) and Kx[n - 1, 6] >= 0
    assert float(ks[:n - 1, 6].abs().max()) == 0.0 if n > 1 else True
    beta = [[np.float32(v) for v in row] for row in _BETA]
    worst = 0
    for i in range(n):
        dt = np.float32(c["tn"][i, 1])
        y, k = c["states"][i], ks[i]
        for s in range(7 if i == n - 1 else 6):
            h = y
            if s > 0:
                acc = torch.zeros_like(y)
                for j in range(s):
                    acc = acc + k[j] * float(beta[s - 1][j] * dt)
                h = y + acc
            f, it = ops.dyn_eval(h.contiguous(), c["xd"], c["w"], c["dyn"])
            d = abs(int(it.item()) - int(Kx[i, s]))
            worst = max(worst, d)
            assert d <= 1, (i, s, int(it.item()), int(Kx[i, s]))
            if d == 0:
                assert float((f - k[s]).abs().max()) <= 1e-6, (i, s)
    # FSAL: k1 of step n + 1 is the k7 = f(y1) of step n, and y1 is the next logged state
    print(f"{case}: exit iterations {Kx.tolist()}, largest distance {worst}")


# ---- 4. the module ----------------------------------------------------------------------------------
def _module(dev, activation="GroupSort", seed=0):
    from tests.test_groupsort_dyn import build_module
    mod = build_module(activation, seed=seed).to(dev)
    mod.dyn_fun.scale_nominal = True
    mod.val_ode_solver, mod.val_ode_tol = "dopri5", 1e-3
    mod.eval()
    return mod


def _images(dev, B, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, 32, 32, generator=g).to(dev)


def _count(monkeypatch, obj, name):
    calls = []
    real = getattr(obj, name)

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(obj, name, wrapper)
    return calls


def test_module_forward_takes_the_native_dopri5_route(monkeypatch):
    from fiode_amd import odeint as OI
    from fiode_amd import ops
    from fiode_amd.lyapunov import no_param_grad
    dev = _dev()
    mod = _module(dev)
    x = _images(dev, 4)
    # as today: parameters require grad, the solve runs without grad (also the module's first forward, as in
    # test_module_forward_routes_rk4_to_the_native_backward: a fresh module's first forward was measured
    # 1.4e-5 from its later ones, with either route)
    xa = x.clone().requires_grad_(True)
    out = mod(xa)
    assert out.grad_fn is None and not out.requires_grad
    with torch.no_grad():
        clean = mod(x)
    bwd = _count(monkeypatch, ops, "odeint_dopri5_backward_x")
    stepper = _count(monkeypatch, OI, "_odeint_torch")
    with no_param_grad(mod):
        xb = x.clone().requires_grad_(True)
        out = mod(xb)
        assert out.grad_fn is not None and torch.equal(out.detach(), clean)
        loss = torch.nn.functional.cross_entropy(out, clean.argmax(-1))
        gx, = torch.autograd.grad(loss, xb)
        assert gx.shape == x.shape and bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
        assert len(bwd) == 1 and len(stepper) == 0
        # once differentiable
        xc = x.clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="differentiable once"):
            torch.autograd.grad(torch.nn.functional.cross_entropy(mod(xc), clean.argmax(-1)), xc, create_graph=True)
        # the switch puts the torch stepper back
        monkeypatch.setattr(OI, "DOPRI5_NATIVE_INPUT_GRAD", False)
        del bwd[:], stepper[:]
        xd = x.clone().requires_grad_(True)
        old = mod(xd)
        gx_old, = torch.autograd.grad(torch.nn.functional.cross_entropy(old, clean.argmax(-1)), xd)
        assert len(bwd) == 0 and len(stepper) == 1
        assert float((old.detach() - clean).abs().max()) <= 1e-3          # the solver's own tolerance
    print(f"image gradient max {float(gx.abs().max()):.3e}; torch stepper's {float(gx_old.abs().max()):.3e}, "
          f"distance {rel_err(gx, gx_old):.2e} (the routes' float32 controllers may accept different steps)")
    assert all(p.requires_grad for p in mod.parameters())


def test_validation_step_attacks_a_groupsort_module_with_dopri5(monkeypatch):
    from fiode_amd import odeint as OI
    from fiode_amd import ops
    dev = _dev()
    mod = _module(dev)
    mod.val_adv, mod.norm, mod.eps = True, "L2", 36 / 255
    mod.val_adv_generator = torch.Generator(device=dev).manual_seed(7)
    x = _images(dev, 4)
    with torch.no_grad():
        y = mod(x).argmax(-1)
    flags = [p.requires_grad for p in mod.parameters()]
    bwd = _count(monkeypatch, ops, "odeint_dopri5_backward_x")
    stepper = _count(monkeypatch, OI, "_odeint_torch")
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
    assert len(bwd) == 5 and len(stepper) == 0                           # one native backward per PGD iteration
    assert [p.requires_grad for p in mod.parameters()] == flags and not mod.training
    assert float(mod.logged["validation_adv_error"]) >= float(mod.logged["validation_error"])
