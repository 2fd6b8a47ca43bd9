"""CPU checks of the native input gradients of the dopri5 inference solve: the float64 reference of the
adjoint on the accepted steps (tests/_dopri5_grad_ref.py) against finite differences, the C-ABI boundary
of fiode_odeint_act_log / fiode_odeint_dopri5_backward_x, and the routing of
``fiode_amd.odeint._odeint_native_input_grad`` on a stub (no library call)."""
import ctypes as ct
import pathlib
import re
import types

import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _dopri5_grad_ref as D
from tests._util import make_params

ROOT = pathlib.Path(__file__).resolve().parents[1]


# ---- the float64 adjoint reference ----------------------------------------------------------------
# accepted steps of the float64 controller at rtol = atol = 1e-3 and the least share of rows kept
EXPECTED = {("ReLU", 0.25): (3, 0.5), ("ReLU", 1.0): (6, 0.5), ("GroupSort", 0.25): (3, 22 / 24),
            ("GroupSort", 1.0): (7, 22 / 24)}


@pytest.mark.parametrize("activation", ["ReLU", "GroupSort"])
@pytest.mark.parametrize("t1", [0.25, 1.0])
def test_adjoint_on_the_log_matches_finite_differences(activation, t1):
    """dL/dh0 and dL/dx of L = sum(g_y * y(t1)) from the restated adjoint against central differences
    (step 1e-7) of ``solve_on_log`` on the SAME log (the steps are constants of the gradient), the
    inputs of test_ode_backward_x.py.  Rows within 1e-5 of a kink in any evaluation are left out (at
    most half of them); the others agree to 1e-6 of the array's max, that file's tolerance."""
    B = 24
    P = make_params(seed=21)
    cfg = O.DynConfig(scale_nominal=True)
    rng = np.random.default_rng(22)
    h0 = rng.dirichlet(np.ones(10), B)
    x = rng.normal(0, 1, (B, 10))
    g_y = rng.normal(size=(B, 10))
    times, dts, n_rej = D.controller_solve(h0, x, P, cfg, activation, 0.0, t1, 1e-3, 1e-3)
    n_exp, keep_min = EXPECTED[(activation, t1)]
    assert len(times) == n_exp, (len(times), n_rej)
    assert times[0] == 0.0 and times[-1] < t1 <= times[-1] + dts[-1]
    on_log = lambda hh, xx: D.solve_on_log(hh, xx, P, cfg, activation, times, dts, t1)
    y, states, ks, margin = on_log(h0, x)
    assert states.shape == (n_exp, B, 10) and ks.shape == (n_exp, 7, B, 10)
    g_h0, g_x = D.adjoint_on_log(g_y, x, P, cfg, activation, times, dts, t1, states, ks)
    keep = margin >= 1e-5
    assert keep.mean() >= keep_min, keep.mean()
    d = 1e-7
    fd_h, fd_x = np.zeros_like(h0), np.zeros_like(x)
    for j in range(10):
        e = np.zeros(10)
        e[j] = d
        fd_h[:, j] = ((on_log(h0 + e, x)[0] - on_log(h0 - e, x)[0]) * g_y).sum(1) / (2 * d)
        fd_x[:, j] = ((on_log(h0, x + e)[0] - on_log(h0, x - e)[0]) * g_y).sum(1) / (2 * d)
    for name, fd, g in (("g_h0", fd_h, g_h0), ("g_x", fd_x, g_x)):
        scale = float(np.abs(g).max())
        err = float(np.abs(fd - g)[keep].max())
        print(f"{activation} t1 {t1} {name}: {n_exp} steps, {n_rej} rejected, kept {keep.mean():.2f}, "
              f"err {err / scale:.2e} of max {scale:.3f}")
        assert scale > 1e-3
        assert err <= 1e-6 * scale, (name, err, scale)


def test_dense_output_weights_sum_as_the_quartic_requires():
    """At x = 1 the dense output is y1, at x = 0 it is y, and the weights of (y, y1, ymid) sum to one."""
    for tn, dtn, t1 in ((0.75, 0.25, 1.0), (0.5, 0.7, 0.5), (0.6, 0.7, 1.0)):
        p0, p1, pm, pa, pb = D.interp_weights(tn, dtn, t1)
        assert abs(p0 + p1 + pm - 1.0) < 1e-12
        if t1 == tn + dtn:
            assert (p0, p1, pm, pa, pb) == (0.0, 1.0, 0.0, 0.0, 0.0)
        if t1 == tn:
            assert (p0, p1, pm, pa, pb) == (1.0, 0.0, 0.0, 0.0, 0.0)


# ---- the C-ABI ------------------------------------------------------------------------------------
NEW_SYMBOLS = ("fiode_odeint_act_log", "fiode_odeint_dopri5_backward_x_workspace_bytes",
               "fiode_odeint_dopri5_backward_x")


def test_header_declares_and_library_exports_the_entry_points():
    from fiode_amd import _lib
    text = (ROOT / "include" / "fiode.h").read_text()
    syms = re.findall(r"FIODE_API\s+[\w\s\*]+?\b(fiode_\w+)\s*\(", text)
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert re.search(r"#define\s+FIODE_ODEINT_LOG_MAX_STEPS\s+1024\b", text)
    assert _lib.FIODE_ODEINT_LOG_MAX_STEPS == 1024
    assert lib.fiode_abi_version() == 5 == _lib.ABI_VERSION          # new symbols only


def _dyn(L, **kw):
    f = dict(n_hidden=10, mlp_size=128, x_dim=10, alpha_1=100.0, alpha_2=20.0, sigma_1=0.02, scale_nominal=1,
             dropout=0.5, qp_max_iter=30, qp_tol=1e-4)
    f.update(kw)
    return L.DynConfig(*f.values())


def _bwd(lib, L, *, dyn=None, act=0, batch=4, n_steps=6, t1=1.0, times=1, states=1, x=1, g_y=1, g_h0=1, g_x=1,
         w_null=None, nbytes=0):
    d = ct.c_void_p(1)
    dyn = dyn or _dyn(L)
    w = L.DynWeights(*([d] * 8))
    if w_null:
        setattr(w, w_null, None)
    p = lambda v: d if v else None
    return lib.fiode_odeint_dopri5_backward_x(None, ct.byref(dyn), ct.byref(w), batch, n_steps, t1, p(times), p(states),
                                              p(x), p(g_y), p(g_h0), p(g_x), None, None, d, nbytes, act)


def test_backward_checks_arguments_before_workspace():
    """Every argument check runs on the host before the workspace-size check, and nothing is launched
    on an error (dummy non-NULL pointers, a zero-byte workspace)."""
    from fiode_amd import _lib as L
    lib = L.lib()
    EINVAL, ESHAPE, EWORKSPACE = 1, 2, 3
    assert _bwd(lib, L, act=0) == EWORKSPACE and _bwd(lib, L, act=1) == EWORKSPACE
    assert _bwd(lib, L, act=2) == EINVAL and _bwd(lib, L, act=-1) == EINVAL
    assert _bwd(lib, L, n_steps=0) == EINVAL and _bwd(lib, L, n_steps=-1) == EINVAL
    assert _bwd(lib, L, n_steps=1025) == EINVAL
    assert _bwd(lib, L, n_steps=1) == EWORKSPACE and _bwd(lib, L, n_steps=1024) == EWORKSPACE
    assert _bwd(lib, L, batch=0) == EINVAL and _bwd(lib, L, batch=-1) == EINVAL
    assert _bwd(lib, L, batch=L.FIODE_ODEINT_MAX_BATCH + 1) == EINVAL
    assert _bwd(lib, L, t1=float("nan")) == EINVAL
    assert _bwd(lib, L, dyn=_dyn(L, n_hidden=12)) == ESHAPE
    assert _bwd(lib, L, dyn=_dyn(L, qp_max_iter=33)) == EINVAL
    for k in ("times", "states", "x", "g_y", "g_h0", "g_x"):
        assert _bwd(lib, L, **{k: 0}) == EINVAL, k
    assert _bwd(lib, L, w_null="Q2") == EINVAL
    # the workspace: the stage derivatives, one pass's MLP outputs, u and g_u; no [N][128] arrays
    B, n = 128, 7
    nb = lib.fiode_odeint_dopri5_backward_x_workspace_bytes(B, n)
    assert 8 * n * B * 10 * 4 + 2 * B * 128 * 4 <= nb <= 8 * n * B * 10 * 4 + 2 * B * 128 * 4 + 4096
    assert _bwd(lib, L, batch=B, n_steps=n, nbytes=nb - 1) == EWORKSPACE
    for bad in ((0, 6), (4, 0), (4, 1025), (L.FIODE_ODEINT_MAX_BATCH + 1, 6)):
        assert lib.fiode_odeint_dopri5_backward_x_workspace_bytes(*bad) == 256


def _solve(lib, L, *, act=0, batch=4, method=1, log=(8, 1, 1), nbytes=0, n_times=2):
    d = ct.c_void_p(1)
    cfg = L.OdeConfig(method, batch, n_times, 0, 1e-3, 1e-3, 0.25)
    dyn = _dyn(L)
    w = L.DynWeights(*([d] * 8))
    cap, times, states = log
    return lib.fiode_odeint_act_log(None, ct.byref(cfg), ct.byref(dyn), ct.byref(w), d, d, d, d, d, d, d, nbytes, act,
                                    cap, d if times else None, d if states else None)


def test_logged_solve_checks_arguments_before_workspace():
    from fiode_amd import _lib as L
    lib = L.lib()
    EINVAL, EWORKSPACE = 1, 3
    assert _solve(lib, L) == EWORKSPACE and _solve(lib, L, act=1) == EWORKSPACE
    assert _solve(lib, L, log=(0, 0, 0)) == EWORKSPACE             # no log: fiode_odeint_act
    assert _solve(lib, L, log=(8, 1, 0)) == EINVAL and _solve(lib, L, log=(8, 0, 1)) == EINVAL
    assert _solve(lib, L, log=(0, 1, 1)) == EINVAL and _solve(lib, L, log=(-1, 1, 1)) == EINVAL
    assert _solve(lib, L, log=(1025, 1, 1)) == EINVAL and _solve(lib, L, log=(1024, 1, 1)) == EWORKSPACE
    assert _solve(lib, L, act=2) == EINVAL
    assert _solve(lib, L, batch=0) == EINVAL and _solve(lib, L, n_times=1) == EINVAL
    assert _solve(lib, L, method=0) == EWORKSPACE                  # rk4 ignores the log
    assert lib.fiode_odeint_workspace_bytes(4) > 256


def test_ops_wrappers_refuse_bad_arguments_before_any_library_call():
    from fiode_amd import ops
    P = make_params(seed=1)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))) for k in ops.WEIGHT_KEYS}
    dyn = ops.DynCfg(dropout=0.0, activation="GroupSort")
    z = torch.zeros(4, 10)
    kw = dict(t1=1.0, step_times=torch.zeros(8, 2, dtype=torch.float64), step_states=torch.zeros(8, 4, 10))
    with pytest.raises(ValueError, match="activation"):
        ops.odeint_dopri5_backward_x(z, z, w, ops.DynCfg(activation="Tanh"), n_steps=6, **kw)
    for n in (0, 1025):
        with pytest.raises(ValueError, match="n_steps"):
            ops.odeint_dopri5_backward_x(z, z, w, dyn, n_steps=n, **kw)
    with pytest.raises(ValueError, match="step log"):
        ops.odeint_dopri5_backward_x(z, z, w, dyn, n_steps=9, **kw)
    with pytest.raises(ValueError, match="ROCm device"):
        ops.odeint_dopri5_backward_x(z, z, w, dyn, n_steps=6, **kw)
    with pytest.raises(ValueError, match="log_steps"):
        ops.odeint_dyn(z, z, torch.zeros(2, dtype=torch.float64), w, dyn, log_steps=1025)


# ---- routing on a stub -----------------------------------------------------------------------------
class _Dyn:
    """What _odeint_native_input_grad reads of the dynamics module."""

    def __init__(self, activation, B):
        from fiode_amd import ops
        self.static_state = torch.zeros(B, 10, requires_grad=True)
        self._cfg = ops.DynCfg(dropout=0.0, activation=activation)

    def dyn_cfg(self):
        return self._cfg

    def effective_weights(self):
        from fiode_amd import ops
        return {k: torch.zeros(ops.WEIGHT_SHAPES[k]) for k in ops.WEIGHT_KEYS}

    def _eval(self, y, x):
        return y


@pytest.fixture
def routes(monkeypatch):
    """Every route replaced by a recorder: the Functions' ``apply`` and the torch stepper."""
    from fiode_amd import odeint as OI
    from fiode_amd import ops
    seen = []

    def fake(name, overflow=False):
        def apply(dyn, plan, h0, x, *w):
            seen.append((name, plan))
            if overflow:
                raise OI._Dopri5LogOverflow(plan["capacity"] + 1)
            return torch.zeros_like(h0)
        return types.SimpleNamespace(apply=apply)

    for name in ("_OdeintRk4XFn", "_OdeintDopri5XFn", "_OdeintDopri5LogXFn"):
        monkeypatch.setattr(OI, name, fake(name))
    monkeypatch.setattr(OI, "_odeint_torch", lambda f, y0, t, *a, **k: (seen.append(("torch", None)),
                                                                         torch.zeros(t.numel(), *y0.shape))[1])
    monkeypatch.setattr(ops, "rk4_grid", lambda *a: np.zeros(5))
    monkeypatch.setattr(ops, "odetrain_config", lambda *a, **k: "cfg")
    monkeypatch.setattr(ops, "odetrain_default_attempts", lambda B: 64)
    return types.SimpleNamespace(OI=OI, seen=seen, fake=fake, monkeypatch=monkeypatch)


def _route(routes, method, activation, h0_grad, n_times, B=4):
    dyn = _Dyn(activation, B)
    h0 = torch.full((B, 10), 0.1, requires_grad=h0_grad)
    t = torch.linspace(0.0, 1.0, n_times)
    del routes.seen[:]
    opts = dict(step_size=0.25) if method == "rk4" else {}
    sol = routes.OI._odeint_native_input_grad(dyn, h0, t, 1e-3, 1e-3, method, opts)
    assert sol.shape == (n_times, B, 10)
    return [s[0] for s in routes.seen]


@pytest.mark.parametrize("activation", ["ReLU", "GroupSort"])
@pytest.mark.parametrize("h0_grad", [False, True])
@pytest.mark.parametrize("n_times", [2, 3])
def test_routing_of_every_combination(routes, activation, h0_grad, n_times):
    LOG, TRAIN, RK4, TORCH = "_OdeintDopri5LogXFn", "_OdeintDopri5XFn", "_OdeintRk4XFn", "torch"
    assert _route(routes, "rk4", activation, h0_grad, n_times) == [RK4 if n_times == 2 else TORCH]
    want = TORCH if n_times != 2 else (TRAIN if activation == "ReLU" and not h0_grad else LOG)
    assert _route(routes, "dopri5", activation, h0_grad, n_times) == [want]


def test_routing_relu_past_the_train_solves_batch_takes_the_log_route(routes):
    from fiode_amd import _lib as L
    B = L.FIODE_ODE_MAX_BATCH + 1
    assert _route(routes, "dopri5", "ReLU", False, 2, B=B) == ["_OdeintDopri5LogXFn"]
    plan = routes.seen[0][1]
    assert plan["capacity"] == routes.OI.dopri5_log_capacity(B) == 128
    assert (plan["t0"], plan["t1"], plan["rtol"], plan["atol"]) == (0.0, 1.0, 1e-3, 1e-3)
    assert routes.OI.dopri5_log_capacity(65536) == 102 and routes.OI.dopri5_log_capacity(10 ** 9) == 8


def test_routing_switch_off_puts_the_torch_stepper_back(routes):
    assert routes.OI.DOPRI5_NATIVE_INPUT_GRAD is True
    routes.monkeypatch.setattr(routes.OI, "DOPRI5_NATIVE_INPUT_GRAD", False)
    assert _route(routes, "dopri5", "GroupSort", False, 2) == ["torch"]
    assert _route(routes, "dopri5", "ReLU", True, 2) == ["torch"]
    assert _route(routes, "dopri5", "ReLU", False, 2) == ["_OdeintDopri5XFn"]       # unchanged
    assert _route(routes, "rk4", "GroupSort", False, 2) == ["_OdeintRk4XFn"]


def test_routing_more_accepted_steps_than_the_log_holds_runs_the_torch_stepper(routes):
    routes.monkeypatch.setattr(routes.OI, "_OdeintDopri5LogXFn", routes.fake("_OdeintDopri5LogXFn", overflow=True))
    assert _route(routes, "dopri5", "GroupSort", False, 2) == ["_OdeintDopri5LogXFn", "torch"]


def test_logged_function_raises_overflow_on_n_accept_above_capacity(monkeypatch):
    """The Function's forward on a stubbed solve: n_accept above the capacity raises the overflow the
    router catches; a bad status raises as the no-grad solve does."""
    from fiode_amd import odeint as OI
    from fiode_amd import ops

    def solve(n_accept, status=0):
        def fn(x, h0, times, w, dyn, **kw):
            assert kw["method"] == "dopri5" and kw["log_steps"] == 8
            stats = torch.tensor([0, n_accept, 0, status, 0, n_accept, 1, 1], dtype=torch.int32)
            return (torch.zeros(2, 4, 10), stats, torch.zeros(4, dtype=torch.float64),
                    torch.zeros(8, 2, dtype=torch.float64), torch.zeros(8, 4, 10))
        return fn
    plan = dict(dyn=ops.DynCfg(), t0=0.0, t1=1.0, rtol=1e-3, atol=1e-3, max_steps=100, capacity=8)
    mod = types.SimpleNamespace(last_solve_stats=None)
    h0 = torch.zeros(4, 10, requires_grad=True)
    ws = [torch.zeros(ops.WEIGHT_SHAPES[k]) for k in ops.WEIGHT_KEYS]
    monkeypatch.setattr(ops, "odeint_dyn", solve(9))
    with pytest.raises(OI._Dopri5LogOverflow):
        OI._OdeintDopri5LogXFn.apply(mod, plan, h0, torch.zeros(4, 10), *ws)
    monkeypatch.setattr(ops, "odeint_dyn", solve(8))
    y = OI._OdeintDopri5LogXFn.apply(mod, plan, h0, torch.zeros(4, 10), *ws)
    assert y.grad_fn is not None and mod.last_solve_stats is not None
    monkeypatch.setattr(ops, "odeint_dyn", solve(3, status=2))
    with pytest.raises(RuntimeError, match="max_num_steps"):
        OI._OdeintDopri5LogXFn.apply(mod, plan, h0, torch.zeros(4, 10), *ws)
