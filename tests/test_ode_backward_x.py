"""CPU checks of the differentiable inference solve and the PGD validation: the float64 reference of
the RK4 adjoint (tests/_ode_grad_ref.py) against finite differences, ``no_param_grad``, the two
attacks of ``fiode_amd.attacks``, ``validation_step`` with ``val_adv`` on a stub module, and the
C-ABI boundary of fiode_odeint_backward_x."""
import ctypes as ct
import pathlib
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import fiode_oracle as O
from tests import _ode_grad_ref as R
from tests._util import make_params

ROOT = pathlib.Path(__file__).resolve().parents[1]


# ---- the float64 adjoint reference ----------------------------------------------------------------
@pytest.mark.parametrize("activation", ["ReLU", "GroupSort"])
@pytest.mark.parametrize("step", [0.25, 0.3])
def test_adjoint_reference_matches_finite_differences(activation, step):
    """dL/dh0 and dL/dx of L = sum(g_y * y(1)) from the restated adjoint against central differences
    (step 1e-7) of the float64 solve with the exact projection, scale_nominal=True.  Rows that pass
    within 1e-5 of a kink (QP active-set change, ReLU zero, GroupSort tie) in any of the 16
    evaluations are left out (at most half of them); the others agree to 1e-6 of the array's max,
    the tolerance of test_dyn_backward.py.  A row meets 16 x 256 hidden units on its way, so the
    1e-4 margin of the single-evaluation test would leave out 80 % of the ReLU rows; the margin and
    the difference step are both ten times smaller here (the margin stays 100 x the step, and the
    projection's multiplier is bisected to float64 resolution, so the step is still far above the
    noise of the difference quotient)."""
    B = 24
    P = make_params(seed=21)
    cfg = O.DynConfig(scale_nominal=True)
    rng = np.random.default_rng(22)
    h0 = rng.dirichlet(np.ones(10), B)
    x = rng.normal(0, 1, (B, 10))
    g_y = rng.normal(size=(B, 10))
    _, states, ks, margin = R.solve(h0, x, P, cfg, activation, 0.0, 1.0, step)
    assert states.shape[0] == 5 and ks.shape[:2] == (4, 4)          # 4 steps (0.3: the last one 0.1)
    g_h0, g_x = R.adjoint(g_y, x, P, cfg, activation, 0.0, 1.0, step, states, ks)
    keep = margin >= 1e-5
    assert keep.mean() >= 0.5, keep.mean()
    d = 1e-7
    fd_h, fd_x = np.zeros_like(h0), np.zeros_like(x)
    for j in range(10):
        e = np.zeros(10)
        e[j] = d
        yp = R.solve(h0 + e, x, P, cfg, activation, 0.0, 1.0, step)[0]
        ym = R.solve(h0 - e, x, P, cfg, activation, 0.0, 1.0, step)[0]
        fd_h[:, j] = ((yp - ym) * g_y).sum(1) / (2 * d)
        yp = R.solve(h0, x + e, P, cfg, activation, 0.0, 1.0, step)[0]
        ym = R.solve(h0, x - e, P, cfg, activation, 0.0, 1.0, step)[0]
        fd_x[:, j] = ((yp - ym) * g_y).sum(1) / (2 * d)
    for name, fd, g in (("g_h0", fd_h, g_h0), ("g_x", fd_x, g_x)):
        scale = float(np.abs(g).max())
        err = float(np.abs(fd - g)[keep].max())
        print(f"{activation} step {step} {name}: kept {keep.mean():.2f}, err {err / scale:.2e} of max {scale:.3f}")
        assert scale > 1e-3
        assert err <= 1e-6 * scale, (name, err, scale)


# ---- no_param_grad --------------------------------------------------------------------------------
def test_no_param_grad_restores_flags_and_modes_after_an_exception():
    from fiode_amd.lyapunov import no_param_grad
    net = nn.Sequential(nn.Linear(3, 4), nn.Dropout(0.5), nn.Sequential(nn.Linear(4, 2)))
    net[0].bias.requires_grad_(False)
    net[2].eval()
    flags = [p.requires_grad for p in net.parameters()]
    modes = [m.training for m in net.modules()]
    assert flags == [True, False, True, True] and modes == [True, True, True, False, False]
    with pytest.raises(KeyError):
        with no_param_grad(net) as m:
            assert m is net
            assert not any(p.requires_grad for p in net.parameters())
            assert not any(s.training for s in net.modules())
            x = torch.ones(1, 3, requires_grad=True)
            net(x).sum().backward()
            assert x.grad is not None and all(p.grad is None for p in net.parameters())
            raise KeyError("inside")
    assert [p.requires_grad for p in net.parameters()] == flags
    assert [m.training for m in net.modules()] == modes


# ---- the attacks ----------------------------------------------------------------------------------
def _toy(seed=0):
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Flatten(), nn.Linear(3 * 4 * 4, 16), nn.Tanh(), nn.Linear(16, 10))
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(6, 3, 4, 4, generator=g)
    x[0] = 0.0                      # images on the faces of [0, 1]: the clamp must hold them
    x[1] = 1.0
    y = torch.randint(0, 10, (6,), generator=g)
    return net, x, y


@pytest.mark.parametrize("name,eps", [("PGDL2", 0.5), ("PGD", 8 / 255)])
@pytest.mark.parametrize("random_start", [True, False])
def test_attacks_stay_in_the_ball_and_do_not_lower_the_loss(name, eps, random_start):
    from fiode_amd import attacks
    net, x, y = _toy()
    cls = getattr(attacks, name)
    mk = lambda seed: cls(net, eps=eps, alpha=eps * 2.5 / 10, steps=5, random_start=random_start,
                          generator=torch.Generator().manual_seed(seed))
    adv = mk(5)(x, y)
    assert adv.shape == x.shape and not adv.requires_grad
    assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
    delta = (adv - x).flatten(1)
    if name == "PGDL2":
        assert float(delta.norm(dim=1).max()) <= eps * (1 + 1e-5)
    else:
        assert float(delta.abs().max()) <= eps + 1e-7
    assert float(delta.abs().max()) > 0
    assert torch.equal(adv, mk(5)(x, y))                      # deterministic given the generator
    if random_start:
        assert not torch.equal(adv, mk(6)(x, y))
    ce = nn.CrossEntropyLoss()
    with torch.no_grad():
        assert float(ce(net(adv), y)) >= float(ce(net(x), y))
    assert all(p.grad is None for p in net.parameters())      # the gradient is the image's only


def test_pgdl2_step_and_projection_formulas():
    """One step without a random start from a model with a known gradient: x + alpha g / (|g| + 1e-10),
    then delta min(1, eps / |delta|)."""
    from fiode_amd import attacks
    w = torch.tensor([3.0, -4.0])

    class Lin(nn.Module):
        def forward(self, z):
            s = (z.flatten(1) * w).sum(1, keepdim=True)
            return torch.cat([s, torch.zeros_like(s)], 1)
    x = torch.full((1, 2), 0.5)
    y = torch.tensor([1])
    # d CE / d x = p0 * w with label 1: direction w / |w| = (0.6, -0.8)
    adv = attacks.PGDL2(Lin(), eps=0.1, alpha=0.05, steps=1, random_start=False)(x, y)
    assert torch.allclose(adv, torch.tensor([[0.53, 0.46]]), atol=1e-6)
    adv = attacks.PGDL2(Lin(), eps=0.1, alpha=0.05, steps=5, random_start=False)(x, y)
    assert torch.allclose(adv, torch.tensor([[0.56, 0.42]]), atol=1e-6)          # on the eps sphere
    adv = attacks.PGD(Lin(), eps=0.1, alpha=0.04, steps=5, random_start=False)(x, y)
    assert torch.allclose(adv, torch.tensor([[0.6, 0.4]]), atol=1e-6)


# ---- validation_step -------------------------------------------------------------------------------
def _stub(val_adv, norm="L2", eps=0.5):
    from fiode_amd.lyapunov import LyapunovLearning

    class _Stub(LyapunovLearning):
        """validation_step with the solve replaced by a small differentiable torch model (the HIP solve
        needs a GPU), as tests/test_distributed.py does: __init__ is skipped."""
        def __init__(self):
            nn.Module.__init__(self)
            self.simplex, self.logged = True, {}
            torch.manual_seed(3)
            self.net = nn.Sequential(nn.Flatten(), nn.Linear(3 * 4 * 4, 10))
            self.calls = []

        def forward(self, x, t_steps=2, return_traj=False):
            self.calls.append((x.detach().clone(), torch.is_grad_enabled(), x.requires_grad, self.training,
                               any(p.requires_grad for p in self.parameters())))
            return torch.softmax(4.0 * self.net(x), -1)
    m = _Stub()
    if val_adv is not None:
        m.val_adv, m.norm, m.eps = val_adv, norm, eps
        m.val_adv_generator = torch.Generator().manual_seed(9)
    return m


@pytest.mark.parametrize("norm", ["L2", "Linf"])
def test_validation_step_runs_the_attack(norm):
    from fiode_amd import attacks
    eps = 0.5 if norm == "L2" else 0.1
    m = _stub(True, norm, eps)
    m.train()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(32, 3, 4, 4, generator=g)
    with torch.no_grad():
        y = m.net(x).argmax(-1)                 # every clean prediction is right
    m.calls.clear()
    m.validation_step((x, y))
    # five attack forwards (grad on, input requires grad, eval mode, no parameter requires grad), then
    # the clean and the adversarial forward without grad, in the caller's mode
    assert len(m.calls) == 7
    assert all(c[1:] == (True, True, False, False) for c in m.calls[:5])
    assert all(c[1:] == (False, False, True, True) for c in m.calls[5:])
    assert torch.equal(m.calls[5][0], x)
    adv = m.calls[6][0]
    cls = attacks.PGDL2 if norm == "L2" else attacks.PGD
    with torch.no_grad():
        own = cls(lambda z: torch.softmax(4.0 * m.net(z), -1), eps=eps, alpha=eps * 2.5 / 10, steps=5,
                  generator=torch.Generator().manual_seed(9))(x, y)
        err_adv = (m.net(adv).argmax(-1) != y).float().mean()
    assert torch.equal(adv, own)
    assert float(m.logged["validation_error"]) == 0.0
    assert float(err_adv) > 0.0                                   # the attack flips some of them
    assert float(m.logged["validation_adv_error"]) == float(err_adv)
    assert m.training and all(p.requires_grad for p in m.parameters())


def test_validation_step_without_val_adv_is_unchanged():
    for val_adv in (None, False):               # None: the attribute is absent (a stub that skips __init__)
        m = _stub(val_adv)
        x = torch.rand(8, 3, 4, 4, generator=torch.Generator().manual_seed(1))
        y = torch.arange(8) % 10
        m.validation_step((x, y))
        assert len(m.calls) == 1 and m.calls[0][1] is False
        assert m.logged["validation_adv_error"] is m.logged["validation_error"]


def test_validation_attack_refuses_an_unknown_norm():
    m = _stub(True, "L1")
    with pytest.raises(ValueError, match="L1"):
        m.validation_step((torch.rand(2, 3, 4, 4), torch.zeros(2, dtype=torch.long)))


# ---- the C-ABI ------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from fiode_amd import _lib
    text = (ROOT / "include" / "fiode.h").read_text()
    syms = re.findall(r"FIODE_API\s+[\w\s\*]+?\b(fiode_\w+)\s*\(", text)
    lib = _lib.lib()
    for s in ("fiode_odeint_backward_x", "fiode_odeint_backward_x_workspace_bytes", "fiode_odeint_backward_x_steps"):
        assert s in syms, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.fiode_abi_version() == 5 == _lib.ABI_VERSION


def _call(lib, L, *, dyn=None, act=0, batch=4, t=(0.0, 1.0, 0.25), x=1, states=1, g_y=1, g_h0=1, g_x=1, w_null=None,
          nbytes=0):
    d = ct.c_void_p(1)
    dyn = dyn or L.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
    w = L.DynWeights(*([d] * 8))
    if w_null:
        setattr(w, w_null, None)
    p = lambda v: d if v else None
    return lib.fiode_odeint_backward_x(None, ct.byref(dyn), ct.byref(w), batch, t[0], t[1], t[2], p(x), p(states),
                                       p(g_y), p(g_h0), p(g_x), None, None, d, nbytes, act)


def test_entry_points_check_arguments_before_workspace():
    """Every argument check runs on the host before the workspace-size check, and nothing is launched
    on an error (dummy non-NULL pointers, a zero-byte workspace)."""
    from fiode_amd import _lib as L
    lib = L.lib()
    EINVAL, ESHAPE, EWORKSPACE = 1, 2, 3
    assert _call(lib, L, act=0) == EWORKSPACE and _call(lib, L, act=1) == EWORKSPACE
    assert _call(lib, L, act=2) == EINVAL and _call(lib, L, act=-1) == EINVAL
    assert _call(lib, L, dyn=L.DynConfig(12, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)) == ESHAPE
    assert _call(lib, L, dyn=L.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 33, 1e-4)) == EINVAL
    for k in ("x", "states", "g_y", "g_h0", "g_x"):
        assert _call(lib, L, **{k: 0}) == EINVAL, k
    assert _call(lib, L, w_null="Q2") == EINVAL
    assert _call(lib, L, batch=0) == EINVAL and _call(lib, L, batch=-1) == EINVAL
    assert _call(lib, L, batch=L.FIODE_ODEINT_MAX_BATCH + 1) == EINVAL
    for t in ((0.0, 1.0, 0.0), (0.0, 1.0, -0.1), (1.0, 1.0, 0.1), (1.0, 0.0, 0.1), (0.0, 1.0, 1e-4),
              (0.0, 1.0, float("nan"))):
        assert _call(lib, L, t=t) == EINVAL, t
        assert lib.fiode_odeint_backward_x_steps(*t) == -1, t
        assert lib.fiode_odeint_backward_x_workspace_bytes(4, *t) == 256
    # the grid of FixedGridODESolver: ceil((t1 - t0) / h + 1) - 1 steps
    assert lib.fiode_odeint_backward_x_steps(0.0, 1.0, 0.25) == 4
    assert lib.fiode_odeint_backward_x_steps(0.0, 1.0, 0.3) == 4
    assert lib.fiode_odeint_backward_x_steps(0.0, 1.0, 0.1) == 10
    assert lib.fiode_odeint_backward_x_steps(0.0, 1.0, 2.0) == 1
    # no [N][128] activation arrays: the stage derivatives, one pass's MLP outputs, u and g_u
    B, n = 128, 10
    nb = lib.fiode_odeint_backward_x_workspace_bytes(B, 0.0, 1.0, 0.1)
    assert 5 * n * B * 10 * 4 + 2 * B * 128 * 4 <= nb <= 5 * n * B * 10 * 4 + 2 * B * 128 * 4 + 4096
    assert lib.fiode_odeint_backward_x_workspace_bytes(0, 0.0, 1.0, 0.1) == 256


def test_rk4_grid_is_the_solves_float32_grid():
    from fiode_amd import ops
    g = ops.rk4_grid(0.0, 1.0, 0.3)
    h = np.float32(0.3)
    assert g.dtype == np.float64 and len(g) == 5 and g[-1] == 1.0
    assert [np.float32(v) for v in g[:4]] == [np.float32(0), h, np.float32(2) * h, np.float32(3) * h]
    assert len(ops.rk4_grid(0.0, 1.0, 0.25)) == 5 and len(ops.rk4_grid(0.0, 1.0, 0.1)) == 11
    with pytest.raises(ValueError):
        ops.rk4_grid(0.0, 1.0, 0.0)


def test_ops_wrapper_refuses_mismatched_shapes():
    """ops.odeint_backward_x checks shapes and devices before any library call (host tensors: nothing
    can launch)."""
    from fiode_amd import ops
    P = make_params(seed=1)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))) for k in ops.WEIGHT_KEYS}
    dyn = ops.DynCfg(dropout=0.0)
    kw = dict(t0=0.0, t1=1.0, step_size=0.25)
    with pytest.raises(ValueError, match="activation"):
        ops.odeint_backward_x(torch.zeros(4, 10), torch.zeros(4, 10), torch.zeros(4, 10), w,
                              ops.DynCfg(activation="Tanh"), **kw)
    with pytest.raises(ValueError, match="ROCm device"):
        ops.odeint_backward_x(torch.zeros(4, 10), torch.zeros(4, 10), torch.zeros(4, 10), w, dyn, **kw)
