"""GPU parity of the GroupSort dynamics (fiode_dyn_eval_act / fiode_odeint_act / fiode_certify_act
with FIODE_ACT_GROUPSORT) against the oracle with a float64 GroupSort MLP installed
(tests/_groupsort_ref.py), and bit-identity of the FIODE_ACT_RELU case with the base entry points.

Tolerances are the ReLU tests' (test_gpu_lyap.py:190-192, test_gpu_ode.py:4-7, test_gpu_certify.py:4-6):
the only difference between device and reference is the MLP's float32 accumulation order, which
GroupSort (a selection, exact) does not change.  The GroupSort and ReLU references differ by 0.05 to
2.0 on these inputs, so a kernel that still applied ReLU, or paired the wrong units, cannot pass.
"""
import ctypes as ct

import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _groupsort_ref as R
from tests._util import make_params

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _groupsort_oracle(monkeypatch):
    monkeypatch.setattr(O, "mlp_forward", R.mlp_forward)


def _wt(P, dev):
    from fiode_amd import ops
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}


def _gs(scale_nominal):
    from fiode_amd import ops
    return ops.DynCfg(scale_nominal=scale_nominal, dropout=0.0, activation="GroupSort")


# ---- 1. exact pairing on the 32-row tiles --------------------------------------------------------
# The barrier of the dyadic test.  The MLP output is exact, so what is left between device and
# reference is the QP, and with the default constants that is not small: lower = -alpha_1 (exp(sigma_1
# h) - 1) cancels, so one ulp of expf is alpha_1 2^-23 = 1.2e-5 in lower at alpha_1 = 100, the bracket's
# upper end max(nominal - lower) moves with it, and a bisection that stops at the first iteration with
# |eps| < 1e-4 (iteration 18 here) answers on a grid of (hi - lo) / 2^19 ~ 1e-4: perturbing exp by
# +-2 ulp in the REFERENCE alone moves its f by 2e-4 (measured on the host; the device's first run
# differed by 1.8e-4 with the exit iteration equal).  With alpha_1 = 1, sigma_1 = 2 (lower between 0
# and -1.72 on these rows, one ulp of expf <= 2.4e-7) and a tolerance no row can meet, both sides run
# all 30 iterations and answer to the float32 resolution of the multiplier (|mu| <= 9.5: ulp 9.5e-7);
# the same +-2 ulp perturbation then moves the reference by 1.9e-6, five times inside the bound.
DYADIC_BARRIER = dict(alpha_1=1.0, sigma_1=2.0, qp_tol=1e-12)


def test_dyn_eval_dyadic_pairing_exact():
    """Dyadic weights (tests/_groupsort_ref.py): the MLP output is the same bits on both sides in any
    accumulation order, every pair (u, u + 64) of both layers is >= 0.25 apart on every row, and
    which unit of a layer-1 pair is the larger changes from row to row.  N = 150 rows (B=50, S=3):
    four full 32-row tiles and one of 22 rows.  Bound 1e-5 on |f| <= 3 (DYADIC_BARRIER: why the QP
    resolves that), four orders below the 0.25 a mis-paired unit moves; the GroupSort and ReLU
    references differ by 3.1 here."""
    from fiode_amd import ops
    dev = _dev()
    P, h = R.dyadic_params(), R.dyadic_rows(150)
    x = np.random.default_rng(5).normal(size=(50, 10)).astype(np.float32)      # Qx = 0: no effect
    ref = O.eval_dot(h, np.repeat(O.static_projection(x, P), 3, 0), P,
                     O.DynConfig(scale_nominal=False, **DYADIC_BARRIER))
    assert R.pair_separation(ref.mlp) >= 0.25
    swaps = (ref.mlp["z1"][:, :64] > ref.mlp["z1"][:, 64:]).mean(0)
    assert ((swaps > 0) & (swaps < 1)).sum() >= 32          # the larger unit of a pair depends on the row
    f, it = ops.dyn_eval(torch.from_numpy(h).to(dev), torch.from_numpy(x).to(dev), _wt(P, dev),
                         ops.DynCfg(scale_nominal=False, dropout=0.0, activation="GroupSort", **DYADIC_BARRIER),
                         rows_per_image=3)
    err = float(np.abs(f.cpu().numpy() - ref.f).max())
    print("dyadic dyn_eval: err", err, "exit", int(it.item()), ref.qp.iters)
    assert abs(int(it.item()) - ref.qp.iters) <= 1
    assert err <= 1e-5, err


# ---- 2. dyn_eval, random Cayley weights ----------------------------------------------------------
def _eval_case(scale_nominal):
    P = make_params(seed=9)
    rng = np.random.default_rng(10)
    x = rng.normal(size=(50, 10)).astype(np.float32)
    h = O.uniform_simplex(rng.exponential(1, (150, 10)).astype(np.float32))
    return P, x, h


@pytest.mark.parametrize("scale_nominal", [True, False])
def test_dyn_eval_matches_reference(scale_nominal):
    from fiode_amd import ops
    dev = _dev()
    P, x, h = _eval_case(scale_nominal)
    f, it = ops.dyn_eval(torch.from_numpy(h).to(dev), torch.from_numpy(x).to(dev), _wt(P, dev),
                         _gs(scale_nominal), rows_per_image=3)
    ref = O.eval_dot(h, np.repeat(O.static_projection(x, P), 3, 0), P, O.DynConfig(scale_nominal=scale_nominal))
    err = float(np.abs(f.cpu().numpy() - ref.f).max())
    print("dyn_eval: err", err, "exit", int(it.item()), ref.qp.iters)
    assert abs(int(it.item()) - ref.qp.iters) <= 1
    assert err <= 1e-3, err


# ---- 3 / 4. ODE solves ---------------------------------------------------------------------------
def _ode_setup(B, seed, scale_nominal):
    dev = _dev()
    P = make_params(seed=seed)
    rng = np.random.default_rng(seed + 1)
    x = rng.normal(size=(B, 10)).astype(np.float32)
    h0 = np.full((B, 10), 0.1, np.float32)
    return dev, P, x, h0, O.DynConfig(scale_nominal=scale_nominal), _wt(P, dev)


def _solve(dev, x, h0, times, w, scale_nominal, **kw):
    from fiode_amd import ops
    sol, st, _ = ops.odeint_dyn(torch.from_numpy(x).to(dev), torch.from_numpy(h0).to(dev),
                                torch.from_numpy(times.astype(np.float64)).to(dev), w, _gs(scale_nominal), **kw)
    torch.cuda.synchronize()
    return sol.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("B,scale_nominal", [(37, True), (128, False)])
def test_rk4_matches_reference(B, scale_nominal):
    """B=37: two full 16-row tiles and one of 5 rows.  Step 0.1 over [0, 1]: 10 steps, 40 evals."""
    dev, P, x, h0, cfg, w = _ode_setup(B, 10 + B, scale_nominal)
    times = O.linspace32(0.0, 1.0, 2)
    cnt = [0]
    ref, nsteps = O.rk4_fixed_grid(O.make_ode_func(x, P, cfg, cnt), h0, 0.0, 1.0, 0.1, times=times)
    sol, s = _solve(dev, x, h0, times, w, scale_nominal, method="rk4", step_size=0.1)
    err = float(np.abs(sol - ref).max())
    print("rk4: err", err, "stats", s)
    assert s[3] == 0 and s[1] == nsteps == 10 and s[0] == cnt[0] == 40
    assert err <= 2e-4, err
    assert np.allclose(sol[-1].sum(-1), 1.0, atol=1e-3)


# (B, scale_nominal, n_times) -> make_params seed.  Each seed was checked on the host: the reference's
# (nfe, n_accept, n_reject) is the same with the MLP output shifted by +2e-5 and by -2e-5
# (_groupsort_ref.mlp_forward_shifted), i.e. no accept / reject decision of its step sequence is
# borderline at the size of the device's rounding differences: seed 120 -> (44, 7, 0); 220, 320 and
# 420 -> (20, 3, 0), all three runs each; the shifted runs' states moved by <= 5.7e-5.
DOPRI5_SEEDS = {(64, True, 2): 120, (128, False, 2): 220, (1024, False, 2): 320, (96, False, 9): 420}


@pytest.mark.parametrize("B,scale_nominal,tol,n_times", [(64, True, 1e-3, 2), (128, False, 1e-3, 2),
                                                         (1024, False, 1e-3, 2), (96, False, 1e-3, 9)])
def test_dopri5_matches_reference(B, scale_nominal, tol, n_times):
    """Same steps as the reference (seeds: DOPRI5_SEEDS), states within 2e-4; n_times = 9: the dense
    output.  B=1024: 64 workgroups exchanging the QP exits and the error norm."""
    dev, P, x, h0, cfg, w = _ode_setup(B, DOPRI5_SEEDS[(B, scale_nominal, n_times)], scale_nominal)
    times = O.linspace32(0.0, 1.0, n_times)
    ref, st_ref = O.dopri5(O.make_ode_func(x, P, cfg), h0, 0.0, 1.0, rtol=tol, atol=tol, times=times)
    sol, s = _solve(dev, x, h0, times, w, scale_nominal, method="dopri5", rtol=tol, atol=tol)
    err = float(np.abs(sol - ref).max())
    print("dopri5: err", err, "stats", s, "ref", st_ref.nfe, st_ref.n_accept, st_ref.n_reject)
    assert s[3] == 0, s
    assert sol.shape == (n_times, B, 10)
    assert (s[0], s[1], s[2]) == (st_ref.nfe, st_ref.n_accept, st_ref.n_reject), (s[:3], st_ref)
    assert err <= 2e-4, err


# ---- 5. certification grid -----------------------------------------------------------------------
def _certify(P, x, T, label, scale_nominal):
    from fiode_amd import ops
    dev = _dev()
    vmax, vtmax = O.certify_image(x, label, O.db_grid_rows(10, T), P, O.DynConfig(scale_nominal=scale_nominal),
                                  O.CertifyConst(T=T, batches=10))
    out, _ = ops.certify_image(torch.from_numpy(x).to(dev), label, ops.certify_grid(T, device=dev), _wt(P, dev),
                               _gs(scale_nominal), T=T, batches=10)
    o = out.cpu().numpy()
    assert o.shape == (len(vmax), 2)
    return float(np.abs(o[:, 0] - vmax).max()), float(np.abs(o[:, 1] - vtmax).max())


@pytest.mark.parametrize("T,label,scale_nominal", [(8, 0, False), (12, 3, False), (12, 7, True)])
def test_certify_image_matches_reference(T, label, scale_nominal):
    x = np.random.default_rng(T).normal(size=10).astype(np.float32)
    err = _certify(make_params(seed=40 + T), x, T, label, scale_nominal)
    print("certify: err", err)
    assert max(err) <= 2e-3, err


def test_certify_image_dyadic_pairing():
    """The dyadic weights on the T=8 grid (eta a multiple of 1/8, entries <= 4/8 as dyadic_rows'):
    only the reported violations are exposed, so the bound is theirs (2e-3)."""
    x = np.zeros(10, np.float32)
    P = R.dyadic_params()
    eta = O.db_grid_for_label(O.db_grid_rows(10, 8), 2, 8)
    assert R.pair_separation(R.mlp_forward(eta, np.zeros((len(eta), 128), np.float32), P, None, None, 0.0)) >= 0.25
    err = _certify(P, x, 8, 2, False)
    print("certify dyadic: err", err)
    assert max(err) <= 2e-3, err


# ---- 6. ReLU untouched ---------------------------------------------------------------------------
def test_relu_act_entry_points_are_bit_identical():
    """fiode_dyn_eval_act / fiode_odeint_act with FIODE_ACT_RELU against fiode_dyn_eval / fiode_odeint."""
    from fiode_amd import ops, _lib as L
    dev = _dev()
    lib = L.lib()
    st = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P, x, h = _eval_case(True)
    for scale_nominal in (True, False):
        w = _wt(P, dev)
        cw = L.DynWeights(*[w[k].data_ptr() for k in ops.WEIGHT_KEYS])
        dc = ops.DynCfg(scale_nominal=scale_nominal, dropout=0.0).to_c()
        xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(h).to(dev)
        ws = torch.empty(lib.fiode_dyn_eval_workspace_bytes(150), dtype=torch.uint8, device=dev)
        f0, f1 = torch.empty_like(hd), torch.empty_like(hd)
        i0, i1 = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
        L.check(lib.fiode_dyn_eval(st, ct.byref(dc), ct.byref(cw), 50, 3, xd.data_ptr(), hd.data_ptr(), f0.data_ptr(),
                                   i0.data_ptr(), ws.data_ptr(), ws.numel()), "fiode_dyn_eval")
        L.check(lib.fiode_dyn_eval_act(st, ct.byref(dc), ct.byref(cw), 50, 3, xd.data_ptr(), hd.data_ptr(),
                                       f1.data_ptr(), i1.data_ptr(), ws.data_ptr(), ws.numel(), L.FIODE_ACT_RELU),
                "fiode_dyn_eval_act")
        torch.cuda.synchronize()
        assert torch.equal(f0, f1) and torch.equal(i0, i1)
    B = 37
    _, P, x, h0, _, w = _ode_setup(B, 10 + B, True)
    cw = L.DynWeights(*[w[k].data_ptr() for k in ops.WEIGHT_KEYS])
    dc = ops.DynCfg(scale_nominal=True, dropout=0.0).to_c()
    cfg = L.OdeConfig(L.FIODE_ODE_RK4, B, 2, 100000, 1e-3, 1e-3, 0.1)
    xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(h0).to(dev)
    times = torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev)
    ws = torch.empty(lib.fiode_odeint_workspace_bytes(B), dtype=torch.uint8, device=dev)
    outs = []
    for act in (None, L.FIODE_ACT_RELU):
        sol = torch.empty((2, B, 10), dtype=torch.float32, device=dev)
        stats = torch.zeros(8, dtype=torch.int32, device=dev)
        dst = torch.zeros(4, dtype=torch.float64, device=dev)
        args = (st, ct.byref(cfg), ct.byref(dc), ct.byref(cw), xd.data_ptr(), hd.data_ptr(), times.data_ptr(),
                sol.data_ptr(), stats.data_ptr(), dst.data_ptr(), ws.data_ptr(), ws.numel())
        L.check(lib.fiode_odeint(*args) if act is None else lib.fiode_odeint_act(*args, act), "fiode_odeint")
        torch.cuda.synchronize()
        outs.append((sol, stats))
    assert int(outs[0][1][3]) == 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- 7. through the modules ----------------------------------------------------------------------
def test_groupsort_module_forward_certify_and_training_refusal():
    from fiode_amd.certify import certify_lipschitz
    from tests.test_groupsort_dyn import build_module
    dev = _dev()
    mod = build_module("GroupSort").to(dev).eval()
    x = torch.rand(64, 3, 32, 32, device=dev)
    with torch.no_grad():
        out = mod(x)
    stats, _ = mod.dyn_fun.last_solve_stats
    assert out.shape == (64, 10) and torch.isfinite(out).all()
    assert torch.allclose(out.sum(-1), torch.ones(64, device=dev), atol=1e-3)
    assert int(stats[3]) == 0 and int(stats[0]) >= 8
    y = torch.tensor([1, 4, 9], device=dev)
    res = certify_lipschitz(mod, x[:3], y, T=12, batches=10)
    assert res.n_images == 3 and len(res.max_violations) == 3 and all(np.isfinite(res.max_violations))
    with torch.no_grad():
        ref = sum(int(int(mod(x[i:i + 1]).argmax(-1)) == int(y[i])) for i in range(3))
    assert res.correct == ref
    mod.train()
    with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
        mod.compute_loss(x, torch.randint(0, 10, (64,), device=dev))
