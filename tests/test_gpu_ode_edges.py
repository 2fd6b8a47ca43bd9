"""GPU parity of the HIP ODE solves (fiode_odeint_act, csrc/odesolve.hip) on the parts of the stepper
that tests/test_gpu_ode.py and tests/test_gpu_groupsort_dyn.py do not reach: rejected dopri5 attempts
(one workgroup and eight), rtol != atol, one-hot initial states (exact zeros), t0 != 0, rk4 output times
off the grid, the grid itself as output times, and status 2 (max_steps).

The cases, and why each is a fair comparison with the oracle's torchdiffeq restatement
(oracle/fiode_oracle.py dopri5 / rk4_fixed_grid / rk4_on_grid), are in tests/_ode_cases.py; the
conditions that select them are asserted on the host by tests/test_ode_cases.py.  States: 2e-4 absolute,
the suite's bound (test_gpu_ode.py's header); the cases move by <= 5e-5 under an MLP-output shift of
2e-5.  The logged (t_n, dt_n) of the accepted steps are compared with the oracle's under a relative
tolerance taken from the reference itself: 4x their largest relative move under that shift, floored at
1e-6 (dt follows ratio^(-1/5), so it is not bit-comparable).
"""
import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _ode_cases as K

pytestmark = pytest.mark.gpu

LOG_CAP = 16


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


def _wt(P, dev):
    from fiode_amd import ops
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}


def _dyn(act, scale_nominal):
    from fiode_amd import ops
    return ops.DynCfg(scale_nominal=scale_nominal, dropout=0.0, activation=act)


def _solve(dev, cid, act, scale_nominal, times, h0=None, **kw):
    """ops.odeint_dyn on the inputs of case ``cid`` (``h0``: another initial state); returns host arrays
    (sol, stats, dstats[, log times, log states])."""
    from fiode_amd import ops
    P, x, h0_case = K.case_inputs(cid)
    h0 = h0_case if h0 is None else h0
    out = ops.odeint_dyn(torch.from_numpy(x.copy()).to(dev), torch.from_numpy(h0.copy()).to(dev),
                         torch.from_numpy(np.asarray(times, np.float64)).to(dev), _wt(P, dev),
                         _dyn(act, scale_nominal), **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _dopri5(dev, cid, **kw):
    c = K.DOPRI5_CASES[cid]
    return _solve(dev, cid, c["act"], c["scale_nominal"], K.case_times(c), method="dopri5", rtol=c["rtol"],
                  atol=c["atol"], **kw)


def _check_dopri5(dev, cid):
    """The assertions shared by the dopri5 cases; returns the plain call's (sol, stats)."""
    c = K.DOPRI5_CASES[cid]
    ref, st_ref = K.dopri5_ref(cid)
    times = K.case_times(c)
    sol, s, ds = _dopri5(dev, cid)
    err = float(np.abs(sol - ref).max())
    print(f"{cid}: stats {s.tolist()} oracle {(st_ref.nfe, st_ref.n_accept, st_ref.n_reject)} state err {err:.3e}")
    assert s[3] == 0, s
    assert sol.shape == ref.shape == (len(times), c["B"], 10)
    assert (s[0], s[1], s[2]) == (st_ref.nfe, st_ref.n_accept, st_ref.n_reject) == c["ref"], (s, c["ref"])
    assert s[5] == st_ref.n_accept + st_ref.n_reject
    assert err <= K.TOL, err
    # the same solve with the step log: bit-equal, and the accepted steps are the oracle's
    sol_l, s_l, ds_l, lt, _ = _dopri5(dev, cid, log_steps=LOG_CAP)
    assert np.array_equal(sol_l, sol) and np.array_equal(s_l, s) and np.array_equal(ds_l, ds)
    n = st_ref.n_accept
    assert n <= LOG_CAP
    steps_ref = K.accepted_steps(st_ref)
    rtol = K.log_tolerance(cid)
    d_log = K.rel_diff(lt[:n], steps_ref)
    tend_ref = K.dopri5_final_t(st_ref)
    d_end = K.rel_diff(ds[1], tend_ref)
    rel_each = np.abs(lt[:n] - steps_ref) / np.maximum(np.abs(steps_ref), 1e-300)
    print(f"{cid}: per accepted step, rel diff of (t_n, dt_n):", np.array2string(rel_each, precision=2).replace("\n", ""))
    print(f"{cid}: logged (t_n, dt_n) vs oracle: rel {d_log:.3e}, time reached {ds[1]!r} vs {tend_ref!r}: rel "
          f"{d_end:.3e}; tolerance {rtol:.3e}")
    assert np.all(lt[n:] == 0.0)                                  # nothing past the accepted steps
    assert lt[0, 0] == float(times[0])
    assert np.all(lt[1:n, 0] == lt[:n - 1, 0] + lt[:n - 1, 1])    # t_{n+1} = t_n + dt_n exactly, in float64
    assert d_log <= rtol, (d_log, rtol)
    assert ds[1] >= float(times[-1])
    assert ds[1] == lt[n - 1, 0] + lt[n - 1, 1]
    assert d_end <= rtol, (d_end, rtol)
    return sol, s


@pytest.mark.parametrize("cid", ["D1", "D2", "D3", "D4", "D5", "D6"])
def test_dopri5_rejects_match_oracle(cid):
    """Solves whose controller rejects an attempt (D6: two in a row, t0 = 0.25) from one-hot states:
    the same NFE / accepted / rejected counts as the oracle, states within 2e-4, the accepted steps'
    (t_n, dt_n) and the time reached those of the oracle.  B=37: three workgroups, the last with 5
    rows; B=128: eight workgroups take the reject decision from the exchanged error norm."""
    dev = _dev()
    sol, s = _check_dopri5(dev, cid)
    assert s[2] >= 1
    assert np.array_equal(sol[0], K.case_inputs(cid)[2])


@pytest.mark.parametrize("cid", ["D7", "D8"])
def test_dopri5_rtol_differs_from_atol(cid):
    """rtol != atol (D7: 1e-4 / 1e-6, D8: 1e-6 / 1e-4): a solve that used one for the other takes other
    steps -- the oracle with the two swapped accepts another number of steps and ends > 5e-4 away.  The
    three places that form atol + rtol |y| (the scale of the initial step's d0 and d1, that of its d2, the
    error ratio's) are each visible in D8, through the first logged dt and the step counts; D7's first dt
    does not depend on the second."""
    dev = _dev()
    sol, s = _check_dopri5(dev, cid)
    ref_sw, st_sw = K.dopri5_ref(cid, 0.0, True)
    d_sw = float(np.abs(sol - ref_sw).max())
    print(f"{cid}: swapped-tolerance oracle accepts {st_sw.n_accept}, device is {d_sw:.3e} from it")
    assert s[1] != st_sw.n_accept
    assert d_sw > K.SWAP_MIN, d_sw


@pytest.mark.parametrize("cid,act", [("R1", "ReLU"), ("R2", "ReLU"), ("R3", "ReLU"), ("R1", "GroupSort"),
                                     ("R2", "GroupSort")])
def test_rk4_off_grid_outputs(cid, act):
    """Output times between the grid points (linear interpolation), several in one step, an exact grid
    hit, one inside the snapped short last step (R1); t0 != 0 (R2); a step longer than the interval (R3)."""
    dev = _dev()
    c = K.RK4_CASES[cid]
    ref, steps, nfe = K.rk4_ref(cid, act)
    sol, s, _ = _solve(dev, cid, act, False, K.rk4_times(cid), method="rk4", step_size=c["step"])
    err = float(np.abs(sol - ref).max())
    print(f"{cid} {act}: stats {s.tolist()} oracle steps {steps} state err {err:.3e}")
    assert s[3] == 0, s
    assert s[1] == steps == c["steps"] and s[0] == nfe == 4 * steps
    assert sol.shape == ref.shape
    assert err <= K.TOL, err
    assert np.array_equal(sol[0], K.case_inputs(cid)[2])


def test_rk4_grid_outputs_are_step_states():
    """ops.rk4_grid's promise (odeint_backward_x relies on it), with t0 != 0: asked for as output times,
    the grid returns the step states -- output k is, bit for bit, the end state of the solve over
    [t0, g_k] wherever that solve's grid is the prefix g_0..g_k (k = 1..7; the last point is snapped to
    t1, and is compared with the [t0, t1] solve)."""
    from fiode_amd import ops
    dev = _dev()
    c = K.RK4_CASES["R4"]
    t0, t1, hs = c["t0"], c["t1"], c["step"]
    grid = ops.rk4_grid(t0, t1, hs)
    g_ref = O.rk4_grid(t0, t1, hs)
    assert grid.dtype == np.float64 and np.array_equal(grid, g_ref.astype(np.float64))
    assert len(grid) == 9
    ref, steps, nfe = K.rk4_ref("R4")
    sol, s, _ = _solve(dev, "R4", "ReLU", False, grid, method="rk4", step_size=hs)
    err = float(np.abs(sol - ref).max())
    print(f"R4: stats {s.tolist()} state err {err:.3e}")
    assert s[3] == 0 and s[1] == steps == 8 and s[0] == nfe == 32, s
    assert sol.shape == (9, K.RK4_B, 10)
    assert err <= K.TOL, err
    assert np.array_equal(sol[0], K.case_inputs("R4")[2])
    for k in range(1, 9):
        if k < 8:
            assert np.array_equal(O.rk4_grid(t0, float(g_ref[k]), hs), g_ref[:k + 1])
        end, sk, _ = _solve(dev, "R4", "ReLU", False, np.array([grid[0], grid[k]]), method="rk4", step_size=hs)
        assert sk[3] == 0 and sk[1] == k, (k, sk)
        assert np.array_equal(end[-1], sol[k]), (k, float(np.abs(end[-1] - sol[k]).max()))
    # Both sides of that comparison pass through the same output expression, so also: output k is the state
    # step k starts from.  One rk4 step from sol[k] over [g_k, g_k+1] (a step size longer than the interval:
    # dt = g_k+1 - g_k, the solve's own; the dynamics do not depend on t, and an eval's result does not depend
    # on the evals before it) ends in sol[k+1], bit for bit.  (What this cannot tell apart is an end-of-step
    # output that is interpolated instead of copied: y + 1 * (y' - y) is y' exactly wherever y' - y is exact in
    # float32, which is every entry of these simplex trajectories.)
    for k in (1, 4, 7):
        end, sk, _ = _solve(dev, "R4", "ReLU", False, np.array([grid[k], grid[k + 1]]), h0=sol[k], method="rk4",
                            step_size=1.0)
        assert sk[3] == 0 and sk[1] == 1, (k, sk)
        assert np.array_equal(end[0], sol[k])
        assert np.array_equal(end[1], sol[k + 1]), (k, float(np.abs(end[1] - sol[k + 1]).max()))


def test_max_steps_reports_and_leaves_workspace_clean():
    """D1 (attempts AAARA) stopped after 4: every workgroup returns at the same attempt with status 2,
    the counts are those of AAAR, and the next solve on the same cached workspace is the full D1."""
    from fiode_amd.dynamics import OrthoClassDynProjectSimplexLips
    from fiode_amd.odeint import odeint
    dev = _dev()
    assert K.seq_of(K.dopri5_ref("D1")[1])[:4] == "AAAR"
    sol, s, ds = _dopri5(dev, "D1", max_steps=4)
    print("D1, max_steps=4: stats", s.tolist())
    assert s[3] == 2, s
    assert s[5] == 4
    assert (s[0], s[1], s[2]) == (26, 3, 1), s
    assert np.array_equal(sol[0], K.case_inputs("D1")[2])
    _check_dopri5(dev, "D1")
    # through the front end
    P, x, h0 = K.case_inputs("D1")
    torch.manual_seed(0)
    dyn = OrthoClassDynProjectSimplexLips(n_hidden=10, activation="ReLU", dropout=0.5, mlp_size=128, kappa=2.0,
                                          kappa_length=0, alpha_1=100.0, alpha_2=20.0, sigma_1=0.02,
                                          scale_nominal=False, x_dim=10, cayley=True).to(dev).eval()
    dyn.static_state = torch.from_numpy(x.copy()).to(dev)
    t = torch.from_numpy(K.case_times(K.DOPRI5_CASES["D1"])).to(dev)
    with pytest.raises(RuntimeError, match="max_num_steps exceeded"):
        odeint(dyn.ode_forward, (torch.from_numpy(h0.copy()).to(dev),), t, method="dopri5",
               options=dict(max_num_steps=4))       # odeint's default tolerances (1e-7, 1e-9): far more than 4 attempts
    st = dyn.last_solve_stats[0].cpu().numpy()
    assert st[3] == 2 and st[5] == 4 and st[1] + st[2] == 4, st
