"""The selection conditions of tests/_ode_cases.py, on the reference alone (no device): every case the
device tests compare against is decided well away from the accept / reject threshold, keeps its step
sequence and moves by at most a quarter of the suite's 2e-4 when the MLP output is shifted by +-2e-5,
has the feature it is in the table for, and has the recorded step counts."""
import numpy as np
import pytest

from oracle import fiode_oracle as O
from tests import _ode_cases as K


def _moves(cid):
    ref, st = K.dopri5_ref(cid)
    out = []
    for d in (K.SHIFT, -K.SHIFT):
        r2, s2 = K.dopri5_ref(cid, d)
        out.append((K.seq_of(s2), float(np.abs(r2 - ref).max()) if r2.shape == ref.shape else np.inf))
    return out


@pytest.mark.parametrize("cid", list(K.DOPRI5_CASES))
def test_dopri5_case_meets_the_conditions(cid):
    c = K.DOPRI5_CASES[cid]
    P, x, h0 = K.case_inputs(cid)
    assert h0.shape == (c["B"], 10) and np.allclose(h0.sum(-1), 1.0, atol=1e-6)
    if c["kind"] == "vertex":
        assert ((h0 == 0).sum(-1) == 9).all() and (h0.max(-1) == 1).all()   # exact zeros reach the stepper
    ref, st = K.dopri5_ref(cid)
    seq = K.seq_of(st)
    ratios = [s[3] for s in st.steps]
    moves = _moves(cid)
    print(cid, (st.nfe, st.n_accept, st.n_reject), seq, "reject ratios",
          [round(r, 3) for r, s in zip(ratios, seq) if s == "R"], "moved", [m[1] for m in moves])
    assert np.isfinite(ref).all()
    # the recorded counts and sequence
    assert (st.nfe, st.n_accept, st.n_reject) == c["ref"]
    assert st.nfe == 2 + 6 * len(seq) and seq.count("A") == st.n_accept and seq.count("R") == st.n_reject
    if c["seq"] is not None:
        assert seq == c["seq"]
    # (a) no borderline decision
    assert not any(K.RATIO_BAND[0] <= r <= K.RATIO_BAND[1] for r in ratios), ratios
    # (b), (c) stable under the shifts
    for s2, moved in moves:
        assert s2 == seq
        assert moved <= K.MOVE_MAX, moved
    # (d) the feature
    if c["need"] == "reject":
        assert st.n_reject >= 1
    elif c["need"] == "double reject":
        assert "RR" in seq and float(K.case_times(c)[0]) != 0.0
    elif c["need"].startswith("swap"):
        assert c["rtol"] != c["atol"]
        refs, sts = K.dopri5_ref(cid, 0.0, True)
        assert sts.n_accept != st.n_accept
        assert float(np.abs(refs - ref).max()) > K.SWAP_MIN
        dt0 = K.initial_dt(cid)
        assert dt0 == st.steps[0][1]                    # the restatement is the reference's initial step
        moved = [abs(K.initial_dt(cid, *sw) - dt0) / dt0 for sw in ((True, False), (False, True))]
        print(cid, "first dt", dt0, "moves under a swap in the first / second expression alone", moved,
              "log tolerance", K.log_tolerance(cid))
        if c["need"] == "swap, initial step":
            # each expression of the initial step, swapped alone, moves the first dt ten times past what the
            # device's log is held to
            assert min(moved) > 10 * K.log_tolerance(cid), moved
    else:
        raise AssertionError(c["need"])


def test_max_steps_prefix_of_d1():
    """test_max_steps_reports_and_leaves_workspace_clean stops D1 after 4 attempts: AAAR."""
    assert K.seq_of(K.dopri5_ref("D1")[1])[:4] == "AAAR"


@pytest.mark.parametrize("cid,act", [("R1", "ReLU"), ("R2", "ReLU"), ("R3", "ReLU"), ("R4", "ReLU"),
                                     ("R1", "GroupSort"), ("R2", "GroupSort")])
def test_rk4_case_meets_the_conditions(cid, act):
    c = K.RK4_CASES[cid]
    ref, steps, nfe = K.rk4_ref(cid, act)
    t = K.rk4_times(cid)
    assert ref.shape == (len(t), K.RK4_B, 10) and np.isfinite(ref).all()
    assert steps == c["steps"] == len(O.rk4_grid(c["t0"], c["t1"], c["step"])) - 1 and nfe == 4 * steps
    moved = max(float(np.abs(K.rk4_ref(cid, act, d)[0] - ref).max()) for d in (K.SHIFT, -K.SHIFT))
    print(cid, act, "steps", steps, "moved", moved)
    assert moved <= K.MOVE_MAX, moved


def test_rk4_case_features():
    g1 = O.rk4_grid(0.0, 1.0, 0.3)
    t1 = K.rk4_times("R1")
    assert len(g1) == 5 and g1[3] != np.float32(0.9) and g1[4] == 1.0          # the snapped short last step
    assert ((t1 > g1[0]) & (t1 <= g1[1])).sum() == 2 and t1[2] == g1[1]        # two outputs in one step, one exact hit
    assert g1[3] < t1[4] < g1[4]                                               # an output inside the short step
    g2 = O.rk4_grid(0.25, 1.0, 0.1)
    t2 = K.rk4_times("R2")
    assert len(g2) == 9 and g2[-1] == 1.0 and np.float32(g2[-1] - g2[-2]) < np.float32(0.06)
    assert not np.isin(t2[1:-1], g2).any()                                     # interior outputs all interpolated
    assert len(O.rk4_grid(0.0, 0.5, 2.0)) == 2                                 # a step longer than the interval
    # R4: the grid's prefixes up to g_k are the grids of [t0, g_k] for k = 1..7 (not for the snapped end)
    for k in range(1, 8):
        assert np.array_equal(O.rk4_grid(0.25, float(g2[k]), 0.1), g2[:k + 1]), k
    # and the step states over the grid are what the fixed-grid solve returns at those times
    P, x, h0 = K.case_inputs("R4")
    on_grid = K.rk4_ref("R4")[0]
    fixed, n = O.rk4_fixed_grid(O.make_ode_func(x, P, O.DynConfig(scale_nominal=False)), h0, 0.25, 1.0, 0.1, times=g2)
    assert n == 8 and np.array_equal(fixed, on_grid)
