"""Inputs, case table and shifted reference for the ODE-solve edge tests (tests/test_ode_cases.py on
the host, tests/test_gpu_ode_edges.py on the device).

The device and the reference run the same float32 solver arithmetic and differ in the MLP's
accumulation order.  A case is only a fair comparison of the step controller if that difference cannot
change an accept / reject decision, and only fits the suite's 2e-4 (test_gpu_ode.py's header) if the
trajectory is not too sensitive to it.  So every dopri5 case here meets, on the reference alone
(asserted by tests/test_ode_cases.py):

  (a) no attempt's error ratio (Dopri5Stats.steps[i][3]) lies in RATIO_BAND = [0.8, 1.25];
  (b) the accept / reject sequence is the same with the MLP output shifted by +SHIFT and by -SHIFT
      (2e-5, the shifts of test_gpu_groupsort_dyn.py's seed check, far above the device's rounding);
  (c) under those shifts the output states move by at most MOVE_MAX = 5e-5, a quarter of 2e-4;
  (d) the case has the feature it is in the table for (``need``).

rk4 cases take no decisions and need (c) only.

Inputs that do NOT meet the conditions (do not use): seed 1 vertex (AAARRRA) moves 1.2e-3 under the
shift, the edge seeds 2-4 move 5e-4 to 7e-4.
"""
import functools

import numpy as np

from oracle import fiode_oracle as O
from tests import _groupsort_ref as G
from tests._util import make_params

SHIFT = 2e-5
RATIO_BAND = (0.8, 1.25)
MOVE_MAX = 5e-5
TOL = 2e-4                      # the suite's bound on the states (test_gpu_ode.py's header)

_RELU_MLP = O.mlp_forward       # taken at import, before any test installs another MLP


def inputs(B, seed, kind):
    """(P, x, h0): ``vertex`` rows are one-hot, ``edge`` rows hold two 0.5 (exact zeros, where the
    barrier bound is 0), ``simplex`` rows are uniform on the simplex."""
    P = make_params(seed=seed)
    rng = np.random.default_rng(seed + 1)
    x = rng.normal(size=(B, 10)).astype(np.float32)
    if kind == "vertex":
        h0 = np.zeros((B, 10), np.float32)
        h0[np.arange(B), rng.integers(0, 10, B)] = 1.0
    elif kind == "edge":
        h0 = np.zeros((B, 10), np.float32)
        i = rng.integers(0, 10, B)
        j = (i + 1 + rng.integers(0, 9, B)) % 10
        h0[np.arange(B), i] = 0.5
        h0[np.arange(B), j] = 0.5
    elif kind == "simplex":
        h0 = O.uniform_simplex(rng.exponential(1, (B, 10)).astype(np.float32))
    else:
        raise ValueError(kind)
    return P, x, h0


def _relu_shifted(delta):
    def f(h, u_rows, P, mask1, mask2, p):
        out = _RELU_MLP(h, u_rows, P, mask1, mask2, p)
        out["ftilde"] = (out["ftilde"] + np.float32(delta)).astype(np.float32)
        return out
    return f


def _mlp(act, delta):
    if act == "ReLU":
        return _RELU_MLP if delta == 0.0 else _relu_shifted(delta)
    if act == "GroupSort":
        return G.mlp_forward if delta == 0.0 else G.mlp_forward_shifted(delta)
    raise ValueError(act)


def with_mlp(act, delta, fn):
    """fn() with the oracle's MLP replaced by ``act``'s, its output ftilde shifted by ``delta``."""
    saved = O.mlp_forward
    O.mlp_forward = _mlp(act, delta)
    try:
        return fn()
    finally:
        O.mlp_forward = saved


_T = (0.0, 0.3, 0.55, 1.0)

# id -> case.  ``ref`` = the reference's (nfe, accepted, rejected), ``seq`` its attempts in order (A an
# accepted step, R a rejected one), as measured on the host; the comment gives the rejected attempts'
# error ratios and the largest move of the output states under +-SHIFT.  All seeds are the first choice
# (no case had to move to another seed).
DOPRI5_CASES = {
    # one reject, one 16-row tile short of three: ratio 2.96, moved 2.2e-5
    "D1": dict(act="ReLU", B=37, kind="vertex", scale_nominal=False, rtol=1e-5, atol=1e-5, seed=2, times=_T,
               ref=(32, 4, 1), seq="AAARA", need="reject"),
    # the same over 8 workgroups that exchange the error norm: ratio 5.23, moved 2.2e-5
    "D2": dict(act="ReLU", B=128, kind="vertex", scale_nominal=False, rtol=1e-5, atol=1e-5, seed=4, times=_T,
               ref=(32, 4, 1), seq="AAARA", need="reject"),
    # scale_nominal, 13 attempts: ratio 2.23, moved 1.6e-5
    "D3": dict(act="ReLU", B=128, kind="vertex", scale_nominal=True, rtol=1e-5, atol=1e-5, seed=4, times=_T,
               ref=(80, 12, 1), seq="AAAAAAAAARAAA", need="reject"),
    # ratio 2.10, moved 3.5e-5
    "D4": dict(act="ReLU", B=37, kind="vertex", scale_nominal=True, rtol=1e-5, atol=1e-5, seed=4, times=_T,
               ref=(80, 12, 1), seq="AAAAAAAAARAAA", need="reject"),
    # GroupSort: ratio 1.35, moved 7e-6
    "D5": dict(act="GroupSort", B=128, kind="vertex", scale_nominal=True, rtol=1e-5, atol=1e-5, seed=4, times=_T,
               ref=(86, 13, 1), seq="AAAAAAAAARAAAA", need="reject"),
    # two rejections in a row and t0 != 0: ratios 2.83, 1.91, moved 1.9e-5
    "D6": dict(act="ReLU", B=37, kind="vertex", scale_nominal=False, rtol=1e-5, atol=1e-5, seed=26,
               times=(0.25, 0.3, 0.55, 1.25), ref=(38, 4, 2), seq="AAARRA", need="double reject"),
    # rtol != atol: with the two swapped the reference takes 4 accepted steps and ends 1.8e-3 away
    "D7": dict(act="ReLU", B=37, kind="simplex", scale_nominal=False, rtol=1e-4, atol=1e-6, seed=17, times=_T,
               ref=(38, 6, 0), seq="AAAAAA", need="swap"),
    # rtol != atol where the SECOND tolerance expression of the initial step decides it.  D7's first dt is the
    # same whether or not that expression (the scale of d2 = |f1 - f0| / h0) has the two swapped, so D7 alone
    # cannot see a swap there; here each of the three expressions, swapped alone, changes the first dt by far
    # more than the log tolerance (asserted for the two of the initial step by test_ode_cases.py; swapped in
    # the error ratio alone the reference accepts 12 steps).  atol > rtol, the other order than D7.  Added to
    # the issue's table after that finding.  Moved 6e-6.
    "D8": dict(act="ReLU", B=37, kind="simplex", scale_nominal=True, rtol=1e-6, atol=1e-4, seed=4, times=_T,
               ref=(50, 8, 0), seq="AAAAAAAA", need="swap, initial step"),
}
SWAP_MIN = 5e-4                 # D7: the swapped-tolerance reference is further than this from the true one

# id -> case: 37 rows, seed 2, scale_nominal off.  ``steps`` = the reference's step count (nfe = 4 steps).
RK4_CASES = {
    # grid [0, .3, .6, .90000004, 1]: two outputs inside the first step, an exact grid hit (0.3), one
    # output inside the snapped short last step
    "R1": dict(kind="simplex", t0=0.0, t1=1.0, step=0.3, times=(0.0, 0.1, 0.3, 0.45, 0.95, 1.0), steps=4),
    # t0 != 0; 0.26 inside the first step; last step 0.95 -> 1.0
    "R2": dict(kind="simplex", t0=0.25, t1=1.0, step=0.1, times=(0.25, 0.26, 0.5, 0.77, 1.0), steps=8),
    # a step longer than the interval: one step of 0.5
    "R3": dict(kind="simplex", t0=0.0, t1=0.5, step=2.0, times=(0.0, 0.2, 0.5), steps=1),
    # the grid itself as output times: the step states
    "R4": dict(kind="vertex", t0=0.25, t1=1.0, step=0.1, times="grid", steps=8),
}
RK4_B, RK4_SEED = 37, 2


def seq_of(st):
    return "".join("A" if s[2] else "R" for s in st.steps)


def case_times(c):
    return np.asarray(c["times"], np.float32)


@functools.lru_cache(maxsize=None)
def case_inputs(cid):
    if cid in DOPRI5_CASES:
        c = DOPRI5_CASES[cid]
        out = inputs(c["B"], c["seed"], c["kind"])
    else:
        out = inputs(RK4_B, RK4_SEED, RK4_CASES[cid]["kind"])
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dopri5_ref(cid, delta=0.0, swap=False):
    """(states [T,B,C], Dopri5Stats) of the reference on case ``cid``, the MLP output shifted by
    ``delta``; ``swap``: rtol and atol exchanged.  Computed once; the arrays are read-only."""
    c = DOPRI5_CASES[cid]
    P, x, h0 = case_inputs(cid)
    t = case_times(c)
    rtol, atol = (c["atol"], c["rtol"]) if swap else (c["rtol"], c["atol"])
    cfg = O.DynConfig(scale_nominal=c["scale_nominal"])
    ref, st = with_mlp(c["act"], delta, lambda: O.dopri5(O.make_ode_func(x, P, cfg), h0, float(t[0]), float(t[-1]),
                                                         rtol=rtol, atol=atol, times=t))
    ref.setflags(write=False)
    return ref, st


def dopri5_final_t(st):
    """The time the reference's controller has reached after its last attempt."""
    t, dt = [(s[0], s[1]) for s in st.steps if s[2]][-1]
    return t + dt


def accepted_steps(st):
    """float64 [n_accept, 2]: (t_n, dt_n) of the accepted steps."""
    return np.array([(s[0], s[1]) for s in st.steps if s[2]], np.float64)


def log_tolerance(cid):
    """Relative tolerance for the device's accepted (t_n, dt_n) and the time it reached, from the reference
    alone: 4x the largest relative move of those values under +-SHIFT, floored at 1e-6."""
    st = dopri5_ref(cid)[1]
    steps, tend = accepted_steps(st), dopri5_final_t(st)
    move = 0.0
    for d in (SHIFT, -SHIFT):
        s2 = dopri5_ref(cid, d)[1]
        assert seq_of(s2) == seq_of(st)
        move = max(move, rel_diff(accepted_steps(s2), steps), rel_diff(dopri5_final_t(s2), tend))
    return max(4.0 * move, 1e-6)


def rel_diff(a, ref):
    """Largest |a - ref| / |ref|; entries where ref == 0 must be equal (inf otherwise)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    z = ref == 0
    if np.any(a[z] != 0):
        return np.inf
    return float((np.abs(a - ref)[~z] / np.abs(ref)[~z]).max()) if (~z).any() else 0.0


def initial_dt(cid, swap_first=False, swap_second=False):
    """The first step size of case ``cid``: O.dopri5's _select_initial_step restated with the tolerance
    expression of d0 and d1 (``swap_first``) and that of d2 (``swap_second``) taking rtol for atol and
    atol for rtol when asked.  Unswapped it is the reference's first dt, bit for bit (asserted)."""
    c = DOPRI5_CASES[cid]
    P, x, y = case_inputs(cid)
    F32 = np.float32
    rtol, atol = F32(c["rtol"]), F32(c["atol"])
    t0 = float(case_times(c)[0])

    def run():
        func = O.make_ode_func(x, P, O.DynConfig(scale_nominal=c["scale_nominal"]))
        sc = [(b + np.abs(y) * a).astype(F32) if sw else (a + np.abs(y) * b).astype(F32)
              for sw, a, b in ((swap_first, atol, rtol), (swap_second, atol, rtol))]
        f0 = func(t0, y)
        d0, d1 = O.rms_norm(y / sc[0]), O.rms_norm(f0 / sc[0])
        h0 = F32(1e-6) if d0 < 1e-5 or d1 < 1e-5 else F32(F32(0.01) * d0 / d1)
        f1 = func(t0 + float(h0), (y + h0 * f0).astype(F32))
        d2 = F32(O.rms_norm((f1 - f0).astype(F32) / sc[1]) / h0)
        if d1 <= 1e-15 and d2 <= 1e-15:
            h1 = max(F32(1e-6), F32(h0 * F32(1e-3)))
        else:
            h1 = F32(F32(0.01) / max(d1, d2)) ** F32(1.0 / 5.0)
        return float(min(F32(100) * h0, F32(h1)))
    return with_mlp(c["act"], 0.0, run)


def rk4_times(cid):
    c = RK4_CASES[cid]
    if isinstance(c["times"], str):
        return O.rk4_grid(c["t0"], c["t1"], c["step"])
    return np.asarray(c["times"], np.float32)


@functools.lru_cache(maxsize=None)
def rk4_ref(cid, act="ReLU", delta=0.0):
    """(states at the case's output times, steps, nfe) of the reference's fixed-grid solve (R4: of
    rk4_on_grid over the grid, the step states)."""
    c = RK4_CASES[cid]
    P, x, h0 = case_inputs(cid)
    cfg = O.DynConfig(scale_nominal=False)
    t = rk4_times(cid)
    cnt = [0]

    def run():
        f = O.make_ode_func(x, P, cfg, cnt)
        if isinstance(c["times"], str):
            return O.rk4_on_grid(f, h0, t), len(t) - 1
        return O.rk4_fixed_grid(f, h0, c["t0"], c["t1"], c["step"], times=t)
    ref, steps = with_mlp(act, delta, run)
    ref.setflags(write=False)
    return ref, steps, cnt[0]
