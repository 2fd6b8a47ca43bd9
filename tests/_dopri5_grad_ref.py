"""float64 reference of the input gradients of the dopri5 inference solve on its accepted steps
(fiode_odeint_dopri5_backward_x), for test_dopri5_backward_x.py and test_gpu_dopri5_backward_x.py.
Built on tests/_ode_grad_ref.f / .vjp (one evaluation with the exact projection and its Jacobian).

``controller_solve`` is torchdiffeq 0.2.2's dopri5 controller in float64 (_select_initial_step,
the batch-global RMS error ratio, _optimal_step_size): it returns the accepted steps (t_n, dt_n) and the
number of rejected attempts.  ``solve_on_log`` takes such a log as CONSTANTS -- the step sizes carry no
gradient -- and runs the steps and the dense output at t1 inside the last one; the step size of the
stage sums is dt_n rounded to float32 and the abscissa x = (t1 - t_n) / ((t_n + dt_n) - t_n) comes from
the float64 times, as the device forms them.  ``adjoint_on_log`` restates the reverse sweep: per step,
from last to first, with a = dL/dy_{n+1}, beta the tableau and h_s = y + dt sum_{j<s} beta[s-1][j] k_j

    gy = a;  gk_j = dt beta[5][j] a  (j < 6)
    s = 5 .. 0:  gh = J(h_s)^T gk_s;  gy += gh;  gk_j += dt beta[s-1][j] gh  (j < s)

and in the last step, with g = dL/dy(t1) and the quartic's weights p0 (y), p1 (y1), pm (ymid), pa
(dt k1), pb (dt k7):  a = p1 g, gy = a + (p0 + pm) g, gk_j += dt cmid[j] pm g (j < 7), gk_0 += dt pa g,
gk_6 += dt pb g, the stage loop starting at s = 6 (k7 = f(y1), y1 = h_6).
"""
import numpy as np

from tests import _ode_grad_ref as R

BETA = [[1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9],
        [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
        [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
        [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
CERR = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720,
        -2187 / 6784 - -12231 / 42400, 11 / 84 - 649 / 6300, -1.0 / 60.0]
CMID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
        187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v))))


def _stage_input(y, k, s, dt):
    if s == 0:
        return y
    acc = np.zeros_like(y)
    for j in range(s):
        acc = acc + k[j] * (BETA[s - 1][j] * dt)
    return y + acc


def controller_solve(h0, x, P, cfg, activation, t0, t1, rtol, atol, max_steps=1000):
    """Returns (times [N], dts [N], n_reject): the accepted steps up to the first that reaches t1."""
    u = R.u_rows(x, P)
    F = lambda yy: R.f(yy, u, P, cfg, activation)[0]
    y = np.asarray(h0, np.float64)
    f0 = F(y)
    scale = atol + np.abs(y) * rtol
    d0, d1 = _rms(y / scale), _rms(f0 / scale)
    hh = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    f1 = F(y + hh * f0)
    d2 = _rms((f1 - f0) / scale) / hh
    h1 = max(1e-6, hh * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** 0.2
    dt = min(100 * hh, h1)
    tcur, fcur = float(t0), f0
    times, dts, n_reject = [], [], 0
    while t1 > tcur:
        assert len(times) + n_reject < max_steps
        k = [fcur]
        for s in range(1, 7):
            k.append(F(_stage_input(y, k, s, dt)))
        ynew = _stage_input(y, k, 6, dt)
        err = sum(k[j] * (CERR[j] * dt) for j in range(7))
        ratio = _rms(err / (atol + rtol * np.maximum(np.abs(y), np.abs(ynew))))
        if ratio <= 1:
            times.append(tcur)
            dts.append(dt)
            y, fcur, tcur = ynew, k[6], tcur + dt
        else:
            n_reject += 1
        dt = dt * 10.0 if ratio == 0 else dt * min(10.0, max(0.9 / ratio ** 0.2, 1.0 if ratio < 1 else 0.2))
    return np.array(times), np.array(dts), n_reject


def _step_dt(dt):
    return float(np.float32(dt))


def interp_weights(tn, dtn, t1):
    """(p0, p1, pm, pa, pb) of the dense output at t1 inside the step (tn, dtn)."""
    x = (t1 - tn) / ((tn + dtn) - tn)
    x2, x3, x4 = x * x, x ** 3, x ** 4
    return (1 - 11 * x2 + 18 * x3 - 8 * x4, -5 * x2 + 14 * x3 - 8 * x4, 16 * x2 - 32 * x3 + 16 * x4,
            x - 4 * x2 + 5 * x3 - 2 * x4, x2 - 3 * x3 + 2 * x4)


def solve_on_log(h0, x, P, cfg, activation, times, dts, t1):
    """Returns (y(t1), states [N, B, C], stage derivatives [N, 7, B, C], margin [B]) of the steps
    (times[n], dts[n]) held fixed; k7 is evaluated in the last step (elsewhere it is the next k1: zeros)."""
    u = R.u_rows(x, P)
    y = np.asarray(h0, np.float64)
    N = len(times)
    states, ks = [], []
    margin = np.full(y.shape[0], np.inf)
    out = None
    for n in range(N):
        dt = _step_dt(dts[n])
        k = []
        for s in range(7 if n == N - 1 else 6):
            v, m = R.f(_stage_input(y, k, s, dt), u, P, cfg, activation)
            k.append(v)
            margin = np.minimum(margin, m)
        y1 = _stage_input(y, k, 6, dt)
        states.append(y)
        if n == N - 1:
            p0, p1, pm, pa, pb = interp_weights(float(times[n]), float(dts[n]), float(t1))
            ym = y + sum(k[j] * (CMID[j] * dt) for j in range(7))
            out = p0 * y + p1 * y1 + pm * ym + pa * dt * k[0] + pb * dt * k[6]
        else:
            k.append(np.zeros_like(y))
        ks.append(np.stack(k))
        y = y1
    return out, np.stack(states), np.stack(ks), margin


def adjoint_on_log(g_y, x, P, cfg, activation, times, dts, t1, states, ks):
    """(dL/dh0 [B, C], dL/dx [B, X]) from g_y = dL/dy(t1) and solve_on_log's states / stage derivatives."""
    W = R._weights(P)
    u = R.u_rows(x, P)
    N = len(times)
    a = np.asarray(g_y, np.float64)
    g_u = np.zeros_like(u)
    for n in range(N - 1, -1, -1):
        dt = _step_dt(dts[n])
        y, k = states[n], list(ks[n])
        if n == N - 1:
            p0, p1, pm, pa, pb = interp_weights(float(times[n]), float(dts[n]), float(t1))
            g = a
            a = p1 * g
            gy = a + (p0 + pm) * g
            gk = [dt * BETA[5][j] * a + dt * CMID[j] * pm * g for j in range(6)]
            gk[0] = gk[0] + dt * pa * g
            gk.append(dt * pb * g + dt * CMID[6] * pm * g)
            top = 6
        else:
            gy = a.copy()
            gk = [dt * BETA[5][j] * a for j in range(6)]
            top = 5
        for s in range(top, -1, -1):
            gh, gz1 = R.vjp(_stage_input(y, k, s, dt), u, gk[s], P, cfg, activation)
            g_u += gz1
            gy = gy + gh
            for j in range(s):
                gk[j] = gk[j] + dt * BETA[s - 1][j] * gh
        a = gy
    return a, g_u @ W["Qx"]
