"""float64 reference of the input gradients of the fixed-grid RK4 (3/8 rule) solve of the eval-mode
dynamics (fiode_odeint_backward_x), for test_ode_backward_x.py.

``solve`` is the solve in float64 with the EXACT projection (tests/_dyn_grad_ref.f64_eval_dot);
``adjoint`` restates its reverse sweep: per step, from last to first, with a = dL/dy_{n+1}

    gk1 = gk4 = a dt / 8,  gk2 = gk3 = 3 a dt / 8,  dL/dy_n = a
    stage 4: gh = J(h4)^T gk4;  dL/dy_n += gh;  gk1 += dt gh;  gk2 -= dt gh;  gk3 += dt gh
    stage 3: gh = J(h3)^T gk3;  dL/dy_n += gh;  gk2 += dt gh;  gk1 -= dt gh / 3
    stage 2: gh = J(h2)^T gk2;  dL/dy_n += gh;  gk1 += dt gh / 3
    stage 1: gh = J(h1)^T gk1;  dL/dy_n += gh

for  h2 = y + dt k1 / 3,  h3 = y + dt (k2 - k1 / 3),  h4 = y + dt (k1 - k2 + k3),
y' = y + dt (k1 + 3 (k2 + k3) + k4) / 8  (torchdiffeq rk4_alt_step_func), and every evaluation's
gradient with respect to u = U_x x + bx + b1 summed per row: dL/dx = g_u Qx.

``vjp`` is the vector-Jacobian product of one evaluation with the exact projection's Jacobian: with
F the coordinates off their lower bound, g_nominal = (g - mean_F g) on F, g_lower = (g - mean_F g)
off F (barrier_projection.py:288-311 on the exact active set), then the barrier and the MLP.
"""
import numpy as np

from tests import _dyn_grad_ref as G


def grid(t0: float, t1: float, step: float) -> np.ndarray:
    """FixedGridODESolver's grid (_grid_constructor_from_step_size), float64."""
    n = int(np.ceil((t1 - t0) / step + 1.0))
    g = np.arange(n) * step + t0
    g[-1] = t1
    return g


def _weights(P):
    return {k: np.asarray(getattr(P, k), np.float64) for k in ("Q1", "b1", "Qx", "bx", "Q2", "b2", "Q3", "b3")}


def u_rows(x, P):
    W = _weights(P)
    return np.asarray(x, np.float64) @ W["Qx"].T + W["bx"]


def f(h, u, P, cfg, activation):
    """eval_dot in float64, exact projection.  Returns (f, margin): margin is the row's distance from
    a kink (QP active-set change, ReLU zero / GroupSort tie)."""
    v, qp_margin = G.f64_eval_dot(h, u, P, cfg, activation)
    W = _weights(P)
    z1 = h @ W["Q1"].T + W["b1"] + u
    z2 = G._act64(z1, activation) @ W["Q2"].T + W["b2"]
    m = []
    for z in (z1, z2):
        if activation == "GroupSort":
            k = z.shape[1] // 2
            m.append(np.abs(z[:, :k] - z[:, k:]).min(1))
        else:
            m.append(np.abs(z).min(1))
    return v, np.minimum(qp_margin, np.minimum(m[0], m[1]))


def _act_bwd(g, z, activation):
    if activation == "GroupSort":
        return G.groupsort_backward(g, z)
    return np.where(z > 0, g, 0.0)


def vjp(h, u, g, P, cfg, activation):
    """(g_h, g_u) of one evaluation for upstream g = dL/df, float64, exact active set."""
    W = _weights(P)
    z1 = h @ W["Q1"].T + W["b1"] + u
    a1 = G._act64(z1, activation)
    z2 = a1 @ W["Q2"].T + W["b2"]
    a2 = G._act64(z2, activation)
    ft = a2 @ W["Q3"].T + W["b3"]
    lower = -cfg.alpha_1 * (np.exp(cfg.sigma_1 * h) - 1.0)
    upper = cfg.alpha_2 * (1.0 - h)
    span = upper - lower
    if cfg.scale_nominal:
        sig = 1.0 / (1.0 + np.exp(-ft))
        nominal = span * sig + lower
    else:
        sig = None
        nominal = ft
    v, mu = G.exact_projection(lower, nominal)
    free = (nominal - mu[:, None]) > lower
    card = np.maximum(free.sum(1), 1)
    d = g - ((g * free).sum(1) / card)[:, None]
    g_nom = np.where(free, d, 0.0)
    g_low = np.where(free, 0.0, d)
    if cfg.scale_nominal:
        g_ft = g_nom * span * sig * (1.0 - sig)
        g_lower_tot = g_low + g_nom * (1.0 - sig)
        g_upper = g_nom * sig
    else:
        g_ft, g_lower_tot, g_upper = g_nom, g_low, np.zeros_like(g_nom)
    g_z2 = _act_bwd(g_ft @ W["Q3"], z2, activation)
    g_z1 = _act_bwd(g_z2 @ W["Q2"], z1, activation)
    dlow = -cfg.alpha_1 * cfg.sigma_1 * np.exp(cfg.sigma_1 * h)
    g_h = g_lower_tot * dlow + g_upper * (-cfg.alpha_2) + g_z1 @ W["Q1"]
    return g_h, g_z1


def _stage_inputs(y, k, dt):
    return (y, y + dt * k[0] / 3.0 if len(k) > 0 else None,
            y + dt * (k[1] - k[0] / 3.0) if len(k) > 1 else None,
            y + dt * (k[0] - k[1] + k[2]) if len(k) > 2 else None)


def solve(h0, x, P, cfg, activation, t0, t1, step):
    """Returns (y(t1), states [n_steps + 1, B, C], stage derivatives [n_steps, 4, B, C], margin [B])."""
    u = u_rows(x, P)
    tg = grid(t0, t1, step)
    y = np.asarray(h0, np.float64)
    states, ks = [y], []
    margin = np.full(y.shape[0], np.inf)
    for a, b in zip(tg[:-1], tg[1:]):
        dt = b - a
        k = []
        for s in range(4):
            v, m = f(_stage_inputs(y, k, dt)[s], u, P, cfg, activation)
            k.append(v)
            margin = np.minimum(margin, m)
        y = y + dt * (k[0] + 3.0 * (k[1] + k[2]) + k[3]) / 8.0
        states.append(y)
        ks.append(np.stack(k))
    return y, np.stack(states), np.stack(ks), margin


def adjoint(g_y, x, P, cfg, activation, t0, t1, step, states, ks):
    """(dL/dh0 [B, C], dL/dx [B, X]) from g_y = dL/dy(t1) and the solve's states / stage derivatives."""
    W = _weights(P)
    u = u_rows(x, P)
    tg = grid(t0, t1, step)
    a = np.asarray(g_y, np.float64)
    g_u = np.zeros_like(u)
    for n in range(len(tg) - 2, -1, -1):
        dt = tg[n + 1] - tg[n]
        y, k = states[n], list(ks[n])
        hs = _stage_inputs(y, k, dt)
        gk = [a * dt / 8.0, 3.0 * a * dt / 8.0, 3.0 * a * dt / 8.0, a * dt / 8.0]
        gy = a.copy()
        coef = {3: (dt, -dt, dt), 2: (-dt / 3.0, dt, 0.0), 1: (dt / 3.0, 0.0, 0.0), 0: (0.0, 0.0, 0.0)}
        for s in (3, 2, 1, 0):
            gh, gz1 = vjp(hs[s], u, gk[s], P, cfg, activation)
            g_u += gz1
            gy += gh
            for i in range(3):
                gk[i] = gk[i] + coef[s][i] * gh
        a = gy
    return a, g_u @ W["Qx"]
