"""Reference of the eval_dot backward (fiode_dyn_eval_backward) for test_dyn_backward.py and
test_gpu_dyn_backward.py, composed from the oracle's own pieces:

  O.static_projection, O.mlp_forward (ReLU) or tests/_groupsort_ref.mlp_forward (GroupSort),
  O.barrier_lower / O.barrier_upper / O.sigmoid32, O.qp_run_fixed(lower, nominal, K) for (v, mu),
  O.qp_backward, and O.mlp_backward (ReLU) or ``mlp_backward_groupsort`` below (ties split in half).

With (g_nom, g_low) from the QP backward, per row and coordinate j

  g_ft[j]        = scale_nominal ? g_nom[j] span[j] sig[j] (1 - sig[j]) : g_nom[j]
  g_lower_tot[j] = g_low[j] + (scale_nominal ? g_nom[j] (1 - sig[j]) : 0)
  g_upper[j]     = scale_nominal ? g_nom[j] sig[j] : 0
  g_h[j]         = g_lower_tot[j] (-alpha_1 sigma_1 exp(sigma_1 h[j])) + g_upper[j] (-alpha_2) + (Q1^T g_z1)[j]

``f64_eval_dot`` is a float64 restatement of eval_dot with the EXACT projection (multiplier bisected
to 1e-14) for the finite-difference check of this composition.
"""
import numpy as np

from oracle import fiode_oracle as O
from tests import _groupsort_ref as R

F32 = np.float32
KEYS = ("Q1", "b1", "Qx", "bx", "Q2", "b2", "Q3", "b3", "x_feat")


def groupsort_backward(g_out: np.ndarray, z: np.ndarray) -> np.ndarray:
    """d/dz of cat(max(a, b), min(a, b)), a = z[:, :m], b = z[:, m:]; a tie gives both members
    (g_max + g_min) / 2 (torch.maximum / torch.minimum)."""
    m = z.shape[1] // 2
    a, b = z[:, :m], z[:, m:]
    gmx, gmn = g_out[:, :m], g_out[:, m:]
    tie = (gmx + gmn) / 2.0
    ga = np.where(a == b, tie, np.where(a > b, gmx, gmn))
    gb = np.where(a == b, tie, np.where(a > b, gmn, gmx))
    return np.concatenate([ga, gb], axis=1)


def mlp_backward_groupsort(g_ft, h, x_feat, S, P, mlp):
    """O.mlp_backward for the GroupSort MLP of tests/_groupsort_ref.mlp_forward (float64 sums)."""
    g3 = np.asarray(g_ft, np.float64)
    a1 = mlp["a1"].astype(np.float64)
    a2 = mlp["a2"].astype(np.float64)
    out = {}
    out["Q3"] = g3.T @ a2
    out["b3"] = g3.sum(0)
    g_z2 = groupsort_backward(g3 @ P.Q3.astype(np.float64), mlp["z2"])
    out["Q2"] = g_z2.T @ a1
    out["b2"] = g_z2.sum(0)
    g_z1 = groupsort_backward(g_z2 @ P.Q2.astype(np.float64), mlp["z1"])
    out["Q1"] = g_z1.T @ np.asarray(h, np.float64)
    out["b1"] = g_z1.sum(0)
    B = x_feat.shape[0]
    g_u = g_z1.reshape(B, S, -1).sum(1)
    out["Qx"] = g_u.T @ np.asarray(x_feat, np.float64)
    out["bx"] = g_u.sum(0)
    out["x_feat"] = g_u @ P.Qx.astype(np.float64)
    out["g_u"] = g_u
    out = {k: v.astype(F32) for k, v in out.items()}
    out["g_z1"] = g_z1
    return out


def preact_margin(mlp, activation: str) -> np.ndarray:
    """Per row: min |z| over both hidden layers (ReLU), min pair gap |z[u] - z[u + 64]| (GroupSort)."""
    d = []
    for z in (mlp["z1"], mlp["z2"]):
        z = z.astype(np.float64)
        if activation == "GroupSort":
            m = z.shape[1] // 2
            d.append(np.abs(z[:, :m] - z[:, m:]).min(1))
        else:
            d.append(np.abs(z).min(1))
    return np.minimum(d[0], d[1])


def eval_dot_backward(g_f, h, x_feat, S, P, cfg, activation="ReLU", qp_inputs=None, K=None, bound_active=False):
    """Returns a dict: g_h [N, C]; Q1 .. b3, x_feat as O.mlp_backward; margin [N] (preact_margin);
    and the intermediates f, mu, K, lower, nominal, g_ft, g_z1.  ``qp_inputs`` pins the QP's (lower,
    nominal) to another implementation's float32 values (O.eval_dot: why); ``K``: the exit iteration
    (None: the batch-global exit of O.qp_forward on the QP inputs).

    ``bound_active``: O.qp_backward decides the active set as the reference does, by the sign of
    (v - nominal) + mu, which for a coordinate off its bound is the float32 rounding residue of
    nominal - mu (DESIGN.md "Parity": a stated deviation the device reproduces bit for bit).  True
    hands O.qp_backward inputs on which that residue is exactly zero, so that a coordinate is active
    iff v sits on its bound -- the set the exact projection has; the finite-difference check of the
    formulas uses it, the device parity tests do not."""
    h = np.asarray(h, F32)
    g_f = np.asarray(g_f, F32)
    N = h.shape[0]
    u_rows = np.repeat(O.static_projection(x_feat, P), S, axis=0)
    fwd = R.mlp_forward if activation == "GroupSort" else O.mlp_forward
    mlp = fwd(h, u_rows, P, None, None, 0.0)
    lower = O.barrier_lower(h, cfg)
    upper = O.barrier_upper(h, cfg)
    span = (upper - lower).astype(F32)
    if cfg.scale_nominal:
        nominal, sig = O.scale_nominal(mlp["ftilde"], lower, upper)
    else:
        nominal, sig = mlp["ftilde"], None
    ql, qn = (lower, nominal) if qp_inputs is None else (np.asarray(qp_inputs[0], F32), np.asarray(qp_inputs[1], F32))
    if K is None:
        K = O.qp_forward(ql, qn, cfg.qp_max_iter, cfg.qp_tol).iters
    v, mu = O.qp_run_fixed(ql, qn, int(K))
    if bound_active:
        g_low, g_nom = O.qp_backward(g_f, v, np.zeros_like(mu), ql, np.where(v > ql, v, (qn - mu[:, None]).astype(F32)))
    else:
        g_low, g_nom = O.qp_backward(g_f, v, mu, ql, qn)
    g_low, g_nom = g_low.astype(np.float64), g_nom.astype(np.float64)
    if cfg.scale_nominal:
        s64 = sig.astype(np.float64)
        g_ft = g_nom * span * s64 * (1.0 - s64)
        g_lower_tot = g_low + g_nom * (1.0 - s64)
        g_upper = g_nom * s64
    else:
        g_ft, g_lower_tot, g_upper = g_nom, g_low, np.zeros_like(g_nom)
    if activation == "GroupSort":
        gr = mlp_backward_groupsort(g_ft, h, x_feat, S, P, mlp)
        g_z1 = gr["g_z1"]
    else:
        gr = O.mlp_backward(g_ft, h, x_feat, S, P, mlp, None, None, 0.0)
        # the per-row g_z1: the same function with one row per "image" (its g_u is then g_z1)
        g_z1 = O.mlp_backward(g_ft, h, np.repeat(np.asarray(x_feat), S, axis=0), 1, P, mlp, None, None,
                              0.0)["g_u"].astype(np.float64)
    h64 = h.astype(np.float64)
    dlow = -cfg.alpha_1 * cfg.sigma_1 * np.exp(cfg.sigma_1 * h64)
    g_h = g_lower_tot * dlow + g_upper * (-cfg.alpha_2) + g_z1 @ P.Q1.astype(np.float64)
    out = {k: gr[k] for k in KEYS}
    out.update(g_h=g_h, margin=preact_margin(mlp, activation), f=v, mu=mu, K=int(K), lower=ql, nominal=qn,
               g_ft=g_ft, g_z1=g_z1, mlp=mlp)
    assert g_h.shape == (N, h.shape[1])
    return out


# ---- float64 restatement with the exact projection (finite differences) --------------------------
def _act64(z, activation):
    if activation == "GroupSort":
        m = z.shape[1] // 2
        return np.concatenate([np.maximum(z[:, :m], z[:, m:]), np.minimum(z[:, :m], z[:, m:])], axis=1)
    return np.maximum(z, 0.0)


def exact_projection(lower, nominal):
    """argmin |v - nominal|^2 s.t. sum v = 0, v >= lower: v = max(nominal - mu, lower) with mu
    bisected until the bracket is below 1e-14.  Returns (v, mu)."""
    lo = nominal.min(1) - 1.0
    hi = (nominal - lower).max(1) + 1.0
    while float((hi - lo).max()) > 1e-14:
        mu = 0.5 * (lo + hi)
        eps = np.maximum(nominal - mu[:, None], lower).sum(1)
        lo = np.where(eps > 0, mu, lo)
        hi = np.where(eps > 0, hi, mu)
        if np.all(0.5 * (lo + hi) == mu):       # the bracket no longer moves (float64 resolution)
            break
    mu = 0.5 * (lo + hi)
    return np.maximum(nominal - mu[:, None], lower), mu


def f64_eval_dot(h, u_rows, P, cfg, activation):
    """eval_dot in float64 with the exact projection.  Returns (f, qp margin [N]) with the QP margin
    min_j |nominal_j - mu - lower_j| (the distance of the row from a change of its active set)."""
    h = np.asarray(h, np.float64)
    Q = {k: np.asarray(getattr(P, k), np.float64) for k in ("Q1", "b1", "Q2", "b2", "Q3", "b3")}
    z1 = h @ Q["Q1"].T + Q["b1"] + np.asarray(u_rows, np.float64)
    z2 = _act64(z1, activation) @ Q["Q2"].T + Q["b2"]
    ft = _act64(z2, activation) @ Q["Q3"].T + Q["b3"]
    lower = -cfg.alpha_1 * (np.exp(cfg.sigma_1 * h) - 1.0)
    upper = cfg.alpha_2 * (1.0 - h)
    nominal = (upper - lower) / (1.0 + np.exp(-ft)) + lower if cfg.scale_nominal else ft
    v, mu = exact_projection(lower, nominal)
    return v, np.abs(nominal - mu[:, None] - lower).min(1)
