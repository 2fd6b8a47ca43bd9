"""Reference of the GroupSort TRAINING step (test_groupsort_train.py, test_gpu_groupsort_train.py).

``mlp_forward`` / ``mlp_backward`` have the signatures of ``oracle.fiode_oracle``'s and compute the
reference's training-mode MLP with ``activation = GroupSort()`` (classification.py:96-102):
a = GroupSort(dropout(z)) per hidden layer.  With the keep mask k and scale = 1 / (1 - p),
d = z * (k * scale) in float32 (``O.mlp_forward``'s expression), and over the 128 units, with
a = d[:, :64] and b = d[:, 64:], the activation is cat(max(a, b), min(a, b)).  Backward: the max and
min gradients go back to the pair's members by the order of d, a tie gives both members
g_max / 2 + g_min / 2 (torch.maximum / minimum), and the result is multiplied by k * scale.
Matmuls in float64, activations rounded to float32 (as tests/_groupsort_ref.py).

Tests install both with ``monkeypatch.setattr(O, "mlp_forward", ...)`` / ``(O, "mlp_backward", ...)``;
``O.eval_dot`` and ``O.lyapunov_step`` then run a GroupSort training step, and nothing under oracle/
changes.  With masks None, ``mlp_forward`` is tests/_groupsort_ref.mlp_forward.
"""
import numpy as np

F32 = np.float32
HALF = 64


def _drop(z, mask, scale):
    return (z * (mask.astype(F32) * scale)).astype(F32) if mask is not None else z


def _sort(d):
    a, b = d[:, :HALF], d[:, HALF:]
    return np.concatenate([np.maximum(a, b), np.minimum(a, b)], axis=1).astype(F32)


def mlp_forward(h, u_rows, P, mask1, mask2, p):
    """Same signature and keys as O.mlp_forward, plus d1 / d2 (the dropped pre-activations the
    sort orders)."""
    scale = F32(1.0 / (1.0 - p)) if p > 0 else F32(1.0)
    h64 = np.asarray(h, np.float64)
    z1 = ((h64 @ P.Q1.astype(np.float64).T + P.b1).astype(F32) + u_rows).astype(F32)
    d1 = _drop(z1, mask1, scale)
    a1 = _sort(d1)
    z2 = (a1.astype(np.float64) @ P.Q2.astype(np.float64).T + P.b2).astype(F32)
    d2 = _drop(z2, mask2, scale)
    a2 = _sort(d2)
    ft = (a2.astype(np.float64) @ P.Q3.astype(np.float64).T + P.b3).astype(F32)
    return dict(z1=z1, d1=d1, a1=a1, z2=z2, d2=d2, a2=a2, ftilde=ft)


def _route(g_a, d):
    """d L / d d from d L / d a (float64) by the order of the float32 d."""
    a, b = d[:, :HALF], d[:, HALF:]
    gmx, gmn = g_a[:, :HALF], g_a[:, HALF:]
    halfsum = gmx / 2.0 + gmn / 2.0
    first, tie = a > b, a == b
    ga = np.where(tie, halfsum, np.where(first, gmx, gmn))
    gb = np.where(tie, halfsum, np.where(first, gmn, gmx))
    return np.concatenate([ga, gb], axis=1)


def mlp_backward(g_ft, h, x_feat, S, P, mlp, mask1, mask2, p):
    """Same signature and keys as O.mlp_backward (float64 sums); ``mlp`` is mlp_forward's result."""
    scale = (1.0 / (1.0 - p)) if (p > 0 and mask1 is not None) else 1.0
    g3 = np.asarray(g_ft, np.float64)
    a1 = mlp["a1"].astype(np.float64)
    a2 = mlp["a2"].astype(np.float64)
    out = {}
    out["Q3"] = g3.T @ a2
    out["b3"] = g3.sum(0)
    g_a2 = g3 @ P.Q3.astype(np.float64)
    m2 = (mask2.astype(np.float64) * scale) if mask2 is not None else 1.0
    g_z2 = _route(g_a2, mlp["d2"]) * m2
    out["Q2"] = g_z2.T @ a1
    out["b2"] = g_z2.sum(0)
    g_a1 = g_z2 @ P.Q2.astype(np.float64)
    m1 = (mask1.astype(np.float64) * scale) if mask1 is not None else 1.0
    g_z1 = _route(g_a1, mlp["d1"]) * m1
    out["Q1"] = g_z1.T @ np.asarray(h, np.float64)
    out["b1"] = g_z1.sum(0)
    B = x_feat.shape[0]
    g_u = g_z1.reshape(B, S, -1).sum(1)
    out["Qx"] = g_u.T @ np.asarray(x_feat, np.float64)
    out["bx"] = g_u.sum(0)
    out["x_feat"] = g_u @ P.Qx.astype(np.float64)
    out["g_u"] = g_u
    return {k: v.astype(F32) for k, v in out.items()}


def pair_separation(mlp, mask1, mask2):
    """Smallest |d[u] - d[u + 64]| over both hidden layers and all rows, over the pairs that are not
    both dropped (those are exact ties of two zeros whose gradient is zero through the mask)."""
    best = np.inf
    for d, m in ((mlp["d1"], mask1), (mlp["d2"], mask2)):
        sep = np.abs(d[:, :HALF].astype(np.float64) - d[:, HALF:])
        if m is not None:
            live = (m[:, :HALF] != 0) | (m[:, HALF:] != 0)
            sep = sep[live]
        if sep.size:
            best = min(best, float(sep.min()))
    return best


def near_ties(mlp, mask1, mask2, eps):
    """Number of pairs (not both dropped) closer than ``eps``, over both layers."""
    n = 0
    for d, m in ((mlp["d1"], mask1), (mlp["d2"], mask2)):
        sep = np.abs(d[:, :HALF].astype(np.float64) - d[:, HALF:])
        live = np.ones_like(sep, bool) if m is None else ((m[:, :HALF] != 0) | (m[:, HALF:] != 0))
        n += int((sep[live] < eps).sum())
    return n


# The GPU parity cases (test_gpu_groupsort_train.py): (B, S, seed, scale_nominal) with
# P = make_params(seed) and make_step_inputs(B, S, seed=seed + 1).  GroupSort's gradient is
# discontinuous where a pair's order flips, and a float32 device may order a pair closer than the
# MLP's rounding differently from this float64 reference; one flipped pair moves entries of the weight
# gradients by ~1e-2 of their max.  An elementwise gradient bound therefore needs inputs without a
# near tie: on these the smallest loss-pass separation is >= 2e-5 (test_groupsort_train.py asserts
# it), about 100 float32 roundings of the O(1) pre-activations.  One tile; a partial last tile with
# images straddling tiles; 32 tiles over 8 rounds.
PARITY_CASES = [(4, 8, 408, True), (4, 8, 408, False), (3, 37, 337, True), (16, 64, 1692, False)]
MIN_SEPARATION = 2e-5
