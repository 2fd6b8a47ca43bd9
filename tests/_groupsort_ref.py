"""Reference pieces of the GroupSort dynamics tests (test_groupsort_dyn.py, test_gpu_groupsort_dyn.py).

``mlp_forward`` is ``oracle.fiode_oracle.mlp_forward`` with GroupSort where ReLU stands
(classification.py:98, 100 with ``activation = GroupSort()``): over the 128 hidden units, with
a = z[:, :64] and b = z[:, 64:], the activation is cat(max(a, b), min(a, b)).  Tests install it with
``monkeypatch.setattr(O, "mlp_forward", mlp_forward)``; O.eval_dot, O.make_ode_func, O.rk4_fixed_grid,
O.dopri5 and O.certify_image then run GroupSort dynamics, and nothing under oracle/ changes.

``dyadic_params`` / ``dyadic_rows`` build weights and states on which float32 is exact in any
accumulation order, so the device MLP and this reference agree bit for bit and a mis-paired unit
moves the output by >= 0.25.
"""
import numpy as np

from oracle import fiode_oracle as O

F32 = np.float32


def groupsort(z: np.ndarray) -> np.ndarray:
    m = z.shape[-1] // 2
    a, b = z[..., :m], z[..., m:]
    return np.concatenate([np.maximum(a, b), np.minimum(a, b)], axis=-1).astype(F32)


def mlp_forward(h, u_rows, P, mask1, mask2, p):
    """Same signature as O.mlp_forward; eval mode only (no dropout masks).  Matmuls in float64,
    activations rounded to float32."""
    assert mask1 is None and mask2 is None, "GroupSort dynamics: eval mode only (no dropout masks)"
    h64 = np.asarray(h, np.float64)
    z1 = ((h64 @ P.Q1.astype(np.float64).T + P.b1).astype(F32) + u_rows).astype(F32)
    a1 = groupsort(z1)
    z2 = (a1.astype(np.float64) @ P.Q2.astype(np.float64).T + P.b2).astype(F32)
    a2 = groupsort(z2)
    ft = (a2.astype(np.float64) @ P.Q3.astype(np.float64).T + P.b3).astype(F32)
    return dict(z1=z1, a1=a1, z2=z2, a2=a2, ftilde=ft)


def mlp_forward_shifted(delta: float):
    """mlp_forward (GroupSort) with the MLP output shifted by ``delta``: the seed check of the
    dopri5 cases reruns the reference with +-2e-5 and keeps seeds whose step sequence stays."""
    def f(h, u_rows, P, mask1, mask2, p):
        out = mlp_forward(h, u_rows, P, mask1, mask2, p)
        out["ftilde"] = (out["ftilde"] + F32(delta)).astype(F32)
        return out
    return f


# ---- dyadic weights ------------------------------------------------------------------------------
# Every state entry is v / 8 (integer v in 0..4, row sum 1), so with Q1 in multiples of 1/4 and the
# biases in multiples of 1/8 every pre-activation is a multiple of 1/32 of magnitude < 16, and every
# partial sum of the three layers is exactly representable in float32: any accumulation order gives
# the same bits.
#
# Layer 1, pair (u, u + 64): Q1[u] = Q1[u + 64] - s/4 + 4 s e_k (s = +-1, k a coordinate, both per
# unit), b1[u] = b1[u + 64]; the rows sum to 1, so z1[u] - z1[u + 64] = s (4 h_k - 1/4), which is one
# of -+1/4, +-1/4, +-3/4, ...: at least 1/4 apart, and WHICH of the two is larger changes from row to
# row with h_k.
# Layer 2: Q2 is a signed permutation (unit i reads unit perm[i]) built so that units move between
# the halves and between 16- and 32-unit blocks; b2[i] = -b2[i + 64] = +-4 keeps each pair 8 - 2 max|a1|
# apart (asserted on the reference by the tests, with max|a1| <= 3.25 here).
# Layer 3: Q3 in {0, +-1}, hidden unit u read by output u % 10 only, with sign (-1)^(u // 10).

def dyadic_params(seed: int = 3):
    rng = np.random.default_rng(seed)
    M, C, X = 128, 10, 10
    half = M // 2
    Q1 = np.zeros((M, C))
    lo = rng.integers(-2, 3, (half, C)) / 4.0               # multiples of 1/4 in [-1/2, 1/2]
    s = rng.choice([-1.0, 1.0], half)
    k = rng.integers(0, C, half)
    Q1[half:] = lo
    Q1[:half] = lo - s[:, None] / 4.0
    Q1[np.arange(half), k] += 4.0 * s
    b1h = rng.integers(-4, 5, half) / 8.0
    b1 = np.concatenate([b1h, b1h])
    # signed permutation: i -> (37 i + 21) mod 128 (37 odd: a bijection); it sends 0..15 to
    # 21, 58, 95, 4, 41, 78, 115, 24, ...: both halves and every 16-/32-unit block within one block
    perm = (37 * np.arange(M) + 21) % M
    sign = rng.choice([-1.0, 1.0], M)
    Q2 = np.zeros((M, M))
    Q2[np.arange(M), perm] = sign
    t = rng.choice([-1.0, 1.0], half)
    b2 = np.concatenate([4.0 * t, -4.0 * t]) + np.tile(rng.integers(-2, 3, half) / 8.0, 2)
    Q3 = np.zeros((C, M))
    # signs alternate along the units an output reads, so the +-4 of b2 cancel to within 4 and the
    # MLP output (and with it the QP's multiplier) stays O(1)
    Q3[np.arange(M) % C, np.arange(M)] = np.where((np.arange(M) // C) % 2 == 0, 1.0, -1.0)
    b3 = rng.integers(-4, 5, C) / 8.0
    P = O.DynParams(Q1=Q1, b1=b1, Qx=np.zeros((M, X)), bx=np.zeros(M), Q2=Q2, b2=b2, Q3=Q3, b3=b3)
    return P.astype32()


def dyadic_rows(n: int, seed: int = 4) -> np.ndarray:
    """n simplex rows v / 8 (integer v, 0 <= v <= 4, sum 8), not all equal."""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < n:
        v = np.bincount(rng.integers(0, 10, 8), minlength=10)
        if v.max() <= 4:
            rows.append(v)
    h = (np.asarray(rows) / 8.0).astype(F32)
    assert len(np.unique(h, axis=0)) > n // 2
    return h


def pair_separation(mlp: dict) -> float:
    """Smallest |z[u] - z[u + 64]| over both hidden layers and all rows of a reference MLP result."""
    d = []
    for z in (mlp["z1"], mlp["z2"]):
        m = z.shape[-1] // 2
        d.append(np.abs(z[..., :m].astype(np.float64) - z[..., m:]).min())
    return float(min(d))
