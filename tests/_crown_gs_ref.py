"""numpy reference of the GroupSort CROWN bounds (fiode_certify_crown_act with FIODE_ACT_GROUPSORT).

GroupSort over the pairs (i, i + H), H = 64 (tests/_groupsort_ref.py): with d = z[:H] - z[H:] and
r = relu(d) the layer is  a[:H] = max = z[H:] + r,  a[H:] = min = z[:H] - r  exactly, i.e.
a = S z + [I; -I] r with S the swap of the halves.  A GroupSort layer is therefore H ReLU units on the
pair differences plus a linear skip path, and backward CROWN (Zhang et al. 2018, Theorem 3.2, restated in
tests/_crown_ref.py) applies with the ReLU relaxation unchanged.  With Delta = [I, -I], N(W) = W[:, :H] -
W[:, H:] and P(W) = W S:

  z1 = W1 eta + u,                    d1 = Delta z1                         (exact interval)
  z2 = P(W2) z1 + N(W2) r1 + b2,      d2 = Delta z2                         (backward pass, H rows)
  o  = P(W3) z2 + N(W3) r2 + b3                                             (backward pass)

Float64 throughout; everything after the bounds is tests/_crown_ref.py's (``crown_image(..., bounds=)``).
``pairs`` names the pairing: 'half' is the net's own; 'adjacent' (i, i + 1) is a mutation that the CPU
tests use to show that a mis-paired relaxation does not enclose the net.
"""
from dataclasses import dataclass

import numpy as np

from tests import _crown_ref as R
from tests._crown_ref import F64, neg, pos, relu_relaxation, sample_box   # noqa: F401  (re-exported)


# The GPU parity cases (tests/test_gpu_certify_crown_gs.py): label, parameter seed and, per T, the seed of
# the unit-scale N(0, 1) features.  tests/test_crown_gs_ref.py asserts on the host that no grid row of
# these cases is within TIE of a slope tie on either layer, so the GPU comparison leaves no row out.
GPU_LABEL, GPU_PARAM_SEED, TIE = 3, 0, 1e-5
GPU_FEATURE_SEED = {6: 1006, 8: 1008}
GPU_BATCHES = {6: 10, 8: 61}


def features(seed: int) -> np.ndarray:
    return np.random.default_rng(seed).normal(size=10).astype(np.float32)


def pairing(M: int, pairs: str = "half"):
    """(ia, ib): unit ia[p] pairs with ib[p]; ia takes the max, ib the min."""
    H = M // 2
    if pairs == "half":
        return np.arange(H), np.arange(H) + H
    if pairs == "adjacent":
        return 2 * np.arange(H), 2 * np.arange(H) + 1
    raise ValueError(pairs)


def pair_maps(M: int, pairs: str = "half"):
    """(Delta [H][M], swap [M]): d = Delta z; (S z)[k] = z[swap[k]]."""
    ia, ib = pairing(M, pairs)
    H = M // 2
    D = np.zeros((H, M))
    D[np.arange(H), ia] = 1.0
    D[np.arange(H), ib] = -1.0
    swap = np.arange(M)
    swap[ia], swap[ib] = ib, ia
    return D, swap


def groupsort(z: np.ndarray, pairs: str = "half") -> np.ndarray:
    ia, ib = pairing(z.shape[-1], pairs)
    a = np.empty_like(z)
    a[..., ia] = np.maximum(z[..., ia], z[..., ib])
    a[..., ib] = np.minimum(z[..., ia], z[..., ib])
    return a


@dataclass
class Net(R.Net):
    """z1 = W1 eta + u; z2 = W2 GroupSort(z1) + b2; out = W3 GroupSort(z2) + b3 (float64)."""

    def hidden(self, eta: np.ndarray):
        z1 = np.asarray(eta, F64) @ self.W1.T + self.u
        z2 = groupsort(z1) @ self.W2.T + self.b2
        return z1, z2

    def forward(self, eta: np.ndarray) -> np.ndarray:
        return groupsort(self.hidden(eta)[1]) @ self.W3.T + self.b3

    def differences(self, eta: np.ndarray):
        """(d1, d2): the pair differences of both hidden layers, [n][H] each."""
        z1, z2 = self.hidden(eta)
        H = z1.shape[-1] // 2
        return z1[..., :H] - z1[..., H:], z2[..., :H] - z2[..., H:]


def net_of(P, x_feat: np.ndarray) -> Net:
    n = R.net_of(P, x_feat)
    return Net(n.W1, n.u, n.W2, n.b2, n.W3, n.b3)


def crown_bounds(net: R.Net, eta0: np.ndarray, eps: float, chunk: int = 1024, form: str = "four",
                 outputs: bool = True, pairs: str = "half") -> R.Bounds:
    """Backward CROWN of the GroupSort ``net`` over the boxes eta0 +- eps.  Returns tests/_crown_ref.py's
    Bounds with l1, u1 / l2, u2 the bounds of the pair differences d1 / d2 ([N][H]), so that tie1 / tie2
    are the distances of the H slope-carrying units of each layer from the lower slope's tie."""
    eta0 = np.asarray(eta0, F64)
    N = len(eta0)
    W1, W2, W3 = net.W1, net.W2, net.W3
    M, no, ni = W2.shape[0], W3.shape[0], W1.shape[1]
    H = M // 2
    D, swap = pair_maps(M, pairs)
    ia, ib = pairing(M, pairs)
    Nf = lambda W: W[:, ia] - W[:, ib]                 # W a = P(W) z + N(W) r
    Pf = lambda W: W[:, swap]
    N2, P2, N3, P3 = Nf(W2), Pf(W2), Nf(W3), Pf(W3)
    A1 = D @ W1                                        # d1 = A1 eta + Delta u
    A2, S2 = D @ N2, D @ P2                            # d2 = S2 z1 + A2 r1 + Delta b2
    S2W1, db2 = S2 @ W1, D @ net.b2
    out = R.Bounds(*[np.zeros((N, no)) for _ in range(2)], *[np.zeros((N, H)) for _ in range(4)])
    for lo in range(0, N, chunk):
        sl = slice(lo, min(N, lo + chunk))
        n = sl.stop - sl.start
        z1 = eta0[sl] @ W1.T + net.u
        d1 = z1 @ D.T
        rad = eps * np.abs(A1).sum(1)
        l1, u1 = d1 - rad, d1 + rad
        s1, t1, al1 = relu_relaxation(l1, u1)
        # layer-2 pair differences: alpha1 d1 <= r1 <= s1 d1 + t1 by the sign of A2, d1 = A1 eta + Delta u;
        # the skip term S2 z1 is affine in eta with a matrix that does not depend on the row
        B = np.concatenate([np.broadcast_to(A1, (n,) + A1.shape), d1[:, :, None]], 2)
        MUB, MLB = R.layer2_products(A2, s1, al1, B, form)
        skip = z1 @ S2.T
        u2 = MUB[:, :, ni] + skip + eps * np.abs(MUB[:, :, :ni] + S2W1).sum(2) + t1 @ pos(A2).T + db2
        l2 = MLB[:, :, ni] + skip - eps * np.abs(MLB[:, :, :ni] + S2W1).sum(2) + t1 @ neg(A2).T + db2
        out.l1[sl], out.u1[sl], out.l2[sl], out.u2[sl] = l1, u1, l2, u2
        if not outputs:
            continue
        s2, t2, al2 = relu_relaxation(l2, u2)
        # outputs: Lambda on r2, Q = P(W3) + Lambda Delta on z2, K = Q N(W2) on r1, R on d1,
        # Q P(W2) + R Delta on z1
        LU = pos(N3)[None] * s2[:, None, :] + neg(N3)[None] * al2[:, None, :]
        LL = pos(N3)[None] * al2[:, None, :] + neg(N3)[None] * s2[:, None, :]
        QU, QL = P3[None] + LU @ D, P3[None] + LL @ D
        KU, KL = QU @ N2, QL @ N2
        RU = pos(KU) * s1[:, None, :] + neg(KU) * al1[:, None, :]
        RL = pos(KL) * al1[:, None, :] + neg(KL) * s1[:, None, :]
        ZU, ZL = QU @ P2 + RU @ D, QL @ P2 + RL @ D
        ub = (np.einsum("nik,nk->ni", ZU, z1) + eps * np.abs(ZU @ W1).sum(2) + np.einsum("nik,nk->ni", pos(KU), t1)
              + QU @ net.b2 + t2 @ pos(N3).T + net.b3)
        lb = (np.einsum("nik,nk->ni", ZL, z1) - eps * np.abs(ZL @ W1).sum(2) + np.einsum("nik,nk->ni", neg(KL), t1)
              + QL @ net.b2 + t2 @ neg(N3).T + net.b3)
        out.lb[sl], out.ub[sl] = lb, ub
    return out


def _affine_interval(W, l, u):
    return l @ pos(W).T + u @ neg(W).T, u @ pos(W).T + l @ neg(W).T


def interval_bounds(net: R.Net, eta0: np.ndarray, eps: float):
    """Interval arithmetic in the same pair-difference form: exact boxes for z1 and d1, then
    z2 = P(W2) z1 + N(W2) r1 + b2, d2 = Delta z2 and o = P(W3) z2 + N(W3) r2 + b3 term by term with
    z and r as independent boxes.  Returns (l_d2, u_d2, l_o, u_o)."""
    eta0 = np.asarray(eta0, F64)
    M = net.W2.shape[0]
    H = M // 2
    D, swap = pair_maps(M)
    Nf = lambda W: W[:, :H] - W[:, H:]
    Pf = lambda W: W[:, swap]
    c, r = eta0 @ net.W1.T + net.u, eps * np.abs(net.W1).sum(1)
    zl, zu = c - r, c + r
    dc, dr = c @ D.T, eps * np.abs(D @ net.W1).sum(1)
    rl, ru = np.maximum(dc - dr, 0), np.maximum(dc + dr, 0)
    res = []
    for W, b, last in ((net.W2, net.b2, False), (net.W3, net.b3, True)):
        if not last:
            pl, pu = _affine_interval(D @ Pf(W), zl, zu)
            ql, qu = _affine_interval(D @ Nf(W), rl, ru)
            dl, du = pl + ql + D @ b, pu + qu + D @ b
            res += [dl, du]
        pl, pu = _affine_interval(Pf(W), zl, zu)
        ql, qu = _affine_interval(Nf(W), rl, ru)
        zl, zu = pl + ql + b, pu + qu + b
        if not last:
            rl, ru = np.maximum(dl, 0), np.maximum(du, 0)
    return res[0], res[1], zl, zu
