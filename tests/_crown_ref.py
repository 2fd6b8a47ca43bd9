"""numpy reference of the CROWN certification pass (fiode_certify_crown, crown.hip).

The bounds are float64 and restate the published algorithm, since the library the reference calls
for them (``auto_LiRPA``, certify_crown.py:108-139, ``method='CROWN'``) is absent:

  * Zhang, Weng, Chen, Hsieh, Daniel, "Efficient Neural Network Robustness Certification with General
    Activation Functions" (NeurIPS 2018): backward substitution of linear relaxations, Theorem 3.2;
    the ReLU relaxation with the adaptive lower slope of its section 3.3 / Table 2 (``auto_LiRPA``'s
    default for ``method='CROWN'``: ``lower_d = (upper_d > 0.5)``, so a tie u = -l gives 0);
  * pre-activation bounds of layer 2 by the same backward pass (not interval arithmetic).

Everything after the bounds is the reference's own text: ``ibp_sigmoid`` (classification.py:175-181),
``ibp_cbf_qp`` with ``upper=False`` (classification.py:208-242), ``perturbed_vdot`` and the runner-up
mask (certify_crown.py:29-34, 143-150).  That stage runs in float32 as torch does, the two solver
calls through ``oracle.fiode_oracle.qp_forward`` (FastBarrierProjectionNoUpper) over rows x 10
problems, each with its own batch-global exit.

Rows are chunked, and no [rows][128][128] array is formed: the coefficient rows are applied to their
right-hand sides directly.
"""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from oracle import fiode_oracle as O

F32 = np.float32
F64 = np.float64


def pos(W):
    return np.maximum(W, 0.0)


def neg(W):
    return np.minimum(W, 0.0)


def relu_relaxation(l: np.ndarray, u: np.ndarray):
    """Upper line a <= s z + t, lower line a >= alpha z on [l, u] (Zhang et al. 2018, section 3.3):
    l >= 0: identity; u <= 0: zero; otherwise s = u / (u - l), t = -s l, alpha = 1 iff u > -l."""
    l = np.asarray(l, F64)
    u = np.asarray(u, F64)
    act, dead = l >= 0, (u <= 0) & ~(l >= 0)
    uns = ~act & ~dead
    den = np.where(uns, u - l, 1.0)
    s = np.where(act, 1.0, np.where(dead, 0.0, u / den))
    t = np.where(uns, -s * l, 0.0)
    al = np.where(act, 1.0, np.where(dead, 0.0, (u > -l).astype(F64)))
    return s, t, al


@dataclass
class Net:
    """z1 = W1 eta + u; z2 = W2 relu(z1) + b2; out = W3 relu(z2) + b3 (float64)."""
    W1: np.ndarray
    u: np.ndarray
    W2: np.ndarray
    b2: np.ndarray
    W3: np.ndarray
    b3: np.ndarray

    def forward(self, eta: np.ndarray) -> np.ndarray:
        a1 = np.maximum(np.asarray(eta, F64) @ self.W1.T + self.u, 0.0)
        a2 = np.maximum(a1 @ self.W2.T + self.b2, 0.0)
        return a2 @ self.W3.T + self.b3


def net_of(P: O.DynParams, x_feat: np.ndarray) -> Net:
    """The dynamics MLP of one image (_h_dot_raw, classification.py:156-162, dropout off) with the
    static term folded into layer 1's bias: u = Qx x + bx + b1."""
    f = lambda a: np.asarray(a, F64)
    u = f(P.Qx) @ f(x_feat).reshape(-1) + f(P.bx) + f(P.b1)
    return Net(f(P.Q1), u, f(P.Q2), f(P.b2), f(P.Q3), f(P.b3))


@dataclass
class Bounds:
    lb: np.ndarray            # [N][out]
    ub: np.ndarray
    l1: np.ndarray            # [N][hidden] layer-1 pre-activation bounds (exact)
    u1: np.ndarray
    l2: np.ndarray            # [N][hidden] layer-2 pre-activation bounds (backward CROWN)
    u2: np.ndarray

    @property
    def tie1(self) -> np.ndarray:
        """min_k |u1_k + l1_k| per row: the distance of layer 1 from the lower slope's tie u = -l."""
        return np.abs(self.u1 + self.l1).min(1)

    @property
    def tie2(self) -> np.ndarray:
        return np.abs(self.u2 + self.l2).min(1)


def layer2_products(W2, s1, al1, B, form: str = "four"):
    """(M^U B, M^L B) for every row, with M^U = W2+ D(s1) + W2- D(alpha1), M^L = W2+ D(alpha1) + W2- D(s1)
    and B [n][k][c]: -> two [n][j][c] arrays, without forming any [n][j][k] matrix.
    form='four': the four products as written; form='half': (1/2)[W2 D(s1 + alpha1) +- |W2| D(s1 - alpha1)] B,
    the two products per row the kernel runs."""
    if form == "four":
        sB, aB = s1[:, :, None] * B, al1[:, :, None] * B
        return pos(W2) @ sB + neg(W2) @ aB, pos(W2) @ aB + neg(W2) @ sB
    A = W2 @ ((s1 + al1)[:, :, None] * B)
    D = np.abs(W2) @ ((s1 - al1)[:, :, None] * B)
    return 0.5 * (A + D), 0.5 * (A - D)


def crown_bounds(net: Net, eta0: np.ndarray, eps: float, chunk: int = 1024, form: str = "four",
                 outputs: bool = True) -> Bounds:
    """Backward CROWN (Zhang et al. 2018, Theorem 3.2) of ``net`` over the L-inf boxes eta0 +- eps.
    outputs=False: stop after the layer-2 pre-activation bounds (lb, ub stay zero): what the tie
    distances need."""
    eta0 = np.asarray(eta0, F64)
    N = len(eta0)
    nh, no, ni = net.W2.shape[0], net.W3.shape[0], net.W1.shape[1]
    out = Bounds(*[np.zeros((N, no)) for _ in range(2)], *[np.zeros((N, nh)) for _ in range(4)])
    W1, W2, W3 = net.W1, net.W2, net.W3
    for lo in range(0, N, chunk):
        sl = slice(lo, min(N, lo + chunk))
        n = sl.stop - sl.start
        # layer 1: the input box through one linear map is exact
        z1 = eta0[sl] @ W1.T + net.u
        r1 = eps * np.abs(W1).sum(1)
        l1, u1 = z1 - r1, z1 + r1
        s1, t1, al1 = relu_relaxation(l1, u1)
        # layer 2 pre-activations: z2 = W2 a1 + b2 with s1 z1 + t1 >= a1 >= alpha1 z1 elementwise;
        # the coefficient rows M^U, M^L applied to [W1 | z1] in one go
        B = np.concatenate([np.broadcast_to(W1, (n,) + W1.shape), z1[:, :, None]], 2)
        MUB, MLB = layer2_products(W2, s1, al1, B, form)
        u2 = MUB[:, :, ni] + eps * np.abs(MUB[:, :, :ni]).sum(2) + t1 @ pos(W2).T + net.b2
        l2 = MLB[:, :, ni] - eps * np.abs(MLB[:, :, :ni]).sum(2) + t1 @ neg(W2).T + net.b2
        out.l1[sl], out.u1[sl], out.l2[sl], out.u2[sl] = l1, u1, l2, u2
        if not outputs:
            continue
        s2, t2, al2 = relu_relaxation(l2, u2)
        # outputs: out = W3 a2 + b3, substituted back through layer 2 and then layer 1
        LU = pos(W3)[None] * s2[:, None, :] + neg(W3)[None] * al2[:, None, :]
        LL = pos(W3)[None] * al2[:, None, :] + neg(W3)[None] * s2[:, None, :]
        QU, QL = LU @ W2, LL @ W2
        RU = pos(QU) * s1[:, None, :] + neg(QU) * al1[:, None, :]
        RL = pos(QL) * al1[:, None, :] + neg(QL) * s1[:, None, :]
        ub = (np.einsum("nik,nk->ni", RU, z1) + eps * np.abs(RU @ W1).sum(2) + np.einsum("nik,nk->ni", pos(QU), t1)
              + LU @ net.b2 + t2 @ pos(W3).T + net.b3)
        lb = (np.einsum("nik,nk->ni", RL, z1) - eps * np.abs(RL @ W1).sum(2) + np.einsum("nik,nk->ni", neg(QL), t1)
              + LL @ net.b2 + t2 @ neg(W3).T + net.b3)
        out.lb[sl], out.ub[sl] = lb, ub
    return out


def interval_bounds(net: Net, eta0: np.ndarray, eps: float) -> Tuple[np.ndarray, np.ndarray]:
    """Plain interval arithmetic through the three layers (what CROWN is NOT)."""
    eta0 = np.asarray(eta0, F64)
    c, r = eta0 @ net.W1.T + net.u, eps * np.abs(net.W1).sum(1)
    l, u = np.maximum(c - r, 0), np.maximum(c + r, 0)
    for W, b, last in ((net.W2, net.b2, False), (net.W3, net.b3, True)):
        l, u = l @ pos(W).T + u @ neg(W).T + b, u @ pos(W).T + l @ neg(W).T + b
        if not last:
            l, u = np.maximum(l, 0), np.maximum(u, 0)
    return l, u


def sample_box(eta0: np.ndarray, eps: float, n: int, rng) -> np.ndarray:
    """[N][n][C] points of the boxes eta0 +- eps: the first half corners, the rest uniform."""
    N, Cn = eta0.shape
    d = rng.uniform(-1.0, 1.0, (N, n, Cn))
    d[:, :n // 2] = np.sign(d[:, :n // 2])
    return eta0[:, None, :].astype(F64) + eps * d


# ---- the stage after the bounds, float32 as torch runs it --------------------------------------------
def barrier_lo(h: np.ndarray, cfg: O.DynConfig) -> np.ndarray:
    """-alpha_1 (exp(sigma_1 h) - 1), classification.py:177-178 / 224-225 (= O.barrier_lower)."""
    return O.barrier_lower(h, cfg)


def ibp_sigmoid(lb, ub, h_lb, h_ub, cfg: O.DynConfig):
    """classification.py:175-181."""
    lower_lb, lower_ub = barrier_lo(h_ub, cfg), barrier_lo(h_lb, cfg)
    a2 = F32(cfg.alpha_2)
    sl, su = O.sigmoid32(lb), O.sigmoid32(ub)
    out_lb = (((a2 * (F32(1) - h_ub)).astype(F32) - lower_lb).astype(F32) * sl).astype(F32) + lower_lb
    out_ub = (((a2 * (F32(1) - h_lb)).astype(F32) - lower_ub).astype(F32) * su).astype(F32) + lower_ub
    return out_lb.astype(F32), out_ub.astype(F32)


def ibp_cbf_qp_problems(h, eps32, lb, ub, cfg: O.DynConfig):
    """The rows x 10 problems of both solver calls, classification.py:210-231 (upper=False): returns
    (lower_lb, f_tilde_lb, lower_ub, f_tilde_ub), each [N * C][C], and the diagonal index."""
    N, Cn = h.shape
    h_lower = (np.repeat(h, Cn, 0) - eps32).astype(F32)
    h_upper = (np.repeat(h, Cn, 0) + eps32).astype(F32)
    row, diag = np.arange(N * Cn), np.tile(np.arange(Cn), N)
    up, lo = h_upper[row, diag].copy(), h_lower[row, diag].copy()
    h_lower[row, diag], h_upper[row, diag] = up, lo
    lower_lb, lower_ub = barrier_lo(h_lower, cfg), barrier_lo(h_upper, cfg)
    ft_lb, ft_ub = np.repeat(ub, Cn, 0).astype(F32), np.repeat(lb, Cn, 0).astype(F32)
    ubd, lbd = ft_lb[row, diag].copy(), ft_ub[row, diag].copy()
    ft_lb[row, diag], ft_ub[row, diag] = lbd, ubd
    return lower_lb, ft_lb, lower_ub, ft_ub, (row, diag)


@dataclass
class CrownImage:
    bounds: Bounds            # float64, before ibp_sigmoid
    eta: np.ndarray           # [G][C] float32
    f_lb: np.ndarray          # [G][C] float32
    f_ub: np.ndarray
    viol: np.ndarray          # [G] float32 (Vdot + kappa)
    slices: List[Tuple[int, int]]
    out: np.ndarray           # [nb] float32 per-batch maximum
    exit_iters: np.ndarray    # [nb][2]


def device_slices(G: int, batches: int) -> List[Tuple[int, int]]:
    """fiode_certify's partition (cert.hip batch_of): the last batch runs to G."""
    ebs = G // batches
    nb = batches + (1 if G % batches else 0)
    return [(b * ebs, (b + 1) * ebs if b < nb - 1 else G) for b in range(nb)]


def kappa_of(eps_cfg: float, min_std: float) -> float:
    """certify_crown.py:65-67: sqrt(2) * (1 / min std) * eps -- no alpha_1 factor."""
    return math.sqrt(2) * (1.0 / min_std) * eps_cfg


def crown_image(x_feat: np.ndarray, label: int, counts: np.ndarray, P: O.DynParams, cfg: O.DynConfig, T: int,
                batches: int, eps_cfg: float = 0.141, min_std: float = 0.225,
                slices: Optional[Sequence[Tuple[int, int]]] = None, bounds: Optional[Bounds] = None) -> CrownImage:
    """certify_crown.py:129-153 for one image without the early exit: every batch is evaluated."""
    counts = np.asarray(counts)
    G = len(counts)
    eta = O.db_grid_for_label(counts.astype(np.int64), label, T)
    eps = 1.0 / T
    eps32 = F32(eps)
    if bounds is None:
        bounds = crown_bounds(net_of(P, x_feat), eta, eps)
    lb, ub = bounds.lb.astype(F32), bounds.ub.astype(F32)
    if cfg.scale_nominal:
        lb, ub = ibp_sigmoid(lb, ub, (eta - eps32).astype(F32), (eta + eps32).astype(F32), cfg)
    if slices is None:
        slices = device_slices(G, batches)
    kappa = F32(kappa_of(eps_cfg, min_std))
    f_lb, f_ub = np.zeros((G, 10), F32), np.zeros((G, 10), F32)
    viol = np.full(G, np.nan, F32)
    outs, exits = np.zeros(len(slices), F32), np.zeros((len(slices), 2), np.int64)
    for b, (lo, hi) in enumerate(slices):
        h = eta[lo:hi]
        lower_lb, ft_lb, lower_ub, ft_ub, (row, diag) = ibp_cbf_qp_problems(h, eps32, lb[lo:hi], ub[lo:hi], cfg)
        q_lb = O.qp_forward(lower_lb, ft_lb, cfg.qp_max_iter, cfg.qp_tol)
        q_ub = O.qp_forward(lower_ub, ft_ub, cfg.qp_max_iter, cfg.qp_tol)
        f_lb[lo:hi] = q_lb.v[row, diag].reshape(hi - lo, -1)
        f_ub[lo:hi] = q_ub.v[row, diag].reshape(hi - lo, -1)
        exits[b] = (q_lb.iters, q_ub.iters)
        wrong = h >= (h.max(1, keepdims=True) - F32(2 * eps)).astype(F32)          # certify_crown.py:144-147
        wrong[:, label] = False
        f_wrong = np.where(wrong, f_ub[lo:hi], -np.inf).max(1).astype(F32)
        vdot = ((-f_lb[lo:hi, label]).astype(F32) + f_wrong).astype(F32)           # perturbed_vdot, :29-34
        viol[lo:hi] = (vdot + kappa).astype(F32)
        outs[b] = viol[lo:hi].max()
    return CrownImage(bounds=bounds, eta=eta, f_lb=f_lb, f_ub=f_ub, viol=viol, slices=list(slices), out=outs,
                      exit_iters=exits)
