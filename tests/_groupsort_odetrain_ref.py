"""Reference of the GroupSort rk4 train_ode solve (test_groupsort_odetrain.py,
test_gpu_groupsort_odetrain.py).

``make_eval_dot`` restates ``oracle.torch_ref.eval_dot`` (same signature, same QP, same pins ``act`` /
``mu``) with ``activation = GroupSort()`` (classification.py:96-102): per hidden layer d = z * (keep *
1 / (1 - p)) and a = cat(maximum(d[:, :64], d[:, 64:]), minimum(d[:, :64], d[:, 64:])).  Tests install
it with ``monkeypatch.setattr(T, "eval_dot", make_eval_dot(...))``; ``T.ode_train_loss`` calls the
module-level ``eval_dot`` once per f-eval, so it then runs a GroupSort solve and nothing under
oracle/ changes.  The function counts its calls: call e is eval e of the solve.

Optional per-eval pinned pair codes (``order`` / ``tie``, bool [B, E, 2, 64]: row, eval, hidden layer,
pair u = units (u, u + 64)): the sort becomes a fixed routing, max output = the first member where
``order`` else the second, min output the other one, and on a pinned tie both outputs are the half sum
d[u] / 2 + d[u + 64] / 2.  Its gradient is then the device's routing rule (the member that held the
larger value takes g_max, the other g_min, a tie gives both g_max / 2 + g_min / 2) at the device's
codes, so a float64 run checks a float32 backward elementwise although GroupSort's gradient jumps
where a pair flips.  Pinning a run's own codes (``pair_codes``) changes nothing: a tie's half sum of
two equal values is the value, and torch.maximum / minimum split a tie's gradient in half.

The numpy forward is ``tests/_groupsort_train_ref.mlp_forward`` monkeypatched into
``oracle.fiode_oracle`` (``O.rk4_train`` then runs GroupSort), as the Lyapunov-step tests do.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_ref as T
from tests._util import make_params

HALF = 64
KEYS = ("Q1", "b1", "Qx", "bx", "Q2", "b2", "Q3", "b3")

# The GPU cases (B, step_size, scale_nominal, dropout p, seed) over ts = [0, 1], P = make_params(seed),
# inputs from ``make_case``.  One full tile with E = 8; one row (15 idle lanes); three tiles with a
# partial last one (the cross-tile exit exchange in use); nine tiles at a B that ReLU sends to the
# 4-row kernels; dropout off.  test_groupsort_odetrain.py checks two conditions on each on the CPU: the
# near-tie census, and that the two references (float64 torch, float32-per-op numpy) agree on every
# stage input within MAX_REFERENCE_SPREAD, half the 2e-4 the device is held to.  The second decides
# which cases run with scale_nominal: at step 0.5 the sigmoid-scaled nominal makes the stages
# sensitive enough that the references themselves differ by 2e-4 .. 5e-4 at B = 16 and 130 (one
# bisection step of the batch-global QP exit moves a stage derivative), so those two run without it
# and B = 1 and 37 with it.
CASES = [(16, 0.5, False, 0.5, 1016), (1, 0.5, True, 0.5, 1001), (37, 0.25, True, 0.5, 1037),
         (130, 0.5, False, 0.5, 1130), (16, 0.5, False, 0.0, 1216)]
MAX_REFERENCE_SPREAD = 1e-4


def n_evals(step, t0=0.0, t1=1.0):
    """Evals of the rk4 solve: 4 (niters - 1), niters = ceil((t1 - t0) / step + 1) in float32."""
    f = np.float32
    return 4 * (int(math.ceil(float((f(t1) - f(t0)) / f(step) + f(1)))) - 1)


def make_case(B, step, p, seed):
    """(P, x [B,10], h0 [B,10], labels [B], masks [E,2,B,128] uint8 or None) of a case."""
    P = make_params(seed=seed)
    rng = np.random.default_rng(seed + 7)
    x = rng.normal(size=(B, 10)).astype(np.float32)
    h0 = np.full((B, 10), 0.1, np.float32)
    labels = rng.integers(0, 10, B)
    E = n_evals(step)
    masks = (rng.random((E, 2, B, 128)) >= p).astype(np.uint8) if p > 0 else None
    return P, x, h0, labels, masks


def _sort(d, order=None, tie=None):
    a, b = d[:, :HALF], d[:, HALF:]
    if order is None:
        return torch.cat([torch.maximum(a, b), torch.minimum(a, b)], dim=1)
    half = a / 2 + b / 2
    mx = torch.where(tie, half, torch.where(order, a, b))
    mn = torch.where(tie, half, torch.where(order, b, a))
    return torch.cat([mx, mn], dim=1)


def make_eval_dot(order=None, tie=None, record=None):
    """An ``eval_dot`` with T.eval_dot's signature.  ``order`` / ``tie``: pinned pair codes
    [B, E, 2, 64] bool (None: the sort).  ``record`` (a list) receives per eval the detached dropped
    values (d1, d2) [B, 128], the keep masks (m1, m2) the sorts ordered, and the stage input h."""
    calls = [0]

    def eval_dot(h, x_rows, W, alpha_1, alpha_2, sigma_1, scale_nominal, mask1=None, mask2=None, p=0.5,
                 stash=None, act=None, mu=None):
        e = calls[0]
        calls[0] += 1
        pin = (lambda l: (order[:, e, l], tie[:, e, l])) if order is not None else (lambda l: (None, None))
        d1 = F.linear(h, W["Q1"], W["b1"]) + F.linear(x_rows, W["Qx"], W["bx"])
        if mask1 is not None:
            d1 = d1 * (mask1.to(d1.dtype) * (1.0 / (1.0 - p)))
        a = _sort(d1, *pin(0))
        d2 = F.linear(a, W["Q2"], W["b2"])
        if mask2 is not None:
            d2 = d2 * (mask2.to(d2.dtype) * (1.0 / (1.0 - p)))
        a = _sort(d2, *pin(1))
        if record is not None:
            record.append((d1.detach().clone(), d2.detach().clone(), mask1, mask2, h.detach().clone()))
        ft = F.linear(a, W["Q3"], W["b3"])
        lower = -alpha_1 * (torch.exp(sigma_1 * h) - 1)
        upper = alpha_2 * (1 - h)
        if scale_nominal:
            ft = (upper - lower) * torch.sigmoid(ft) + lower
        if stash is not None:
            stash["lower"] = lower.detach().clone()
            stash["nominal"] = ft.detach().clone()
        if act is not None:
            return T._PinnedActiveSet.apply(lower, ft, act, mu)
        return T._NoUpperProjection.apply(lower, ft)
    return eval_dot


def pair_codes(record):
    """(order, tie, live, sep) [B, E, 2, 64] of a recorded run: d[u] > d[u + 64], d[u] == d[u + 64],
    the pairs that are not both dropped, and |d[u] - d[u + 64]|."""
    o, t, lv, sp = [], [], [], []
    for d1, d2, m1, m2, _ in record:
        oo, tt, ll, ss = [], [], [], []
        for d, m in ((d1, m1), (d2, m2)):
            a, b = d[:, :HALF], d[:, HALF:]
            oo.append(a > b)
            tt.append(a == b)
            ss.append((a - b).abs())
            ll.append(torch.ones_like(a, dtype=torch.bool) if m is None else
                      ((m[:, :HALF] != 0) | (m[:, HALF:] != 0)))
        o.append(torch.stack(oo, 1)); t.append(torch.stack(tt, 1)); lv.append(torch.stack(ll, 1)); sp.append(torch.stack(ss, 1))
    return tuple(torch.stack(v, 1) for v in (o, t, lv, sp))


def solve_with_grads(monkeypatch, P, x, h0, labels, masks, step, scale_nominal, p, *, acts=None, mus=None,
                     order=None, tie=None):
    """float64 ``T.ode_train_loss`` of the GroupSort solve and its autograd gradients.  Returns
    (loss, y_hat, grads incl. 'x_feat', record)."""
    record = []
    monkeypatch.setattr(T, "eval_dot", make_eval_dot(order, tie, record))
    leaves = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).double().requires_grad_(True) for k in KEYS}
    xf = torch.from_numpy(x).double().requires_grad_(True)
    loss, yy = T.ode_train_loss(xf, torch.from_numpy(h0).double(), torch.from_numpy(labels), leaves,
                                None if masks is None else torch.from_numpy(masks), 0.0, 1.0, step,
                                scale_nominal=scale_nominal, p=p, acts=acts, mus=mus)
    loss.backward()
    grads = {k: leaves[k].grad for k in KEYS}
    grads["x_feat"] = xf.grad
    return loss.detach(), yy.detach(), grads, record
