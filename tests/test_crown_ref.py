"""CPU checks of the numpy CROWN reference tests/_crown_ref.py (what the GPU tests compare with)."""
import functools

import numpy as np

from oracle import fiode_oracle as O
from tests import _crown_ref as R
from tests._util import make_params

T, LABEL = 6, 3


@functools.lru_cache(maxsize=None)
def _case():
    P = make_params(seed=0)
    x = np.random.default_rng(1).normal(size=10).astype(np.float32)
    counts = O.db_grid_rows(10, T).astype(np.uint8)
    eta = O.db_grid_for_label(counts.astype(np.int64), LABEL, T)
    net = R.net_of(P, x)
    return P, x, counts, eta, net, R.crown_bounds(net, eta, 1.0 / T)


def test_bounds_are_sound_on_sampled_points():
    """200 points per box, half of them corners: the float64 MLP lies inside [lb, ub] (and the layer-2
    pre-activations inside [l2, u2])."""
    _, _, _, eta, net, b = _case()
    pts = R.sample_box(eta, 1.0 / T, 200, np.random.default_rng(2)).reshape(-1, 10)
    f = net.forward(pts).reshape(len(eta), 200, 10)
    z2 = (np.maximum(pts @ net.W1.T + net.u, 0) @ net.W2.T + net.b2).reshape(len(eta), 200, -1)
    assert ((f >= b.lb[:, None] - 1e-12) & (f <= b.ub[:, None] + 1e-12)).all()
    assert ((z2 >= b.l2[:, None] - 1e-12) & (z2 <= b.u2[:, None] + 1e-12)).all()
    assert (b.lb <= b.ub).all() and (b.l2 <= b.u2).all()


def test_crown_is_not_interval_arithmetic():
    _, _, _, eta, net, b = _case()
    il, iu = R.interval_bounds(net, eta, 1.0 / T)
    w_crown, w_ibp = float((b.ub - b.lb).mean()), float((iu - il).mean())
    print(f"mean width CROWN {w_crown:.4f} interval {w_ibp:.4f} ratio {w_ibp / w_crown:.1f}")
    assert 5 * w_crown <= w_ibp
    assert (b.lb >= il - 1e-9).all() and (b.ub <= iu + 1e-9).all()       # never looser, row by row


def test_both_hidden_layers_have_unstable_units():
    """The relaxation is exercised: a share of the units of both layers is unstable in every row."""
    _, _, _, _, _, b = _case()
    for l, u in ((b.l1, b.u1), (b.l2, b.u2)):
        share = ((l < 0) & (u > 0)).mean(1)
        assert share.min() > 0.1 and share.max() < 0.9, (share.min(), share.max())


def test_bounds_collapse_at_zero_radius():
    _, _, _, eta, net, _ = _case()
    b = R.crown_bounds(net, eta, 0.0)
    f = net.forward(eta)
    assert np.abs(b.lb - f).max() <= 1e-12 and np.abs(b.ub - f).max() <= 1e-12


def test_hand_worked_case():
    """1 -> 2 -> 2 -> 1, eta0 = 0, eps = 1; one unstable unit per hidden layer, the other stable.
    Layer 1: z1 = (eta + 0.5, eta + 3) in ([-0.5, 1.5], [2, 4]): unit 0 has s = 0.75, t = 0.375,
    alpha = 1 (1.5 > 0.5).  Layer 2: z2 = (a0 - a1 + 2.4, a0 + a1).
      u2_0 = 0.75 * 0.5 - 3 + |0.75 - 1| + 0.375 + 2.4 = 0.4,  l2_0 = 0.5 - 3 - |1 - 1| + 2.4 = -0.1
      u2_1 = 0.375 + 3 + 1.75 + 0.375 = 5.5,                   l2_1 = 0.5 + 3 - 2 = 1.5
    so unit 0 is unstable: s2 = 0.8, t2 = 0.08, alpha2 = 1.  Output a2_0 + a2_1:
      Lambda^U = (0.8, 1), Q^U = (1.8, 0.2), R^U = (1.35, 0.2):
        ub = (0.675 + 0.6) + 1.55 + 1.8 * 0.375 + 0.8 * 2.4 + 0.08 = 5.5   (attained at eta = 1)
      Lambda^L = (1, 1), Q^L = (2, 0), R^L = (2, 0):
        lb = 1 - 2 + 0 + 2.4 + 0 = 1.4                                      (true minimum 2.4)."""
    net = R.Net(W1=np.array([[1.0], [1.0]]), u=np.array([0.5, 3.0]), W2=np.array([[1.0, -1.0], [1.0, 1.0]]),
                b2=np.array([2.4, 0.0]), W3=np.array([[1.0, 1.0]]), b3=np.array([0.0]))
    b = R.crown_bounds(net, np.zeros((1, 1)), 1.0)
    assert np.allclose(b.l1, [[-0.5, 2.0]], atol=1e-12) and np.allclose(b.u1, [[1.5, 4.0]], atol=1e-12)
    assert np.allclose(b.l2, [[-0.1, 1.5]], atol=1e-12) and np.allclose(b.u2, [[0.4, 5.5]], atol=1e-12)
    assert np.allclose(b.lb, [[1.4]], atol=1e-12) and np.allclose(b.ub, [[5.5]], atol=1e-12)
    grid = net.forward(np.linspace(-1, 1, 2001)[:, None])
    assert b.lb[0, 0] <= grid.min() and abs(grid.max() - 5.5) <= 1e-12


def test_relaxation_tie_gives_zero_lower_slope():
    s, t, al = R.relu_relaxation(np.array([-1.0, -1.0, -1.0, 0.0, -2.0]), np.array([1.0, 1.0 + 1e-9, 1.0 - 1e-9, 2.0, 0.0]))
    assert al.tolist() == [0.0, 1.0, 0.0, 1.0, 0.0]
    assert np.allclose(s, [0.5, 0.5, 0.5, 1.0, 0.0]) and np.allclose(t, [0.5, 0.5, 0.5, 0.0, 0.0])


def test_two_product_form_equals_four_product_form():
    _, _, _, eta, net, b = _case()
    h = R.crown_bounds(net, eta, 1.0 / T, form="half")
    for name in ("l2", "u2", "lb", "ub"):
        assert np.abs(getattr(h, name) - getattr(b, name)).max() <= 1e-12, name


def test_tie_distances_and_share_of_rows_near_a_tie():
    _, _, _, _, _, b = _case()
    assert np.array_equal(b.tie1, np.abs(b.u1 + b.l1).min(1)) and np.array_equal(b.tie2, np.abs(b.u2 + b.l2).min(1))
    near = int((np.minimum(b.tie1, b.tie2) < 1e-5).sum())
    print("rows within 1e-5 of a tie:", near, "of", len(b.tie1))
    assert near <= 0.02 * len(b.tie1)


def test_qp_problems_follow_the_reference_construction():
    """ibp_cbf_qp (classification.py:210-231): problem i of a row has h + eps and lb at i, h - eps and ub
    elsewhere (lower-bound call), and the mirror image for the upper-bound call."""
    cfg = O.DynConfig()
    rng = np.random.default_rng(3)
    h = rng.uniform(0, 1, (4, 10)).astype(np.float32)
    lb = rng.normal(size=(4, 10)).astype(np.float32)
    ub = (lb + rng.uniform(0, 1, (4, 10))).astype(np.float32)
    e = np.float32(0.125)
    lower_lb, ft_lb, lower_ub, ft_ub, (row, diag) = R.ibp_cbf_qp_problems(h, e, lb, ub, cfg)
    for r in range(4):
        for i in range(10):
            hl, hu = h[r] - e, h[r] + e
            hl[i], hu[i] = h[r, i] + e, h[r, i] - e
            p = 10 * r + i
            assert np.array_equal(lower_lb[p], R.barrier_lo(hl, cfg)) and np.array_equal(lower_ub[p], R.barrier_lo(hu, cfg))
            want_lb, want_ub = ub[r].copy(), lb[r].copy()
            want_lb[i], want_ub[i] = lb[r, i], ub[r, i]
            assert np.array_equal(ft_lb[p], want_lb) and np.array_equal(ft_ub[p], want_ub)
            assert (row[p], diag[p]) == (p, i)


def test_lower_bound_call_never_meets_the_tolerance():
    """The reference's behaviour, restated and not repaired: grid rows have zero
    coordinates, eta - eps < 0 there, the barrier lower bound is positive, the sub-problem infeasible,
    so the lower-bound solver call runs to qp_max_iter - 1 in every batch; the upper-bound call exits."""
    P, x, counts, _, _, b = _case()
    for sn in (True, False):
        im = R.crown_image(x, LABEL, counts, P, O.DynConfig(scale_nominal=sn), T, 10, bounds=b)
        assert im.slices[-1] == (420, 423) and len(im.out) == 11
        assert (im.exit_iters[:, 0] == 29).all()
        assert (im.exit_iters[:, 1] < 29).all() and (im.exit_iters[:, 1] >= 10).all()
        assert np.isfinite(im.out).all() and np.array_equal(im.out, [im.viol[lo:hi].max() for lo, hi in im.slices])
