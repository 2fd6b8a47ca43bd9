"""CPU checks of the numpy GroupSort CROWN reference tests/_crown_gs_ref.py (what the GPU tests compare
with): soundness on sampled points, exactness where the net is linear, the forms, and the tie census of
the GPU cases."""
import functools

import numpy as np
import pytest

from oracle import fiode_oracle as O
from tests import _crown_gs_ref as G
from tests import _crown_ref as R
from tests import _groupsort_ref as GS
from tests._util import make_params

LABEL = G.GPU_LABEL
ROUND = 1e-12            # float64 rounding of the sums, as tests/test_crown_ref.py


@functools.lru_cache(maxsize=None)
def _eta(T):
    counts = O.db_grid_rows(10, T).astype(np.uint8)
    return O.db_grid_for_label(counts.astype(np.int64), LABEL, T)


@functools.lru_cache(maxsize=None)
def _case(T):
    """The GPU case of this T: (eta, net, bounds); computed once, never modified."""
    net = G.net_of(make_params(seed=G.GPU_PARAM_SEED), G.features(G.GPU_FEATURE_SEED[T]))
    return _eta(T), net, G.crown_bounds(net, _eta(T), 1.0 / T)


def test_forward_is_the_project_groupsort():
    """Net.forward pairs (i, i + 64) as tests/_groupsort_ref.py, and max = z[H:] + r, min = z[:H] - r."""
    z = np.random.default_rng(0).normal(size=(7, 128))
    assert np.array_equal(G.groupsort(z).astype(np.float32), GS.groupsort(z))
    d = z[:, :64] - z[:, 64:]
    r = np.maximum(d, 0)
    assert np.abs(G.groupsort(z) - np.concatenate([z[:, 64:] + r, z[:, :64] - r], 1)).max() <= 1e-15
    P = make_params(seed=0)
    x = G.features(5)
    eta = _eta(6)[:9]
    ref = GS.mlp_forward(eta.astype(np.float32), (P.Qx @ x + P.bx).astype(np.float32)[None], P, None, None, 0.0)
    assert np.abs(G.net_of(P, x).forward(eta.astype(np.float32)) - ref["ftilde"]).max() <= 1e-5


@pytest.mark.parametrize("T", [6, 8])
def test_bounds_enclose_the_net_on_sampled_points(T):
    """200 points per box, half of them corners: d1, d2 and the outputs of the float64 net lie inside
    their bounds, with no violation at all."""
    eta, net, b = _case(T)
    pts = G.sample_box(eta, 1.0 / T, 200, np.random.default_rng(2)).reshape(-1, 10)
    f = net.forward(pts).reshape(len(eta), 200, 10)
    d1, d2 = (d.reshape(len(eta), 200, -1) for d in net.differences(pts))
    for name, v, lo, hi in (("d1", d1, b.l1, b.u1), ("d2", d2, b.l2, b.u2), ("out", f, b.lb, b.ub)):
        bad = int(((v < lo[:, None] - ROUND) | (v > hi[:, None] + ROUND)).sum())
        assert bad == 0, (name, bad)
    assert (b.lb <= b.ub).all() and (b.l2 <= b.u2).all() and (b.l1 <= b.u1).all()
    assert b.l1.shape == b.l2.shape == (len(eta), 64)            # 64 specification rows, not 128


def test_both_layers_have_unstable_pairs():
    for T in (6, 8):
        _, _, b = _case(T)
        for l, u in ((b.l1, b.u1), (b.l2, b.u2)):
            assert ((l < 0) & (u > 0)).sum(1).min() >= 2


def test_exact_where_the_net_is_linear():
    """eps so small that every pair of both layers keeps its order on the whole box (asserted): the net is
    linear there and the bounds are centre -+ eps |row|_1 of that linear map."""
    eta, net, _ = _case(6)
    eps = 1e-7
    b = G.crown_bounds(net, eta, eps)
    assert (((b.l1 > 0) | (b.u1 < 0)) & ((b.l2 > 0) | (b.u2 < 0))).all()
    z1, z2 = net.hidden(eta)

    def select(z):
        """[n][M][M] matrices Pi with GroupSort(z') = Pi z' while the order of every pair is that of z"""
        first = z[:, :64] > z[:, 64:]
        n, i = len(z), np.arange(64)
        Pi = np.zeros((n, 128, 128))
        Pi[:, i, i] = first
        Pi[:, i, i + 64] = ~first
        Pi[:, i + 64, i + 64] = first
        Pi[:, i + 64, i] = ~first
        return Pi
    J = net.W3[None] @ select(z2) @ net.W2[None] @ select(z1) @ net.W1[None]
    f, rad = net.forward(eta), eps * np.abs(J).sum(2)
    for got, want in ((b.lb, f - rad), (b.ub, f + rad)):
        assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), float(np.abs(got - want).max())
    assert rad.min() > 1e-9                                       # the radius is not lost in the comparison


def test_bounds_collapse_at_zero_radius():
    eta, net, _ = _case(6)
    b = G.crown_bounds(net, eta, 0.0)
    f = net.forward(eta)
    d1, d2 = net.differences(eta)
    assert np.abs(b.lb - f).max() <= ROUND and np.abs(b.ub - f).max() <= ROUND
    assert max(np.abs(b.l2 - d2).max(), np.abs(b.u2 - d2).max(), np.abs(b.l1 - d1).max(), np.abs(b.u1 - d1).max()) <= ROUND


@pytest.mark.parametrize("T", [6, 8])
def test_never_looser_than_interval_arithmetic(T):
    eta, net, b = _case(T)
    il2, iu2, il, iu = G.interval_bounds(net, eta, 1.0 / T)
    assert (b.lb >= il - 1e-9).all() and (b.ub <= iu + 1e-9).all()
    assert (b.l2 >= il2 - 1e-9).all() and (b.u2 <= iu2 + 1e-9).all()
    w_crown, w_ibp = float((b.ub - b.lb).mean()), float((iu - il).mean())
    print(f"T={T}: mean width CROWN {w_crown:.4f} interval {w_ibp:.4f}")
    assert 5 * w_crown <= w_ibp
    # and the interval bounds are themselves sound, so the comparison is with a valid enclosure
    pts = G.sample_box(eta, 1.0 / T, 20, np.random.default_rng(4)).reshape(-1, 10)
    f = net.forward(pts).reshape(len(eta), 20, 10)
    assert ((f >= il[:, None]) & (f <= iu[:, None])).all()


def test_two_product_form_equals_four_product_form():
    eta, net, b = _case(6)
    h = G.crown_bounds(net, eta, 1.0 / 6, form="half")
    for name in ("l2", "u2", "lb", "ub"):
        assert np.abs(getattr(h, name) - getattr(b, name)).max() <= ROUND, name


def test_mispaired_units_break_enclosure():
    """The reference with the relaxation on the pairs (i, i + 1) instead of (i, i + 64) does not enclose
    the net: the pairing is checked by the enclosure test, not assumed."""
    eta, net, b = _case(6)
    m = G.crown_bounds(net, eta, 1.0 / 6, pairs="adjacent")
    f = net.forward(G.sample_box(eta, 1.0 / 6, 50, np.random.default_rng(3)).reshape(-1, 10)).reshape(len(eta), 50, 10)
    excess = max(float((m.lb[:, None] - f).max()), float((f - m.ub[:, None]).max()))
    assert excess > 0.1, excess
    assert max(float((b.lb[:, None] - f).max()), float((f - b.ub[:, None]).max())) <= ROUND


def test_groupsort_and_relu_bounds_differ():
    eta, net, b = _case(6)
    r = R.crown_bounds(net, eta, 1.0 / 6)
    scale = float(np.abs(b.ub).max())
    assert np.abs(r.ub - b.ub).max() > 0.1 * scale and np.abs(r.lb - b.lb).max() > 0.1 * scale


@pytest.mark.parametrize("T", [6, 8])
def test_gpu_cases_are_tie_free(T):
    """No row of a GPU case is within TIE (the ReLU test's margin, at unit feature scale) of the lower
    slope's tie u = -l on either layer, so tests/test_gpu_certify_crown_gs.py compares every row."""
    _, _, b = _case(T)
    margin = min(float(b.tie1.min()), float(b.tie2.min()))
    print(f"T={T}: min |u_d + l_d| over both layers and all rows {margin:.3e}")
    assert margin >= G.TIE
