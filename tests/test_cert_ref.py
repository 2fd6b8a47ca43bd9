"""CPU checks of tests/_cert_ref.py: the per-row reference reproduces O.certify_image bit for bit,
and the synthetic multi-round grid of test_gpu_certify_batches.py meets its construction conditions
(planted maxima, their margins and positions, exit gaps) for the seeds that test uses -- on the
256 compute units of the MI355X, so the conditions are known to hold before a device is touched."""
import numpy as np
import pytest

from oracle import fiode_oracle as O
from tests import _cert_ref as CR
from tests import _groupsort_ref as GS
from tests._util import make_params


def _case(T):
    return make_params(seed=40 + T), np.random.default_rng(T).normal(size=10).astype(np.float32)


@pytest.mark.parametrize("label", [0, 6])
@pytest.mark.parametrize("scale_nominal", [True, False])
def test_helper_reproduces_certify_image_T8(label, scale_nominal):
    T = 8
    P, x = _case(T)
    grid_v = O.db_grid_rows(10, T)
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    vmax, vtmax = O.certify_image(x, label, grid_v, P, cfg, O.CertifyConst(T=T, batches=10))
    r = CR.cert_rows(grid_v.astype(np.uint8), label, x, P, cfg, T, 10)
    assert r.out.dtype == np.float32 and r.out.shape == (len(vmax), 2)
    assert np.array_equal(r.vmax, vmax) and np.array_equal(r.vtmax, vtmax)
    assert r.slices == O.certify_batches(len(grid_v), 10) == CR.device_slices(len(grid_v), 10)
    # per-row output: the maxima are attained where argmax says, every row lies in a slice
    assert not np.isnan(r.viol).any() and not np.isnan(r.violT).any()
    for b, (lo, hi) in enumerate(r.slices):
        assert lo <= r.argmax[b] < hi and r.viol[r.argmax[b]] == vmax[b] and r.violT[r.argmaxT[b]] == vtmax[b]
        # the exit is the oracle's own on that slice's rows
        eta = O.db_grid_for_label(grid_v, label, T)[lo:hi]
        u = np.repeat(O.static_projection(x.reshape(1, -1), P), hi - lo, 0)
        assert r.exit_iters[b] == O.eval_dot(eta, u, P, cfg).qp.iters
        assert r.exit_iters[b] == O.global_exit_iteration(r.conv[lo:hi], cfg.qp_max_iter)


def test_helper_groupsort_reproduces_certify_image(monkeypatch):
    T, label = 8, 2
    P, x = _case(T)
    grid_v = O.db_grid_rows(10, T)
    cfg = O.DynConfig(scale_nominal=True)
    relu = CR.cert_rows(grid_v.astype(np.uint8), label, x, P, cfg, T, 10)
    gs = CR.cert_rows(grid_v.astype(np.uint8), label, x, P, cfg, T, 10, activation="groupsort")
    monkeypatch.setattr(O, "mlp_forward", GS.mlp_forward)
    vmax, vtmax = O.certify_image(x, label, grid_v, P, cfg, O.CertifyConst(T=T, batches=10))
    assert np.array_equal(gs.vmax, vmax) and np.array_equal(gs.vtmax, vtmax)
    assert np.abs(gs.viol - relu.viol).max() > 2e-2          # the two activations are told apart


def test_helper_on_repeated_off_simplex_rows():
    """Any counts <= T: rows off the simplex, off the decision boundary, and repeated (the QP of a
    batch runs on its distinct rows only; O.certify_image runs it on all of them)."""
    T, label = 7, 4
    P, x = _case(T)
    rng = np.random.default_rng(5)
    base = rng.integers(0, T + 1, (40, 10)).astype(np.uint8)
    counts = base[rng.integers(0, 40, 333)]
    assert int(counts.max()) == T and len(np.unique(counts, axis=0)) <= 40
    for scale_nominal in (True, False):
        cfg = O.DynConfig(scale_nominal=scale_nominal)
        vmax, vtmax = O.certify_image(x, label, counts.astype(np.int64), P, cfg, O.CertifyConst(T=T, batches=10))
        r = CR.cert_rows(counts, label, x, P, cfg, T, 10)
        assert len(r.slices) == 11 and np.array_equal(r.vmax, vmax) and np.array_equal(r.vtmax, vtmax)


def test_helper_rejects_counts_above_T():
    P, x = _case(8)
    counts = np.zeros((4, 10), np.uint8)
    counts[2, 5] = 9
    with pytest.raises(AssertionError):
        CR.cert_rows(counts, 0, x, P, O.DynConfig(), 8, 1)


def test_device_partition_against_reference_partition():
    """Aligned (G % batches <= G // batches): the same slices.  Otherwise the reference's last slice
    stops at (b + 1) * ebs and leaves the remaining rows out; the device's runs to G."""
    for G, batches in [(1839, 10), (16086, 63), (16086, 64), (16086, 100), (1839, 61), (423, 20)]:
        assert G % batches <= G // batches
        assert CR.device_slices(G, batches) == O.certify_batches(G, batches)
    G, batches = 423, 50
    assert len(O.db_grid_rows(10, 6)) == G and G // batches == 8 and G % batches == 23
    dev, ref = CR.device_slices(G, batches), O.certify_batches(G, batches)
    assert dev[:-1] == ref[:-1] and ref[-1] == (400, 408) and dev[-1] == (400, 423)
    # the helper takes the device's partition: the extra rows are evaluated
    P, x = _case(6)
    counts = O.db_grid_rows(10, 6).astype(np.uint8)
    r_dev = CR.cert_rows(counts, 1, x, P, O.DynConfig(), 6, batches, slices=dev)
    r_ref = CR.cert_rows(counts, 1, x, P, O.DynConfig(), 6, batches)
    assert np.isnan(r_ref.viol[408:]).all() and not np.isnan(r_dev.viol).any()
    assert np.array_equal(r_dev.out[:-1], r_ref.out[:-1])


@pytest.mark.parametrize("activation", ["relu", "groupsort"])
@pytest.mark.parametrize("scale_nominal", [True, False])
def test_planted_grid_conditions(scale_nominal, activation):
    ncu = 256
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    P, x = CR.synthetic_inputs()
    pg = CR.planted_grid(ncu, cfg, activation)
    assert len(pg.counts) == 1_052_709 and pg.ebs == 105_270
    ref = CR.cert_rows(pg.counts, CR.SYN_LABEL, x, P, cfg, CR.SYN_T, CR.SYN_BATCHES, activation=activation, trace=True)
    fig = CR.check_planted(pg, ref, ncu)
    print("planted grid", activation, scale_nominal, fig)
    assert ref.slices[-1] == (1_052_700, 1_052_709)
    # 3 rounds of k_cert_final (8 * ncu * 256 rows each), 9 of k_cert_fwd (2 * ncu * 4 * 64)
    assert -(-len(pg.counts) // pg.R) == 3 and -(-len(pg.counts) // (2 * ncu * 4 * 64)) == 9
    assert pg.t_hard - pg.t_easy >= 3 and ref.exit_iters.tolist() == [pg.t_easy, pg.t_hard] * 5 + [pg.t_easy]


def test_planted_grid_other_cu_count():
    """The builder follows the device's CU count (here 304): the same conditions hold."""
    cfg = O.DynConfig(scale_nominal=True)
    P, x = CR.synthetic_inputs()
    pg = CR.planted_grid(304, cfg, "relu")
    ref = CR.cert_rows(pg.counts, CR.SYN_LABEL, x, P, cfg, CR.SYN_T, CR.SYN_BATCHES, trace=True)
    CR.check_planted(pg, ref, 304)
