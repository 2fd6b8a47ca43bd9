"""Batch bookkeeping of the certification kernels (cert.hip) beyond one round of their persistent
loops, against the per-row reference tests/_cert_ref.py.

The real T <= 12 grids (test_gpu_certify.py) give every wave of k_cert_fwd / k_cert_final exactly
one trip, so the register accumulators that follow a wave from batch to batch (cur_b / cur_and,
acc0 / acc1) never flush in mid-loop there.  Here:

1. a synthetic grid of G = 2 R + 4133 rows (R = 8 * ncu * 256: 3 rounds of k_cert_final, 9 of
   k_cert_fwd on 256 CUs), 11 batches, with one planted maximum per batch and QP exits that
   alternate between batches (construction and its CPU-checked conditions: tests/_cert_ref.py);
2. on that grid, bit-for-bit: a batch certified alone equals its entry of the full run, and
   permuting the rows inside each batch changes nothing (the MLP column of a row does not depend
   on its lane, the QP runs per lane, the exit is an AND, the result a max);
3. the real grids with 1, 64, 65 and 101 batches (k_cert_decode beyond one 64-thread block) and
   with 30-row batches (a wave spans three or four batches), and a grid whose remainder exceeds
   the batch size (the device's last batch runs to G; the reference's stops short).

Tolerances: per-batch maxima 2e-3 absolute (derivation: test_gpu_certify.py); exit iterations
within 1 of the oracle's (the rule of test_dyn_eval_matches_oracle: a row at the tolerance's edge
may meet it one bisection step apart under the MFMA and the float64 MLP).  The planted margins
(>= 2e-2) and the exit gaps (>= 3) are ten and three times those, so a lost row, a lost flush or an
AND that leaks into the neighbouring batch cannot pass; the exit of every odd batch hangs on one
pin row (without it the batch exits 4 iterations early), placed where k_cert_fwd flushes at a batch
switch, after its loop, or through and_by_batch.  Checked by seeding each of four bugs into
cert.hip on the MI355X, every one of which fails test_planted_maxima_multi_round:
k_cert_final without the flush at a batch switch (planted maxima missed by 0.06 to 0.31);
k_cert_fwd without the reset of cur_and at a switch (exits of batches 2..8 four too late);
k_cert_fwd without the atomicAnd at a switch (batches 1 and 5 exit 4 early);
and_by_batch serving only the first batch of a pair (batches 3 and 7 exit 4 early, the tail at 0).

Measured on the MI355X (256 CUs, G = 1,052,709), synthetic grid: max error 7.6e-6 (scale_nominal;
1 ulp of 92) and 4.8e-7 (without); exits oracle = device in all 11 batches: 14 / 18 (ReLU and
GroupSort, scale_nominal), 12 / 16 (both, without), 14 resp. 12 in the odd batches without their
pin; planted margins 0.072, 0.117, 0.051, 0.050.  Real grids: max error 5.3e-5, exits within 1.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _cert_ref as CR
from tests._util import make_params

pytestmark = pytest.mark.gpu

ACT = {"relu": "ReLU", "groupsort": "GroupSort"}
TOL = 2e-3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


def _poison(dev, nb):
    """ops.certify_image allocates its results with torch.empty: leave NaN / INT_MIN in the blocks
    the caching allocator will most likely hand out next, so an entry the kernels never write is
    seen for certain rather than by the luck of what the memory held.  (Best effort: whatever the
    blocks hold, the assertions below reject an unwritten entry unless it happens to be right.)"""
    a = torch.full((nb, 2), float("nan"), dtype=torch.float32, device=dev)
    b = torch.full((nb,), torch.iinfo(torch.int32).min, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    del a, b


def _run(dev, grid, x, label, P, scale_nominal, activation, T, batches):
    from fiode_amd import ops
    if not torch.is_tensor(grid):
        grid = torch.from_numpy(np.ascontiguousarray(grid)).to(dev)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}
    G = grid.shape[0]
    xd = torch.from_numpy(x).to(dev)                  # every other allocation before the poisoned blocks are freed
    _poison(dev, batches + (1 if G % batches else 0))
    out, it = ops.certify_image(xd, label, grid, w,
                                ops.DynCfg(scale_nominal=scale_nominal, dropout=0.0, activation=ACT[activation]),
                                T=T, batches=batches)
    return out.cpu().numpy(), it.cpu().numpy()


def _compare(out, it, ref, what):
    """out at 2e-3, exits within 1; prints the figures first."""
    assert out.shape == ref.out.shape and it.shape == ref.exit_iters.shape, (out.shape, it.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(out.astype(np.float64) - ref.out.astype(np.float64))
    dit = np.abs(it.astype(np.int64) - ref.exit_iters)
    nb = len(dit)
    print(f"{what}: max err viol {np.nanmax(err[:, 0]):.3e} violT {np.nanmax(err[:, 1]):.3e} (bound {TOL}); "
          f"exit oracle {ref.exit_iters.tolist() if nb <= 16 else (int(ref.exit_iters.min()), int(ref.exit_iters.max()))} "
          f"device {it.tolist() if nb <= 16 else (int(it.min()), int(it.max()))} max |diff| {int(dit.max())}")
    assert np.isfinite(out).all(), np.flatnonzero(~np.isfinite(out).all(1))
    assert (err <= TOL).all(), (np.argwhere(err > TOL)[:8].tolist(), float(err.max()))
    assert (dit <= 1).all(), (np.flatnonzero(dit > 1)[:8].tolist(), it.tolist(), ref.exit_iters.tolist())


# ---- 1. the multi-round synthetic grid ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _synthetic(ncu, scale_nominal, activation):
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    P, x = CR.synthetic_inputs()
    pg = CR.planted_grid(ncu, cfg, activation)
    ref = CR.cert_rows(pg.counts, CR.SYN_LABEL, x, P, cfg, CR.SYN_T, CR.SYN_BATCHES, activation=activation, trace=True)
    fig = CR.check_planted(pg, ref, ncu)          # the construction conditions, on the CPU
    return pg, ref, fig, P, x


def _ncu(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.mark.parametrize("activation", ["relu", "groupsort"])
@pytest.mark.parametrize("scale_nominal", [True, False])
def test_planted_maxima_multi_round(scale_nominal, activation):
    dev = _dev()
    pg, ref, fig, P, x = _synthetic(_ncu(dev), scale_nominal, activation)
    print("planted grid:", len(pg.counts), "rows, margins / exits", fig)
    out, it = _run(dev, pg.counts, x, CR.SYN_LABEL, P, scale_nominal, activation, CR.SYN_T, CR.SYN_BATCHES)
    assert out.shape == (11, 2)
    _compare(out, it, ref, f"synthetic {activation} scale_nominal={scale_nominal}")


# ---- 2. exact decomposition and permutation -------------------------------------------------------
CASES_EXACT = [(True, "relu"), (False, "groupsort")]


@pytest.mark.parametrize("scale_nominal,activation", CASES_EXACT)
def test_batch_alone_equals_its_entry_of_the_full_run(scale_nominal, activation):
    dev = _dev()
    pg, ref, _, P, x = _synthetic(_ncu(dev), scale_nominal, activation)
    grid = torch.from_numpy(pg.counts).to(dev)
    args = (x, CR.SYN_LABEL, P, scale_nominal, activation, CR.SYN_T)
    out, it = _run(dev, grid, *args, CR.SYN_BATCHES)
    nb = len(ref.slices)
    for b in (0, 5, nb - 1):                                   # first, a middle hard batch, the tail
        lo, hi = ref.slices[b]
        o1, i1 = _run(dev, grid[lo:hi].clone(), *args, 1)
        assert o1.shape == (1, 2)
        assert np.array_equal(o1[0], out[b]) and int(i1[0]) == int(it[b]), (b, o1, out[b], i1, it[b])
    assert ref.exit_iters[5] >= ref.exit_iters[0] + 3


@pytest.mark.parametrize("scale_nominal,activation", CASES_EXACT)
def test_permutation_inside_batches_changes_nothing(scale_nominal, activation):
    dev = _dev()
    pg, ref, _, P, x = _synthetic(_ncu(dev), scale_nominal, activation)
    args = (x, CR.SYN_LABEL, P, scale_nominal, activation, CR.SYN_T, CR.SYN_BATCHES)
    out, it = _run(dev, pg.counts, *args)
    rng = np.random.default_rng(31)
    perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in ref.slices])
    assert not np.array_equal(perm, np.arange(len(perm)))
    out_p, it_p = _run(dev, pg.counts[perm], *args)
    assert np.array_equal(out_p, out) and np.array_equal(it_p, it), (out_p - out, it_p, it)


# ---- 3. batch counts on the real grids ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real_grid(T):
    return O.db_grid_rows(10, T).astype(np.uint8)


@pytest.mark.parametrize("scale_nominal", [True, False])
@pytest.mark.parametrize("T,batches,activation", [(12, 1, "relu"), (12, 63, "relu"), (12, 64, "relu"), (12, 100, "relu"),
                                                  (8, 61, "relu"), (8, 61, "groupsort"), (12, 64, "groupsort")])
def test_batch_counts_on_real_grids(T, batches, activation, scale_nominal):
    """(12, 63) -> 64 batches, (12, 64) -> 65: k_cert_decode's second block.  (8, 61): ebs = 30."""
    dev = _dev()
    counts = _real_grid(T)
    G = len(counts)
    assert G % batches <= G // batches                          # reference, oracle and device slices coincide
    P, x, label = make_params(seed=40 + T), np.random.default_rng(T).normal(size=10).astype(np.float32), 3
    ref = CR.cert_rows(counts, label, x, P, O.DynConfig(scale_nominal=scale_nominal), T, batches, activation=activation)
    assert ref.slices == CR.device_slices(G, batches)
    out, it = _run(dev, counts, x, label, P, scale_nominal, activation, T, batches)
    assert out.shape == (batches + (1 if G % batches else 0), 2)
    _compare(out, it, ref, f"T={T} batches={batches} {activation} scale_nominal={scale_nominal}")


def test_last_batch_runs_to_G_when_remainder_exceeds_batch_size():
    """T = 6: G = 423, batches = 50: ebs = 8, remainder 23 > ebs.  The reference's last slice is
    [400, 408) and rows 408..422 are never evaluated; the device's last batch is [400, 423)
    (conservative: a superset).  Pinned against the helper on the device's partition."""
    dev = _dev()
    T, batches, label = 6, 50, 1
    counts = _real_grid(T)
    G = len(counts)
    assert (G, G // batches, G % batches) == (423, 8, 23)
    sl = CR.device_slices(G, batches)
    assert sl[-1] == (400, 423) and O.certify_batches(G, batches)[-1] == (400, 408)
    P, x = make_params(seed=40 + T), np.random.default_rng(T).normal(size=10).astype(np.float32)
    for scale_nominal in (True, False):
        cfg = O.DynConfig(scale_nominal=scale_nominal)
        ref = CR.cert_rows(counts, label, x, P, cfg, T, batches, slices=sl)
        out, it = _run(dev, counts, x, label, P, scale_nominal, "relu", T, batches)
        _compare(out, it, ref, f"T=6 batches=50 scale_nominal={scale_nominal} (device partition)")
