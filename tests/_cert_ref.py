"""Per-row reference of the certification pass (fiode_certify) for an arbitrary count grid.

``cert_rows`` restates ``oracle.fiode_oracle.certify_image`` (float64 matmuls, every float32 cast
of the oracle kept) and keeps what that function reduces away: the violation of every row, the
slices, and per batch the oracle's QP exit iteration, the two maxima and the rows that attain
them.  The grid is any uint8 ``[G][10]`` array of counts in 0..T: rows need not lie on the simplex
or on the decision boundary, and may repeat.

Cost: the MLP, the barrier and the nominal are computed once per unique row and gathered; the QP
runs per batch (its exit is the first iteration at which EVERY row of the batch meets the
tolerance), through ``O.qp_forward`` on the set of distinct rows of the batch: every step of
``qp_forward`` but the ``ok.all()`` of the exit is row-wise, and ``all`` over a multiset equals
``all`` over its set, so a repeated row changes nothing.  (tests/test_cert_ref.py checks this
against ``O.certify_image`` on a grid with repeats.)
"""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from oracle import fiode_oracle as O
from tests import _groupsort_ref as GS

F32 = np.float32


@dataclass
class CertRows:
    viol: np.ndarray          # [G] float32 violation of every row (NaN: in no slice)
    violT: np.ndarray         # [G] float32 violation_larger_T
    slices: List[Tuple[int, int]]
    exit_iters: np.ndarray    # [nb] the oracle's QP exit iteration of each batch
    vmax: np.ndarray          # [nb] float32 max viol of the batch
    vtmax: np.ndarray         # [nb] float32 max violT
    argmax: np.ndarray        # [nb] first row (global index) that attains vmax
    argmaxT: np.ndarray       # [nb] ... vtmax
    conv: np.ndarray          # [G] uint32: bit i set iff the row alone meets the QP tolerance at iteration i
    inv: np.ndarray           # [G] index of each row among the grid's distinct rows
    eps_u: Optional[np.ndarray] = None   # trace=True: [U][max_iter] the QP's eps of each distinct row at each iteration

    @property
    def out(self) -> np.ndarray:
        """[nb][2], the layout of ops.certify_image's first result."""
        return np.stack([self.vmax, self.vtmax], 1)


def device_slices(G: int, batches: int) -> List[Tuple[int, int]]:
    """The device's partition (cert.hip batch_of): batch b = min(r // ebs, nb - 1), so the last batch
    always runs to G.  Equal to O.certify_batches(G, batches) iff G % batches <= G // batches."""
    ebs = G // batches
    nb = batches + (1 if G % batches else 0)
    return [(b * ebs, (b + 1) * ebs if b < nb - 1 else G) for b in range(nb)]


def row_keys(counts: np.ndarray, T: int) -> np.ndarray:
    """One uint64 per row, injective for counts <= T <= 64 (base T + 1 digits)."""
    k = np.zeros(len(counts), np.uint64)
    for j in range(counts.shape[1]):
        k = k * np.uint64(T + 1) + counts[:, j].astype(np.uint64)
    return k


def qp_eps_trace(lower: np.ndarray, nominal: np.ndarray, max_iter: int) -> np.ndarray:
    """eps = sum v of every row at every iteration of O.qp_convergence_masks' loop (each row's
    bisection path is its own): [N][max_iter] float32."""
    mu_ceil = (nominal - lower).astype(F32).max(axis=1)
    mu_floor = nominal.min(axis=1)
    out = np.zeros((len(nominal), max_iter), F32)
    for i in range(max_iter):
        mu = ((mu_ceil - mu_floor).astype(F32) / F32(2) + mu_floor).astype(F32)
        v = np.maximum((nominal - mu[:, None]).astype(F32), lower)
        eps = O.row_sum_seq(v)
        out[:, i] = eps
        mu_floor = np.where(eps > 0, mu, mu_floor).astype(F32)
        mu_ceil = np.where(eps < 0, mu, mu_ceil).astype(F32)
    return out


def cert_rows(counts: np.ndarray, label: int, x_feat: np.ndarray, P: O.DynParams, cfg: O.DynConfig, T: int,
              batches: int, activation: str = "relu", eps: float = 0.141, min_std: float = 0.225,
              slices: Optional[Sequence[Tuple[int, int]]] = None, trace: bool = False) -> CertRows:
    counts = np.asarray(counts)
    assert counts.dtype == np.uint8 and counts.ndim == 2 and counts.shape[1] == 10
    G = len(counts)
    assert G > 0 and int(counts.max()) <= T <= 64, "every count must lie in 0..T (the kernel's eta table has T + 1 entries)"
    mlp_forward = {"relu": O.mlp_forward, "groupsort": GS.mlp_forward}[activation]
    cc = O.CertifyConst(T=T, eps_cfg=eps, min_std=min_std, batches=batches)
    if slices is None:
        slices = O.certify_batches(G, batches)

    # ---- once per unique row: eta, MLP, barrier, nominal (O.eval_dot up to the QP) ---------------
    _, first, inv = np.unique(row_keys(counts, T), return_index=True, return_inverse=True)
    uniq = counts[first]
    eta = O.db_grid_for_label(uniq.astype(np.int64), label, T)
    u = O.static_projection(np.asarray(x_feat, F32).reshape(1, -1), P)
    ft = mlp_forward(eta, np.repeat(u, len(eta), 0), P, None, None, 0.0)["ftilde"]
    lower = O.barrier_lower(eta, cfg)
    if cfg.scale_nominal:
        nominal, _ = O.scale_nominal(ft, lower, O.barrier_upper(eta, cfg))
    else:
        nominal = ft
    # ---- the terms of the violation that do not depend on f (O.certify_image) --------------------
    eps_g = F32(1.0 / T)
    dist = F32(math.sqrt(cc.n) / T)
    kappa = F32(cc.kappa(cfg))
    ub = (eta.max(1) + eps_g).astype(F32)
    lf = ((F32(math.sqrt(cc.n)) * (F32(cfg.sigma_1 * cfg.alpha_1) * np.exp(F32(cfg.sigma_1) * ub).astype(F32)))
          .astype(F32) + F32(1)).astype(F32)
    perturb = ((F32(math.sqrt(2)) * lf).astype(F32) * dist).astype(F32)
    wrong = eta == eta.max(1, keepdims=True)
    wrong[:, label] = False
    conv = O.qp_convergence_masks(lower, nominal, cfg.qp_max_iter, cfg.qp_tol)
    eps_u = None
    if trace:
        eps_u = qp_eps_trace(lower, nominal, cfg.qp_max_iter)
        bits = ((np.abs(eps_u) < F32(cfg.qp_tol)).astype(np.uint32) << np.arange(cfg.qp_max_iter, dtype=np.uint32)).sum(1)
        assert np.array_equal(bits.astype(np.uint32), conv)

    viol = np.full(G, np.nan, F32)
    violT = np.full(G, np.nan, F32)
    nb = len(slices)
    exits = np.zeros(nb, np.int64)
    vmax, vtmax = np.zeros(nb, F32), np.zeros(nb, F32)
    amax, amaxT = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    pos = np.zeros(len(uniq), np.int64)
    for b, (lo, hi) in enumerate(slices):
        assert 0 <= lo < hi <= G
        ib = inv[lo:hi]
        ub_ = np.unique(ib)                                   # the distinct rows of this batch
        qp = O.qp_forward(lower[ub_], nominal[ub_], cfg.qp_max_iter, cfg.qp_tol)
        f = qp.v
        fw = np.where(wrong[ub_], f, -np.inf).max(1).astype(F32)
        hv = ((-f[:, label]).astype(F32) + fw).astype(F32)
        v_u = ((hv + perturb[ub_]).astype(F32) + kappa).astype(F32)
        vt_u = (hv + kappa).astype(F32)
        pos[ub_] = np.arange(len(ub_))
        viol[lo:hi] = v_u[pos[ib]]
        violT[lo:hi] = vt_u[pos[ib]]
        exits[b] = qp.iters
        vmax[b], vtmax[b] = viol[lo:hi].max(), violT[lo:hi].max()
        amax[b], amaxT[b] = lo + int(viol[lo:hi].argmax()), lo + int(violT[lo:hi].argmax())
    return CertRows(viol=viol, violT=violT, slices=list(slices), exit_iters=exits, vmax=vmax, vtmax=vtmax,
                    argmax=amax, argmaxT=amaxT, conv=conv[inv], inv=inv, eps_u=eps_u)


# ---- the multi-round synthetic grid with planted maxima (test_gpu_certify_batches.py) ------------
# k_cert_fwd and k_cert_final are persistent: on the real T <= 12 grids every wave makes one trip, so
# the per-wave accumulators (cur_b / cur_and, acc0 / acc1) never switch batch and never flush in
# mid-loop.  This grid has G = 2 R + 4133 rows, R = 8 * ncu * 256 = one round of k_cert_final (four
# rounds of k_cert_fwd):
#   * one planted row per batch carries the batch's maximum of viol AND of violT, above every other
#     row of the batch by >= MARGIN = 10 x the 2e-3 comparison tolerance: a planted row that is lost
#     (or counted in the neighbouring batch) costs >= 2e-2 and cannot hide behind a repeat;
#   * the planted rows of even and odd batches differ by >= MARGIN too, so a maximum that leaks
#     from an odd batch into an even one shows as well;
#   * even batches are "easy" (exit t_easy), odd ones "hard" (exit t_hard >= t_easy + 3), so an exit
#     AND that leaks into a neighbouring batch moves that batch's exit by more than the +-1 the
#     comparison allows;
#   * the exit of a hard batch hangs on ONE row, its pin: every other row of the batch (the planted
#     one included) meets the tolerance at t_easy already, so a kernel that loses the pin's
#     contribution to the AND (a flush dropped at a batch switch, a lane dropped in and_by_batch)
#     makes the batch exit >= 3 iterations early.  The pins sit where the paths differ: in a
#     64-row pair inside the batch whose k_cert_fwd wave later lands in another batch (flush at
#     the switch), in one whose wave makes no later trip (flush after the loop), and in a pair
#     that straddles a batch boundary (and_by_batch).
# The exits are made to hold on BOTH sides of the comparison.  A batch exits at the first iteration
# at which every row has |eps| < tol (1e-4).  At iteration k a row's |eps| is what is left of a
# bracket halved k times, so by k ~ 13 a typical |eps| is itself ~1e-4 and whether a given row meets
# the tolerance at a given iteration can hang on the last bits of the MLP output, where the device
# (float32 MFMA accumulation) and the reference (float64 matmuls) differ.  A first design, whose
# easy batches were rows that merely met the tolerance at one iteration in the reference, exited at
# 13 there and at 17 on the MI355X, with the same 17 when the batch was certified alone (so not a
# leak between batches; that edge rows flipped is inferred from this, not traced row by row).  So:
#   - an easy batch (exit t) is built from rows with |eps_t| <= tol / 2 and |eps_k| >= tol / 2 at
#     every k < t (neither the bit at t nor the branch taken earlier hangs on the last bits), one
#     of them, the easy pin, with |eps_k| >= 3 tol / 2 at every k < t;
#   - a hard batch is built from such rows for t = t_easy that have |eps| <= tol / 2 at t_hard too
#     and |eps_k| >= tol / 4 at every k < t_hard, plus an easy pin, plus the hard pin:
#     |eps_k| >= 3 tol / 2 at every k < t_hard, |eps| <= tol / 2 at t_hard.
# Both then exit at exactly t for any implementation whose eps is within tol / 4 = 2.5e-5 of the
# reference's.  The device's is: eps sums ten terms nominal_j - mu of magnitude <= 20, each within
# a few float32 ulps (2e-6) of the reference's (the MLP's 128-term float32 dot products give
# ~sqrt(128) 2^-24 relative; measured end to end: the violations agree within 1 ulp), i.e. ~1e-5.
# Bulk and planted rows are unique rows of the T = 12 grid.  The hard pins are not: no row of that
# grid stays 3 tol / 2 open up to an iteration by which a usable set of grid rows has met the
# tolerance twice, so they are drawn from rows of arbitrary counts <= T (N_EXTRA seeded draws).
MARGIN = 2e-2            # 10 x the suite's 2e-3
BULK_GAP = 0.05          # bulk rows lie this far below their batch's planted row on the pool's one-batch run
SYN_T, SYN_LABEL, SYN_BATCHES = 12, 3, 10
SYN_PARAM_SEED, SYN_X_SEED = 52, 12
N_EXTRA, EXTRA_SEED = 8000, 3


@dataclass
class PlantedGrid:
    counts: np.ndarray        # [G][10] uint8
    R: int                    # rows of one k_cert_final round
    ebs: int
    planted: np.ndarray       # [nb] global row index of each batch's planted row
    lanes: dict               # lane -> planted row that sits on that lane of a boundary-straddling pair
    pins: np.ndarray          # [nb] global row index of each batch's easy pin (open before t_easy)
    hard_pins: dict           # odd batch -> global row index of the pin its exit hangs on
    t_easy: int
    t_hard: int


def synthetic_inputs():
    from tests._util import make_params
    return make_params(seed=SYN_PARAM_SEED), np.random.default_rng(SYN_X_SEED).normal(size=10).astype(F32)


def _all_before(m: np.ndarray) -> np.ndarray:
    """out[r, t] = m[r, :t].all()"""
    return np.concatenate([np.ones((len(m), 1), bool), np.cumprod(m, axis=1).astype(bool)[:, :-1]], 1)


def robust_sets(eps_u: np.ndarray, tol: float):
    """closed[r, t]: |eps_t| <= tol / 2 and |eps_k| >= tol / 2 at every k < t (no earlier iteration
    leaves the sign of eps, and with it the row's bisection path, to the last bits);
    pin[r, t]: closed at t and |eps_k| >= 3 tol / 2 for all k < t."""
    a = np.abs(eps_u.astype(np.float64))
    closed = (a <= 0.5 * tol) & _all_before(a >= 0.5 * tol)
    return closed, closed & _all_before(a >= 1.5 * tol)


def twice_closed(eps_u: np.ndarray, tol: float, t_lo: int, t_hi: int) -> np.ndarray:
    """Rows closed (robust_sets) at t_lo that meet the tolerance again at t_hi, with tol / 2 to spare
    there and |eps_k| >= tol / 4 at every k < t_hi."""
    a = np.abs(eps_u.astype(np.float64))
    return robust_sets(eps_u, tol)[0][:, t_lo] & (a[:, t_hi] <= 0.5 * tol) & (a[:, :t_hi] >= 0.25 * tol).all(1)


def straddles(r: int, ebs: int, nb: int, G: int) -> bool:
    """Row r's 64-row pair holds rows of two batches."""
    g0 = r // 64 * 64
    return min(g0 // ebs, nb - 1) != min(min(g0 + 63, G - 1) // ebs, nb - 1)


def planted_grid(ncu: int, cfg: O.DynConfig, activation: str = "relu", seed: int = 7) -> PlantedGrid:
    """Build the grid for a device with ``ncu`` compute units (see the block comment above).  The
    conditions it aims at are ASSERTED by check_planted on the reference of the built grid; this
    function only chooses rows by the pool's own one-batch reference run."""
    T, label, batches = SYN_T, SYN_LABEL, SYN_BATCHES
    tol = cfg.qp_tol
    P, x = synthetic_inputs()
    grid = O.db_grid_rows(10, T).astype(np.uint8)
    NG = len(grid)
    extra = np.random.default_rng(EXTRA_SEED).integers(0, T + 1, (N_EXTRA, 10)).astype(np.uint8)
    pool = np.concatenate([grid, extra])
    pr = cert_rows(pool, label, x, P, cfg, T, 1, activation=activation, trace=True)
    eps = pr.eps_u[pr.inv]
    closed, pin = robust_sets(eps, tol)
    on_grid = np.arange(len(pool)) < NG
    rng = np.random.default_rng(seed)

    def below(rows, p):
        return rows[(pr.viol[rows] <= pr.viol[p] - BULK_GAP) & (pr.violT[rows] <= pr.violT[p] - BULK_GAP)
                    & np.isfinite(pr.viol[rows]) & np.isfinite(pr.violT[rows])]

    def choose(rows, t_pin, away_from=None, hard_pin_at=None):
        """(planted row, bulk rows, easy pin, hard pin or None) from the grid rows ``rows``, or None."""
        if len(rows) < 64:
            return None
        deficit = np.minimum(pr.viol[rows] - pr.viol[rows].max(), pr.violT[rows] - pr.violT[rows].max())
        cand = rows[np.argsort(-deficit)]
        if away_from is not None:
            cand = cand[(np.abs(pr.viol[cand] - pr.viol[away_from]) >= BULK_GAP)
                        & (np.abs(pr.violT[cand] - pr.violT[away_from]) >= BULK_GAP)]
        for p in cand[:64]:
            bulk = below(rows, p)
            pins = bulk[pin[bulk, t_pin]]
            hp = below(np.flatnonzero(pin[:, hard_pin_at]), p) if hard_pin_at is not None else [None]
            if len(bulk) >= 32 and len(pins) and len(hp):
                return int(p), bulk, int(pins[0]), hp[0]
        return None

    hard = easy = None
    for t_hard in range(cfg.qp_max_iter - 1, 2, -1):         # the latest exit that a pin row holds
        if not pin[:, t_hard].any():
            continue
        for gap in (4, 3):
            t_easy = t_hard - gap
            hard = choose(np.flatnonzero(on_grid & twice_closed(eps, tol, t_easy, t_hard)), t_easy, hard_pin_at=t_hard)
            easy = choose(np.flatnonzero(on_grid & closed[:, t_easy]), t_easy, away_from=hard[0]) if hard else None
            if easy is not None:
                break
        if easy is not None:
            break
    assert hard is not None and easy is not None, "no pair of robust exits"

    R = 8 * ncu * 256
    G = 2 * R + 4133
    ebs = G // batches
    sl = device_slices(G, batches)
    nb = len(sl)
    idx = np.empty(G, np.int64)
    for b, (lo, hi) in enumerate(sl):
        src = (easy if b % 2 == 0 else hard)[1]
        idx[lo:hi] = src[rng.integers(0, len(src), hi - lo)]

    # planted positions.  A 64-row group that straddles a batch boundary takes the kernels' direct
    # path (and_by_batch / max_by_batch); every other group goes through the register accumulators,
    # which are flushed when the wave's next trip lands in another batch.  So besides the positions
    # at the boundaries, three planted rows sit inside a batch, in a group whose wave makes a later
    # trip: two in the first round of k_cert_final, one at the start of the second.
    planted = np.full(nb, -1, np.int64)
    for b in (0, 1):
        planted[b] = rng.integers(sl[b][0] + 64, sl[b][1] - 64)
    bR = (R + 100) // ebs
    planted[bR] = R + 100                                   # second round; its wave's third trip is row 2 R + 100
    planted[6] = sl[6][0]                                   # first row of a batch
    planted[7] = sl[7][1] - 1                               # last row of a batch
    planted[nb - 1] = sl[nb - 1][0] + (sl[nb - 1][1] - sl[nb - 1][0]) // 2        # in the tail
    last_pair = G - G % 64
    planted[nb - 2] = max(last_pair, sl[nb - 2][0]) + 1 if last_pair + 1 < sl[nb - 2][1] else sl[nb - 2][1] - 2
    lanes = {}
    for L in (0, 31, 32, 63):                               # lanes of a pair that straddles a boundary
        for k in range(1, nb - 1):
            s = (k * ebs) % 64
            bt = k - 1 if L < s else k
            if s == 0 or planted[bt] >= 0:
                continue
            planted[bt] = lanes[L] = k * ebs - s + L
            break
    for b in range(nb):
        if planted[b] < 0:
            planted[b] = rng.integers(sl[b][0] + 64, sl[b][1] - 64)
    pins = np.zeros(nb, np.int64)
    hard_pins = {}
    for b, (lo, hi) in enumerate(sl):
        p, _, q, hq = easy if b % 2 == 0 else hard
        idx[planted[b]] = p
        pins[b] = lo + (hi - lo) // 3
        pins[b] += 1 if pins[b] == planted[b] else 0
        idx[pins[b]] = q
        if b % 2 == 1:
            if b % 4 == 3:                                  # in the pair that straddles the batch's first boundary
                r = next(r for r in range(lo, lo + 64) if straddles(r, ebs, nb, G) and r != planted[b])
            else:                                           # inside the batch
                r = lo + 2 * (hi - lo) // 3
                r += 1 if r == planted[b] else 0
            idx[r] = hq
            hard_pins[b] = r
    return PlantedGrid(counts=np.ascontiguousarray(pool[idx]), R=R, ebs=ebs, planted=planted, lanes=lanes,
                       pins=pins, hard_pins=hard_pins, t_easy=t_easy, t_hard=t_hard)


def check_planted(pg: PlantedGrid, ref: CertRows, ncu: int, tol: float = 1e-4, max_iter: int = 30) -> dict:
    """The construction conditions of the planted grid, on the reference (trace=True) of the built
    grid.  Returns the figures (smallest margins, exits, gap)."""
    G = len(pg.counts)
    assert G == 2 * pg.R + 4133 and int(pg.counts.max()) <= SYN_T
    assert ref.slices == device_slices(G, SYN_BATCHES) == O.certify_batches(G, SYN_BATCHES)
    nb = len(ref.slices)
    assert nb == SYN_BATCHES + 1 and G % 64 != 0
    closed, pin = robust_sets(ref.eps_u, tol)
    twice = twice_closed(ref.eps_u, tol, pg.t_easy, pg.t_hard)
    conv_u = np.zeros(len(ref.eps_u), np.uint32)
    conv_u[ref.inv] = ref.conv
    margins = np.zeros((nb, 2))
    exits_without_pin = {}
    for b, (lo, hi) in enumerate(ref.slices):
        p = int(pg.planted[b])
        assert lo <= p < hi
        for c, q in enumerate((ref.viol, ref.violT)):
            rest = np.delete(q[lo:hi], p - lo)
            margins[b, c] = float(q[p]) - float(rest.max())
        assert ref.argmax[b] == p and ref.argmaxT[b] == p
        # the exit holds with room to spare (see the block comment)
        rows = np.unique(ref.inv[lo:hi])
        assert lo <= pg.pins[b] < hi and pin[ref.inv[pg.pins[b]], pg.t_easy]
        if b % 2 == 0:
            assert ref.exit_iters[b] == pg.t_easy and closed[rows, pg.t_easy].all()
        else:
            hp = int(pg.hard_pins[b])
            u = ref.inv[hp]
            assert lo <= hp < hi and pin[u, pg.t_hard] and int((ref.inv[lo:hi] == u).sum()) == 1
            rest = rows[rows != u]
            assert ref.exit_iters[b] == pg.t_hard and twice[rest].all()
            # ... and hangs on the pin alone: without it the batch exits >= 3 iterations earlier
            exits_without_pin[b] = O.global_exit_iteration(conv_u[rest], max_iter)
            assert exits_without_pin[b] <= pg.t_hard - 3
    assert margins.min() >= MARGIN, margins
    # neighbouring batches' maxima differ by the margin too
    step = np.abs(np.diff(ref.out.astype(np.float64), axis=0))
    assert step.min() >= MARGIN, step
    gaps = np.abs(np.diff(ref.exit_iters))
    assert gaps.min() >= 3, ref.exit_iters
    # positions
    sl, pl = ref.slices, pg.planted
    assert any(pl[b] == sl[b][0] for b in range(nb)) and any(pl[b] == sl[b][1] - 1 for b in range(nb))
    assert sorted(pg.lanes) == [0, 31, 32, 63]
    for L, r in pg.lanes.items():
        assert r % 64 == L and r in pl and straddles(r, pg.ebs, nb, G), "pair does not straddle a boundary"
    assert any(r >= G - G % 64 for r in pl[:nb - 1]) and sl[nb - 1][0] <= pl[nb - 1] < G
    assert sl[nb - 1][1] - sl[nb - 1][0] == G % SYN_BATCHES < 64
    assert any(pg.R <= r < 2 * pg.R for r in pl) and any(r >= 2 * pg.R for r in pl)

    def batch(r):
        return min(r // pg.ebs, nb - 1)

    def accumulated(r, stride):
        """r's 64-row group lies in one batch (register path) and its wave (a persistent loop of
        ``stride`` rows per round) makes a later full trip, in another batch: what the group
        contributes reaches the batch's word only through the flush at the switch."""
        g0 = r // 64 * 64
        return not straddles(r, pg.ebs, nb, G) and g0 + 63 + stride < G and batch(g0 + stride) != batch(r)

    assert sum(accumulated(r, pg.R) for r in pl if r < pg.R) >= 2 and any(accumulated(r, pg.R) for r in pl if r >= pg.R)
    fwd_round = 2 * ncu * 4 * 64                              # rows of one k_cert_fwd round
    assert any(r >= fwd_round for r in pl) and G > 8 * fwd_round
    hp = list(pg.hard_pins.values())
    assert sum(accumulated(r, fwd_round) for r in hp) >= 2                      # flush at the batch switch
    assert any(not straddles(r, pg.ebs, nb, G) and r // 64 * 64 + fwd_round >= G for r in hp)   # flush after the loop
    assert sum(straddles(r, pg.ebs, nb, G) for r in hp) >= 2                    # and_by_batch
    return dict(margin_viol=float(margins[:, 0].min()), margin_violT=float(margins[:, 1].min()),
                exits=ref.exit_iters.tolist(), exits_without_pin=exits_without_pin, min_exit_gap=int(gaps.min()),
                min_step=float(step.min()))
