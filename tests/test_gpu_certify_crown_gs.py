"""GPU parity of the GroupSort CROWN certification path (fiode_certify_crown_act, k_crown_bounds_gs of
crown.hip) against the float64 numpy reference tests/_crown_gs_ref.py.

Grids (the smallest that still exercise the kernel):
  T = 6    423 rows, 10 batches: 42-row batches and a 3-row tail (an odd row count: a wave tile holds two
           rows, so the last tile is half empty);
  T = 8    1,839 rows, 61 batches: 30-row batches, a 9-row tail.
Features: unit-scale N(0, 1) draws whose grids have no row within 1e-5 of a slope tie on either layer
(tests/_crown_gs_ref.py GPU_FEATURE_SEED, asserted on the host by tests/test_crown_gs_ref.py), so every row
is compared.

Tolerances: those of tests/test_gpu_certify_crown.py (the same math at the same widths).
  * bounds lb, ub and the bounds l2, u2 of the layer-2 pair differences: 2e-5 of the array's maximum;
  * f_lb, f_ub and the per-batch maxima: 2e-3 absolute;
  * exits: the upper-bound call within 1 iteration; the lower-bound call equal where the reference's call
    never meets the tolerance (exit qp_max_iter - 1) and within 1 where it converges;
  * device soundness: the device GroupSort MLP on 40 points per box (half of them corners) lies inside the
    device's [lb, ub] with slack 2e-5 of max(1, the largest bound).

Measured on the MI355X: bounds, largest error as a fraction of the array's maximum: l2 6.3e-7, u2 8.3e-7,
lb 6.9e-7, ub 6.0e-7; f within 6.2e-5 (T = 6) / 1.9e-4 (T = 8), out within 4.4e-5 / 7.3e-5; exits device =
reference in every batch (T = 6: lower call 29, upper 18 with scale_nominal, 17 without; T = 8: lower 16-17 /
13-14, upper 17-18 / 17); device soundness: worst excess -3.0e-2 (inside).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _crown_gs_ref as G
from tests import _crown_ref as R
from tests._util import make_params

pytestmark = pytest.mark.gpu

TOL_MLP, TOL_CERT = 2e-5, 2e-3
LABEL = G.GPU_LABEL
H = 64


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _counts(T):
    return O.db_grid_rows(10, T).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _params():
    return make_params(seed=G.GPU_PARAM_SEED)


@functools.lru_cache(maxsize=None)
def _x(T):
    return G.features(G.GPU_FEATURE_SEED[T])


@functools.lru_cache(maxsize=None)
def _bounds(T):
    """The float64 bounds of the case: computed once, shared, never modified."""
    eta = O.db_grid_for_label(_counts(T).astype(np.int64), LABEL, T)
    return G.crown_bounds(G.net_of(_params(), _x(T)), eta, 1.0 / T)


def _weights(dev):
    from fiode_amd import ops
    P = _params()
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}


def _run(dev, counts, x, label, scale_nominal, T, batches, activation="GroupSort", **kw):
    from fiode_amd import ops
    grid = torch.from_numpy(np.ascontiguousarray(counts)).to(dev)
    with ops.groupsort_crown():
        res = ops.certify_crown_image(torch.from_numpy(x).to(dev), label, grid, _weights(dev),
                                      ops.DynCfg(scale_nominal=scale_nominal, dropout=0.0, activation=activation),
                                      T=T, batches=batches, **kw)
    return [r.cpu().numpy() if torch.is_tensor(r) else {k: v.cpu().numpy() for k, v in r.items()} for r in res]


# ---- 1. bounds, QP stage, batch maxima, exits ----------------------------------------------------------
@pytest.mark.parametrize("scale_nominal", [True, False])
@pytest.mark.parametrize("T", [6, 8])
def test_matches_float64_reference(T, scale_nominal):
    dev = _dev()
    batches = G.GPU_BATCHES[T]
    ref_b = _bounds(T)
    assert min(float(ref_b.tie1.min()), float(ref_b.tie2.min())) >= G.TIE
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    ref = R.crown_image(_x(T), LABEL, _counts(T), _params(), cfg, T, batches, bounds=ref_b)
    out, it, dbg = _run(dev, _counts(T), _x(T), LABEL, scale_nominal, T, batches, debug=True)
    for name in ("l2", "u2"):
        assert np.isnan(dbg[name][:, H:]).all(), name             # columns 64..127 are not written
        dbg[name] = dbg[name][:, :H]
    for name in ("l2", "u2", "lb", "ub"):
        d, r = dbg[name].astype(np.float64), getattr(ref_b, name)
        assert d.shape == r.shape and np.isfinite(d).all(), (name, np.argwhere(~np.isfinite(d))[:4].tolist())
        scale = float(np.abs(r).max())
        err = float(np.abs(d - r).max())
        print(f"T={T} scale_nominal={scale_nominal} {name}: max err {err:.3e} = {err / scale:.3e} of max |{name}| = "
              f"{scale:.4f} (bound {TOL_MLP})")
        assert err <= TOL_MLP * scale, (name, err, scale)
    assert out.shape == ref.out.shape and it.shape == ref.exit_iters.shape
    e_f = max(float(np.abs(dbg["f_lb"] - ref.f_lb).max()), float(np.abs(dbg["f_ub"] - ref.f_ub).max()))
    e_o = float(np.abs(out.astype(np.float64) - ref.out).max())
    print(f"T={T} scale_nominal={scale_nominal}: max err f {e_f:.3e} out {e_o:.3e} (bound {TOL_CERT}); "
          f"exits lower call device {sorted(set(it[:, 0].tolist()))} reference {sorted(set(ref.exit_iters[:, 0].tolist()))}; "
          f"upper call device {sorted(set(it[:, 1].tolist()))} reference {sorted(set(ref.exit_iters[:, 1].tolist()))}")
    assert np.isfinite(out).all()
    assert e_f <= TOL_CERT and e_o <= TOL_CERT
    never = ref.exit_iters[:, 0] == cfg.qp_max_iter - 1
    assert np.array_equal(it[never, 0], ref.exit_iters[never, 0]), (it[:, 0].tolist(), ref.exit_iters[:, 0].tolist())
    assert (np.abs(it[~never, 0] - ref.exit_iters[~never, 0]) <= 1).all(), (it[:, 0].tolist(), ref.exit_iters[:, 0].tolist())
    assert (np.abs(it[:, 1] - ref.exit_iters[:, 1]) <= 1).all(), (it[:, 1].tolist(), ref.exit_iters[:, 1].tolist())


# ---- 2. the activations are told apart; ReLU through the new entry is the old entry, bit for bit --------
def test_groupsort_and_relu_bounds_differ_on_the_same_weights():
    dev = _dev()
    T = 6
    _, _, gs = _run(dev, _counts(T), _x(T), LABEL, False, T, G.GPU_BATCHES[T], debug=True)
    _, _, relu = _run(dev, _counts(T), _x(T), LABEL, False, T, G.GPU_BATCHES[T], activation="ReLU", debug=True)
    for name in ("lb", "ub"):
        scale = float(np.abs(gs[name]).max())
        assert float(np.abs(gs[name] - relu[name]).max()) > 1000 * TOL_MLP * scale, name


def test_relu_through_the_act_entry_is_bit_identical():
    import ctypes as ct
    from fiode_amd import _lib as L, ops
    dev = _dev()
    T, batches = 8, G.GPU_BATCHES[8]
    counts = _counts(T)
    n, nb = len(counts), batches + 1
    grid = torch.from_numpy(np.ascontiguousarray(counts)).to(dev)
    x = torch.from_numpy(_x(T)).to(dev)
    w = _weights(dev)
    keep, cw = ops._weights_c(w, dev)
    lib = L.lib()
    cfg = L.CrownConfig(10, T, batches, LABEL, 0.141, 0.225, 0)
    dc = ops.DynCfg(scale_nominal=True, dropout=0.0).to_c()
    need = lib.fiode_certify_crown_workspace_bytes_act(n, batches, L.FIODE_ACT_RELU)
    assert need == lib.fiode_certify_crown_workspace_bytes(n, batches)
    res = []
    for entry in (lib.fiode_certify_crown, lib.fiode_certify_crown_act):
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        out = torch.full((nb,), float("nan"), device=dev)
        it = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
        dbg = {k: torch.full((n, c), float("nan"), device=dev) for k, c in ops.CROWN_DEBUG_FIELDS}
        dbg_c = L.CrownDebug(*[dbg[k].data_ptr() for k, _ in ops.CROWN_DEBUG_FIELDS])
        rc = entry(ops._stream(dev), ct.byref(cfg), ct.byref(dc), ct.byref(cw), x.data_ptr(), grid.data_ptr(), n,
                   out.data_ptr(), it.data_ptr(), None, ct.byref(dbg_c), ws.data_ptr(), need, L.FIODE_ACT_RELU)
        assert rc == 0
        torch.cuda.synchronize(dev)
        res.append([out.cpu().numpy(), it.cpu().numpy()] + [dbg[k].cpu().numpy() for k, _ in ops.CROWN_DEBUG_FIELDS])
    del keep
    for a, b in zip(*res):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


# ---- 3. batch independence, bit for bit --------------------------------------------------------------
def test_batch_alone_and_permuted_rows():
    dev = _dev()
    T, sn = 8, True
    batches = G.GPU_BATCHES[T]
    counts, x = _counts(T), _x(T)
    out, it = _run(dev, counts, x, LABEL, sn, T, batches)
    sl = R.device_slices(len(counts), batches)
    assert len(sl) == len(out) == 62
    for b in (0, 30, 61):
        lo, hi = sl[b]
        o1, i1 = _run(dev, np.ascontiguousarray(counts[lo:hi]), x, LABEL, sn, T, 1)
        assert o1.shape == (1,) and o1[0] == out[b] and np.array_equal(i1[0], it[b]), (b, o1, out[b], i1, it[b])
    rng = np.random.default_rng(31)
    perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in sl])
    assert not np.array_equal(perm, np.arange(len(perm)))
    out_p, it_p = _run(dev, counts[perm], x, LABEL, sn, T, batches)
    assert np.array_equal(out_p, out) and np.array_equal(it_p, it), (out_p - out, it_p.tolist(), it.tolist())


# ---- 4. device soundness -----------------------------------------------------------------------------
def test_device_bounds_enclose_the_device_mlp():
    """The device's own GroupSort MLP (the pre-projection output of the eval kernel: qp_nominal without
    scale_nominal) on sampled points of every box lies inside the device's bounds."""
    from fiode_amd import ops
    dev = _dev()
    T, npts = 6, 40
    x = _x(T)
    _, _, dbg = _run(dev, _counts(T), x, LABEL, False, T, G.GPU_BATCHES[T], debug=True)
    eta = O.db_grid_for_label(_counts(T).astype(np.int64), LABEL, T)
    pts = G.sample_box(eta, 1.0 / T, npts, np.random.default_rng(5)).astype(np.float32)
    # the points as float32 must still lie in the float32 box the kernel bounds: shrink by one rounding
    pts = np.clip(pts, eta[:, None, :] - np.float32(1.0 / T), eta[:, None, :] + np.float32(1.0 / T)).astype(np.float32)
    h = torch.from_numpy(pts.reshape(-1, 10)).to(dev)
    xf = torch.from_numpy(x).to(dev).reshape(1, 10)
    dyn = ops.DynCfg(scale_nominal=False, dropout=0.0, activation="GroupSort")
    w = _weights(dev)
    _, it = ops.dyn_eval(h, xf, w, dyn, rows_per_image=len(h))
    _, _, ev = ops.dyn_eval_backward(torch.zeros_like(h), h, xf, w, dyn, rows_per_image=len(h), exit_iter=it, debug=True)
    f = ev["qp_nominal"].cpu().numpy().astype(np.float64).reshape(len(eta), npts, 10)
    ref_f = G.net_of(_params(), x).forward(pts.reshape(-1, 10)).reshape(f.shape)
    assert np.abs(f - ref_f).max() <= 1e-4                       # it is the GroupSort MLP
    lb, ub = dbg["lb"].astype(np.float64), dbg["ub"].astype(np.float64)
    slack = TOL_MLP * max(1.0, float(np.abs(lb).max()), float(np.abs(ub).max()))
    worst = max(float((lb[:, None] - f).max()), float((f - ub[:, None]).max()))
    print(f"device soundness: worst excess {worst:.3e} (slack {slack:.3e}); mean width {float((ub - lb).mean()):.4f}")
    assert worst <= slack


# ---- 5. stop logic -----------------------------------------------------------------------------------
def test_preset_stop_flag_skips_everything():
    dev = _dev()
    T = 6
    flag = torch.ones(1, dtype=torch.int32, device=dev)
    out, it = _run(dev, _counts(T), _x(T), LABEL, True, T, G.GPU_BATCHES[T], stop_flag=flag, stop_on_violation=True)
    assert out.shape == (11,) and np.isneginf(out).all(), out
    assert (it == 0).all(), it
    assert int(flag.item()) == 1


@pytest.mark.parametrize("k", [0, 3, 11])
def test_stop_on_violation_stops_after_the_first_violating_batch(k):
    dev = _dev()
    T, sn, min_std = 6, True, 0.225
    counts, x, batches = _counts(T), _x(T), G.GPU_BATCHES[T]
    full0, _ = _run(dev, counts, x, LABEL, sn, T, batches, eps=0.0)             # kappa = 0: the bare maxima
    nb = len(full0)
    assert nb == 11
    # a kappa that puts the first k maxima below 0 and the next one above needs them to lie below it: take
    # the offset from the running maximum, and let the test say so if the case does not allow it
    before = float(full0[:k].max()) if k else -np.inf
    after = float(full0[k]) if k < nb else np.inf
    assert k in (0, nb) or after - before > 1e-2, ("the first k maxima must lie below the next one", full0.tolist())
    if k == 0:
        kappa = -after + 0.5
    elif k == nb:
        kappa = -before - 0.5
    else:
        kappa = -0.5 * (before + after)
    eps = kappa * min_std / np.sqrt(2.0)
    full, it_full = _run(dev, counts, x, LABEL, sn, T, batches, eps=eps, min_std=min_std)
    assert (full[:k] <= 0).all() and (k == nb or full[k] > 0), (k, full.tolist())
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out, it = _run(dev, counts, x, LABEL, sn, T, batches, eps=eps, min_std=min_std, stop_on_violation=True,
                   stop_flag=flag)
    assert np.array_equal(out[:k + 1], full[:k + 1]) and np.array_equal(it[:k + 1], it_full[:k + 1])
    assert np.isneginf(out[k + 1:]).all() and (it[k + 1:] == 0).all(), (k, out.tolist())
    assert int(flag.item()) == (1 if k < nb else 0)
    out_own, _ = _run(dev, counts, x, LABEL, sn, T, batches, eps=eps, min_std=min_std, stop_on_violation=True)
    assert np.array_equal(out_own, out)


# ---- 6. the driver through a GroupSort module ----------------------------------------------------------
def test_certify_crown_driver_through_groupsort_module():
    from fiode_amd import ops
    from fiode_amd.certify import certify_crown
    from tests.test_groupsort_dyn import build_module
    dev = _dev()
    T, batches = 6, 10
    mod = build_module("GroupSort").to(dev).eval()
    x = torch.rand(3, 3, 32, 32, generator=torch.Generator().manual_seed(6)).to(dev)
    with torch.no_grad():
        pred = torch.cat([mod(x[i:i + 1]).argmax(-1) for i in range(3)]).cpu()
    y = pred.clone()
    y[1] = (y[1] + 1) % 10                                    # image 1 is misclassified
    y = y.to(dev)
    dyn = mod.dyn_fun
    assert dyn.activation_name == "GroupSort"
    with pytest.raises(NotImplementedError, match="ReLU"):     # off by default
        certify_crown(mod, x, y, T=T, batches=batches)
    norm = mod.init_coordinates.param_map[0]
    min_std = float(norm.std.min()) if getattr(norm, "std", None) is not None else 1.0
    counts = _counts(T)
    with torch.no_grad():
        w = {k: v.detach().float().contiguous() for k, v in dyn.effective_weights().items()}
        dc = dyn.dyn_cfg()
        P = O.DynParams(**{k: w[k].cpu().numpy() for k in ops.WEIGHT_KEYS})
        cfg = O.DynConfig(alpha_1=dc.alpha_1, alpha_2=dc.alpha_2, sigma_1=dc.sigma_1, scale_nominal=dc.scale_nominal,
                          dropout=0.0, qp_max_iter=dc.qp_max_iter, qp_tol=dc.qp_tol)
        feats = [mod.init_coordinates(x[i:i + 1], dyn)[0].float().reshape(-1).cpu().numpy() for i in range(3)]
    for eps in (0.141, -1e3):
        with ops.groupsort_crown():
            res = certify_crown(mod, x, y, T=T, batches=batches, eps=eps)
        assert res.n_images == 3 and res.correct == 2 and res.certified_larger_T == 0
        certified = []
        for i in range(3):
            eta = O.db_grid_for_label(counts.astype(np.int64), int(y[i]), T)
            bounds = G.crown_bounds(G.net_of(P, feats[i]), eta, 1.0 / T)
            ref = R.crown_image(feats[i], int(y[i]), counts, P, cfg, T, batches, eps_cfg=eps, min_std=min_std,
                                bounds=bounds)
            viol = np.flatnonzero(ref.out > 0)
            if i == 1:
                assert np.isneginf(res.max_violations[i])
                continue
            assert (np.abs(ref.out) > 10 * TOL_CERT).all(), "a batch maximum too close to 0 to call"
            expect = float(ref.out[viol[0]]) if len(viol) else float(ref.out.max())
            print(f"driver eps={eps} image {i}: max violation {res.max_violations[i]:.6f} reference {expect:.6f}")
            if abs(expect) < 100:                               # eps = -1e3: one float32 ulp of kappa is 5e-4
                assert abs(res.max_violations[i] - expect) <= TOL_CERT
            if not len(viol):
                certified.append(i)
        assert res.certified_idx == certified and res.certified == len(certified)
        assert 1 not in res.certified_idx
    assert certified == [0, 2]
