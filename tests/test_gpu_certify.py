"""GPU parity of the certification path (fiode_certify_grid / fiode_certify) against the oracle
(grid construction order, per-batch max violations with the per-batch QP exit).

Tolerance on the per-batch maxima: 2e-3 absolute (the max over rows of a QP output; a row whose
batch exit iteration differs by one bisection step between the MFMA and the float64 oracle MLP
moves f by at most the bracket / 2^K)."""
import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests._util import make_params

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


@pytest.mark.parametrize("T", [4, 8, 12, 2, 3, 5, 7, 9, 11, 16, 20, 1])
def test_grid_matches_construction_order(T):
    """Even and odd T (odd T ends in db_unrank's k == 2 blocks with no rows), up to the 367,123
    rows of T = 20; T = 1 has no rows at all and the slice is empty."""
    from fiode_amd import ops
    dev = _dev()
    g = ops.certify_grid(T, device=dev).cpu().numpy()
    ref = O.db_grid_rows(10, T)
    assert g.shape == ref.shape
    assert np.array_equal(g.astype(np.int64), ref)
    if T == 1:
        assert g.shape == (0, 10)


def test_grid_T40_count_and_rows():
    from fiode_amd import ops
    dev = _dev()
    g = ops.certify_grid(40, device=dev)
    assert tuple(g.shape) == (41_320_837, 10)
    f = O.db_count_table(10, 40)
    rng = np.random.default_rng(0)
    rows = np.concatenate([[0, 1, 41_320_836], rng.integers(0, 41_320_837, 200)])
    gs = g[torch.from_numpy(rows).to(dev)].cpu().numpy()
    for r, v in zip(rows, gs):
        assert O.db_unrank(int(r), 10, 40, f) == v.tolist()
    s = g.to(torch.int32).sum(1)
    assert int(s.min()) == 40 and int(s.max()) == 40
    assert bool((g[:, 0].to(torch.int32) == g[:, 1:].to(torch.int32).max(1).values).all())


@pytest.mark.parametrize("T,label,scale_nominal", [(8, 0, False), (12, 3, False), (12, 7, True)])
def test_certify_image_matches_oracle(T, label, scale_nominal):
    from fiode_amd import ops
    dev = _dev()
    P = make_params(seed=40 + T)
    x = np.random.default_rng(T).normal(size=10).astype(np.float32)
    grid_v = O.db_grid_rows(10, T)
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    cc = O.CertifyConst(T=T, batches=10)
    vmax, vtmax = O.certify_image(x, label, grid_v, P, cfg, cc)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}
    grid = ops.certify_grid(T, device=dev)
    out, it = ops.certify_image(torch.from_numpy(x).to(dev), label, grid, w,
                                ops.DynCfg(scale_nominal=scale_nominal, dropout=0.0), T=T, batches=10)
    o = out.cpu().numpy()
    assert o.shape == (len(vmax), 2)
    err = float(np.abs(o[:, 0] - vmax).max()), float(np.abs(o[:, 1] - vtmax).max())
    assert max(err) <= 2e-3, err


def test_certify_driver_through_module():
    """certify_lipschitz over a few synthetic images with the bench module (T=12 grid)."""
    import bench
    from fiode_amd.certify import certify_lipschitz
    dev = _dev()
    mod = bench.build_module(dev)
    x = torch.rand(3, 3, 32, 32, device=dev)
    y = torch.tensor([1, 4, 9], device=dev)
    res = certify_lipschitz(mod, x, y, T=12, batches=10)
    assert res.n_images == 3 and len(res.max_violations) == 3
    assert all(np.isfinite(res.max_violations))
    # the accuracy count from the features computed once = the reference's module(image) call
    with torch.no_grad():
        ref = sum(int(int(mod(x[i:i + 1]).argmax(-1)) == int(y[i])) for i in range(3))
    assert res.correct == ref
    _check_driver(mod, x, y, res, T=12, batches=10)
    # 71 batches: more than one 64-thread block of k_cert_decode
    _check_driver(mod, x, y, certify_lipschitz(mod, x, y, T=12, batches=70), T=12, batches=70)


def _check_driver(mod, x, y, res, T, batches):
    """The driver's figures against the per-row reference (tests/_cert_ref.py) evaluated on the
    device's own static_state and effective weights, and its counts against the device's `out`."""
    from fiode_amd import ops
    from tests import _cert_ref as CR
    dyn = mod.dyn_fun
    dev = x.device
    norm = mod.init_coordinates.param_map[0]
    min_std = float(norm.std.min()) if getattr(norm, "std", None) is not None else 1.0
    counts = O.db_grid_rows(10, T).astype(np.uint8)
    grid = ops.certify_grid(T, device=dev)
    certified = certified_T = 0
    with torch.no_grad():
        w = {k: v.detach().float().contiguous() for k, v in dyn.effective_weights().items()}
        dc = dyn.dyn_cfg()
        dc.dropout = 0.0
        P = O.DynParams(**{k: w[k].cpu().numpy() for k in ops.WEIGHT_KEYS})
        cfg = O.DynConfig(alpha_1=dc.alpha_1, alpha_2=dc.alpha_2, sigma_1=dc.sigma_1, scale_nominal=dc.scale_nominal,
                          dropout=0.0, qp_max_iter=dc.qp_max_iter, qp_tol=dc.qp_tol)
        assert len(res.max_violations) == x.shape[0]
        for i in range(x.shape[0]):
            static_state, _ = mod.init_coordinates(x[i:i + 1], dyn)
            xf = static_state.float().reshape(-1)
            out, _ = ops.certify_image(xf, int(y[i]), grid, w, dc, T=T, batches=batches, min_std=min_std)
            o = out.cpu().numpy()
            ref = CR.cert_rows(counts, int(y[i]), xf.cpu().numpy(), P, cfg, T, batches,
                               activation=dc.activation.lower(), min_std=min_std)
            assert o.shape == ref.out.shape and np.isfinite(o).all()
            err = abs(res.max_violations[i] - float(ref.vmax.max()))
            print(f"driver batches={batches} image {i}: max violation {res.max_violations[i]:.6f} "
                  f"reference {float(ref.vmax.max()):.6f} err {err:.3e}")
            assert err <= 2e-3, (i, res.max_violations[i], float(ref.vmax.max()))
            assert float(np.abs(o - ref.out).max()) <= 2e-3
            certified += int(float(o[:, 0].max()) < 0)
            certified_T += int(float(o[:, 1].max()) < 0)
    assert res.certified == certified == len(res.certified_idx) and res.certified_larger_T == certified_T
