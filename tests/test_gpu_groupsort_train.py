"""GPU tests of GroupSort TRAINING through the fused Lyapunov step (fiode_lyap_step_act with
FIODE_ACT_GROUPSORT; k_lyap_fwd<GROUPSORT> / k_lyap_bwd<GROUPSORT>), all inside
``ops.groupsort_training()``.

Reference: tests/_groupsort_train_ref.py installed into the oracle.  Tolerances are those of
test_gpu_lyap.py::test_lyap_step_matches_oracle; the parity inputs hold no pair of pre-sort values
closer than 2e-5 (test_groupsort_train.py), so device and reference order every pair alike.
"""
import ctypes as ct

import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _groupsort_train_ref as R
from tests._util import make_params, make_step_inputs

pytestmark = pytest.mark.gpu
GRAD_KEYS = ("Q3", "b3", "Q2", "b2", "Q1", "b1", "Qx", "bx", "x_feat")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


def _wt(P, dev):
    from fiode_amd import ops
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}


def _dyn(scale_nominal, activation="GroupSort"):
    from fiode_amd import ops
    c = O.DynConfig()
    return ops.DynCfg(alpha_1=c.alpha_1, alpha_2=c.alpha_2, sigma_1=c.sigma_1, scale_nominal=scale_nominal,
                      dropout=c.dropout, activation=activation)


def _run_given(B, S, seed, scale_nominal, dropout=True, activation="GroupSort"):
    from fiode_amd import ops, _lib as L
    dev = _dev()
    P = make_params(seed=seed)
    inp = make_step_inputs(B=B, S=S, seed=seed + 1, dropout=dropout)
    masks, mode = None, L.FIODE_DROPOUT_OFF
    if dropout:
        masks = torch.from_numpy(np.stack([inp.mask1, inp.mask2, inp.lmask1, inp.lmask2])).to(dev)
        mode = L.FIODE_DROPOUT_GIVEN
    with ops.groupsort_training():
        sc, gr, dbg = ops.lyap_step(torch.from_numpy(inp.x_feat).to(dev), torch.from_numpy(inp.y).to(dev),
                                    _wt(P, dev), _dyn(scale_nominal, activation), sample_size=S, n_uniform=S,
                                    sampler=L.FIODE_SAMPLER_GIVEN, dropout_mode=mode, kappa=inp.kappa,
                                    h=torch.from_numpy(inp.h).to(dev), masks=masks, debug=True)
    torch.cuda.synchronize()
    return P, inp, sc, gr, dbg


@pytest.mark.parametrize("B,S,seed,scale_nominal", R.PARITY_CASES)
def test_groupsort_step_matches_reference(B, S, seed, scale_nominal, monkeypatch):
    """One tile (4, 8); a partial last tile with images straddling tiles (3, 37); 32 tiles over 8
    rounds (16, 64).  Dropout masks and samples given."""
    P, inp, sc, gr, dbg = _run_given(B, S, seed, scale_nominal)
    sc = sc.cpu().numpy()
    g = {k: v.cpu().numpy() for k, v in gr.items()}
    d = {k: v.cpu().numpy() for k, v in dbg.items()}
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    relu = O.lyapunov_step(inp, P, cfg)
    monkeypatch.setattr(O, "mlp_forward", R.mlp_forward)
    monkeypatch.setattr(O, "mlp_backward", R.mlp_backward)
    u_rows = np.repeat(O.static_projection(inp.x_feat, P), S, 0)
    # 1) MLP + barrier of both passes against the reference's own forward
    for p, (m1, m2) in enumerate(((inp.mask1, inp.mask2), (inp.lmask1, inp.lmask2))):
        ref = O.eval_dot(inp.h, u_rows, P, cfg, m1, m2)
        scale = max(1.0, float(np.abs(ref.nominal).max()))
        err = float(np.abs(d["qp_nominal"][p] - ref.nominal).max())
        print(f"pass {p}: qp_nominal err {err:.3e} (scale {scale:.3g})")
        assert err <= 2e-5 * scale, (p, err)
    err = float(np.abs(d["qp_lower"] - ref.lower).max())
    assert err <= 2.5e-7 * cfg.alpha_1, err
    # 2) the QP on the device's own inputs: bit-exact, the same global exit iteration
    q = O.qp_forward(d["qp_lower"], d["qp_nominal"][0], cfg.qp_max_iter, cfg.qp_tol)
    assert int(sc[3]) == q.iters
    assert np.array_equal(d["f"], q.v), float(np.abs(d["f"] - q.v).max())
    ql = O.qp_forward(d["qp_lower"], d["qp_nominal"][1], cfg.qp_max_iter, cfg.qp_tol)
    assert int(sc[4]) == ql.iters
    assert np.array_equal(d["f_log"], ql.v), float(np.abs(d["f_log"] - ql.v).max())
    # 3) the whole step with the QP inputs pinned to the device's
    inp.qp_inputs = (d["qp_lower"], d["qp_nominal"][0])
    inp.qp_inputs_log = (d["qp_lower"], d["qp_nominal"][1])
    out = O.lyapunov_step(inp, P, cfg)
    assert np.array_equal(d["V"], out.V)
    assert np.array_equal(d["Vdot"], out.Vdot)
    assert abs(sc[0] - out.loss) <= 1e-5 * max(1.0, abs(out.loss))
    assert int(sc[1]) == out.eff == B * S
    assert abs(sc[2] - out.mean_active) <= 1e-7
    for k in GRAD_KEYS:
        a, b = g[k], out.grads[k]
        err, mx = float(np.abs(a - b).max()), float(np.abs(b).max())
        print(f"{k}: err {err:.3e} of max {mx:.3e} ({err / max(mx, 1e-30):.2e})")
        assert err <= 2e-4 * max(1e-6, mx), (k, err, mx)
    # a kernel still applying ReLU is far outside every tolerance above
    assert abs(sc[0] - relu.loss) > 1e-3


@pytest.mark.parametrize("scale_nominal", [True, False])
def test_dropout_off_step_equals_the_eval_kernels(scale_nominal):
    """Dropout off, device against device, at a size where a float64 reference would meet near ties:
    the step's f is dyn_eval's, and its nine gradients are dyn_eval_backward's of the loss gradient
    rebuilt from the step's own V and V-dot."""
    from fiode_amd import ops
    B, S = 32, 64
    N = B * S
    P, inp, sc, gr, dbg = _run_given(B, S, 3264, scale_nominal, dropout=False)
    dev = sc.device
    w, dyn = _wt(P, dev), _dyn(scale_nominal)
    h, x = torch.from_numpy(inp.h).to(dev), torch.from_numpy(inp.x_feat).to(dev)
    f, it = ops.dyn_eval(h, x, w, dyn, rows_per_image=S)
    assert int(it.item()) == int(sc[3].item())
    scale = max(1.0, float(f.abs().max()))
    err = float((dbg["f"] - f).abs().max())
    print(f"f vs dyn_eval: err {err:.3e}, bit-equal {torch.equal(dbg['f'], f)}")
    assert err <= 2e-5 * scale
    V, Vd = dbg["V"].cpu().numpy(), dbg["Vdot"].cpu().numpy()
    pre = (Vd + (np.float32(inp.kappa) * V).astype(np.float32)).astype(np.float32)
    y_rows = np.repeat(inp.y.astype(np.int64), S)
    gp = np.where(pre > 0, np.float32(1.0) / np.float32(N), np.float32(0)).astype(np.float32)
    g_f = np.zeros((N, 10), np.float32)
    np.put_along_axis(g_f, O.runner_up(inp.h, y_rows)[:, None], gp[:, None], 1)
    np.put_along_axis(g_f, y_rows[:, None], -gp[:, None], 1)
    assert int((pre > 0).sum()) == int(sc[1].item()) > 0
    _, ref = ops.dyn_eval_backward(torch.from_numpy(g_f).to(dev), h, x, w, dyn, rows_per_image=S,
                                   exit_iter=int(sc[3].item()))
    torch.cuda.synchronize()
    for k in GRAD_KEYS:
        a, b = gr[k], ref[k]
        err, mx = float((a - b).abs().max()), float(b.abs().max())
        print(f"{k}: err {err:.3e} of max {mx:.3e}")
        assert mx > 0 and err <= 2e-4 * mx, (k, err, mx)


def _assert_steps_equal(a, b, debug_keys=()):
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for k in debug_keys:
        assert torch.equal(a[2][k], b[2][k]), k


def test_philox_step_equals_given_rerun():
    """The in-kernel sampler and Philox dropout against a rerun fed the variates and keep words it
    reports: every scalar and gradient bit-equal (B = 4, S = 40: five tiles, images straddling them)."""
    from fiode_amd import ops, _lib as L
    from tests.test_gpu_sampler import masks_from_keep_words
    dev = _dev()
    B, S, S1 = 4, 40, 32
    P = make_params(seed=440)
    rng = np.random.default_rng(441)
    x = torch.from_numpy(rng.normal(size=(B, 10)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 10, B)).to(dev)
    w, dyn = _wt(P, dev), _dyn(True)
    with ops.groupsort_training():
        a = ops.lyap_step(x, y, w, dyn, sample_size=S, n_uniform=S1, sampler=L.FIODE_SAMPLER_COMPOSITE,
                          dropout_mode=L.FIODE_DROPOUT_PHILOX, seed=17, offset=5, debug=True)
        a = (a[0].clone(), {k: v.clone() for k, v in a[1].items()}, {k: v.clone() for k, v in a[2].items()})
        masks = masks_from_keep_words(a[2]["keep_words"])
        b = ops.lyap_step(x, y, w, dyn, sample_size=S, n_uniform=S1, sampler=L.FIODE_SAMPLER_COMPOSITE,
                          dropout_mode=L.FIODE_DROPOUT_GIVEN, masks=masks, exp_draws=a[2]["exp_draws"], debug=True)
        torch.cuda.synchronize()
        _assert_steps_equal(a, b, ("h", "keep_words", "V", "Vdot", "f", "f_log", "g_ftilde"))
        c = ops.lyap_step(x, y, w, dyn, sample_size=S, n_uniform=S1, sampler=L.FIODE_SAMPLER_GIVEN, h=a[2]["h"],
                          dropout_mode=L.FIODE_DROPOUT_GIVEN, masks=masks, debug=True)
        torch.cuda.synchronize()
        _assert_steps_equal(a, c, ("V", "Vdot", "f", "f_log", "g_ftilde"))
    m = masks.float().mean().item()
    assert 0.4 < m < 0.6 and torch.isfinite(a[0]).all()
    assert all(torch.isfinite(v).all() and v.abs().max() > 0 for v in a[1].values())


def test_groupsort_step_is_bit_reproducible():
    B, S, seed, sn = R.PARITY_CASES[-1]
    runs = []
    for _ in range(2):
        _, _, sc, gr, dbg = _run_given(B, S, seed, sn)
        runs.append((sc.clone(), {k: v.clone() for k, v in gr.items()}, {k: v.clone() for k, v in dbg.items()}))
    _assert_steps_equal(runs[0], runs[1], tuple(runs[0][2]))


def test_relu_through_act_entry_point_equals_lyap_step():
    """ops.lyap_step (fiode_lyap_step_act, FIODE_ACT_RELU) against a direct call of fiode_lyap_step."""
    from fiode_amd import ops, _lib as L
    B, S = 3, 37
    N = B * S
    P, inp, sc, gr, dbg = _run_given(B, S, 337, True, activation="ReLU")
    dev = sc.device
    w = _wt(P, dev)
    masks = torch.from_numpy(np.stack([inp.mask1, inp.mask2, inp.lmask1, inp.lmask2])).to(dev)
    x, y, h = (torch.from_numpy(t).to(dev) for t in (inp.x_feat, inp.y, inp.h))
    sc2 = torch.empty(8, device=dev)
    gr2 = {k: torch.empty_like(v) for k, v in gr.items()}
    dbg2 = {k: torch.empty_like(v) for k, v in dbg.items()}
    cfg = L.LyapConfig(B, S, S, L.FIODE_SAMPLER_GIVEN, L.FIODE_DROPOUT_GIVEN, float(inp.kappa), 0, 0)
    dc = _dyn(True, "ReLU").to_c()
    cw = L.DynWeights(*[w[k].data_ptr() for k in ops.WEIGHT_KEYS])
    io = L.LyapIO(x.data_ptr(), y.data_ptr(), h.data_ptr(), masks.data_ptr(), sc2.data_ptr(),
                  *[dbg2[k].data_ptr() for k in ("h", "V", "Vdot", "f", "f_log", "qp_lower", "qp_nominal",
                                                 "g_ftilde")],
                  None, 0, None, None, None, dbg2["keep_words"].data_ptr(), None)
    cg = L.LyapGrads(*[gr2[k].data_ptr() for k in ops.WEIGHT_KEYS + ("x_feat",)])
    lib = L.lib()
    ws = torch.empty(lib.fiode_lyap_workspace_bytes(ct.byref(cfg), ct.byref(dc)), dtype=torch.uint8, device=dev)
    rc = lib.fiode_lyap_step(ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream), ct.byref(cfg), ct.byref(dc),
                             ct.byref(cw), ct.byref(io), ct.byref(cg), ct.c_void_p(ws.data_ptr()),
                             ct.c_size_t(ws.numel()))
    assert rc == 0
    torch.cuda.synchronize()
    assert set(dbg) == set(dbg2) and N == dbg["V"].numel()
    _assert_steps_equal((sc, gr, dbg), (sc2, gr2, dbg2), tuple(dbg))


def test_groupsort_module_trains_eager_and_captured():
    """LyapunovLearning with GroupSort dynamics (train_ode False): compute_loss + backward reach every
    parameter; the captured step replays the eager step; with the switch off both refuse as before."""
    from fiode_amd import ops
    from fiode_amd.graph_step import GraphTrainStep
    from tests.test_groupsort_dyn import build_module
    dev = _dev()
    B = 8
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.rand(B, 3, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    mod = build_module("GroupSort", seed=0).to(dev).train()
    with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
        mod.compute_loss(x, y)
    with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
        GraphTrainStep(mod, mod.configure_optimizers(capturable=True)[0][0], x, y, warmup=1)
    with ops.groupsort_training():
        mod.compute_loss(x, y).backward()
        torch.cuda.synchronize()
        for n, p in mod.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and torch.isfinite(p.grad).all(), n
        dyn_grads = [p.grad for p in mod.dyn_fun.parameters() if p.requires_grad]
        assert dyn_grads and all(float(t.abs().max()) > 0 for t in dyn_grads)
        for p in mod.parameters():
            p.grad = None
        # the captured step against the eager step (the comparison of tests/test_gpu_graph.py)
        mod.rng_counter = None
        opt = mod.configure_optimizers(capturable=True)[0][0]
        gs = GraphTrainStep(mod, opt, x, y, warmup=2)
        twin = build_module("GroupSort", seed=1).to(dev).train()
        twin.load_state_dict(mod.state_dict())
        twin.rng_counter = mod.rng_counter.clone()
        twin.seed = mod.seed
        c0 = int(mod.rng_counter)
        loss = gs.step()
        torch.cuda.synchronize()
        assert int(mod.rng_counter) == c0 + 1
        graph_grads = [p.grad.clone() for p in mod.parameters() if p.requires_grad]
        l2 = twin.compute_loss(x, y, B, "relu")
        l2.backward()
        eager_grads = [p.grad for p in twin.parameters() if p.requires_grad]
        torch.testing.assert_close(loss, l2, rtol=1e-5, atol=1e-6)
        for a, b in zip(graph_grads, eager_grads):
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
        before = float(loss.detach())
        assert float(gs.step()) != before           # a second replay, fresh samples
        gs.close()
