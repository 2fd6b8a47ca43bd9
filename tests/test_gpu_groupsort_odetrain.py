"""GPU parity of the GroupSort rk4 train_ode solve (fiode_odetrain_*_act with FIODE_ACT_GROUPSORT,
behind ``ops.groupsort_train_ode()``) against the numpy oracle (``O.rk4_train`` with the GroupSort MLP
of tests/_groupsort_train_ref.py monkeypatched in) and float64 torch autograd
(tests/_groupsort_odetrain_ref.py).

Tolerances are those of tests/test_gpu_odetrain.py: forward 2e-4 absolute on the state, the stage
inputs and the saved activations; gradients 2e-4 of each tensor's max-abs against float64 autograd at
the device's linearisation points -- QP active sets, exit mu and, GroupSort's own, the pair codes
pinned to the device's (GroupSort's gradient jumps where a pair flips, so only a reference that
routes as the device did is comparable elementwise; the codes test keeps that pinning honest: every
pair the reference separates by >= 2e-5 must carry the reference's order).  The near-tie census of
the cases runs on the CPU (tests/test_groupsort_odetrain.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _groupsort_odetrain_ref as G
from tests import _groupsort_train_ref as R

pytestmark = pytest.mark.gpu
KEYS = G.KEYS
CASE_IDS = [f"B{c[0]}-h{c[1]}-sn{int(c[2])}-p{c[3]}" for c in G.CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


def _setup(i):
    from fiode_amd import _lib as L, ops
    B, step, sn, p, seed = G.CASES[i]
    dev = _dev()
    P, x, h0, labels, masks = G.make_case(B, step, p, seed)
    cfg = ops.odetrain_config(B, 0.0, 1.0, step, L.FIODE_DROPOUT_GIVEN if p > 0 else L.FIODE_DROPOUT_OFF)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in KEYS}
    dyn = ops.DynCfg(scale_nominal=sn, dropout=p, activation="GroupSort")
    mk = None if masks is None else torch.from_numpy(masks).to(dev)
    return ops, dev, P, x, h0, labels, masks, cfg, w, dyn, mk


@functools.lru_cache(maxsize=None)
def _run(i):
    """One device solve (forward, loss gradient, one-call backward) and the oracle's solve per case,
    shared by the tests below and left unchanged."""
    ops, dev, P, x, h0, labels, masks, cfg, w, dyn, mk = _setup(i)
    B, step, sn, p, seed = G.CASES[i]
    xt, h0t = torch.from_numpy(x).to(dev), torch.from_numpy(h0).to(dev)
    with ops.groupsort_train_ode():
        y, st, ws = ops.odetrain_forward(xt, h0t, w, dyn, cfg, masks=mk)
        yd = y.detach().clone().requires_grad_(True)
        torch.nn.functional.nll_loss(torch.log(yd), torch.from_numpy(labels).to(dev)).backward()
        sv = {k: v.cpu().clone() for k, v in ops.odetrain_saved(ws, cfg).items()}
        codes = {k: v.cpu().clone() for k, v in ops.odetrain_pair_codes(ws, cfg).items()}
        grads, _ = ops.odetrain_backward(yd.grad, xt, w, dyn, cfg, ws)
        grads = {k: v.cpu().clone() for k, v in grads.items()}
    torch.cuda.synchronize()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(O, "mlp_forward", R.mlp_forward)
        ref, recs = O.rk4_train(x, h0, P, O.DynConfig(scale_nominal=sn), 0.0, 1.0, step, masks, p)
    return dict(y=y.cpu(), stats=st.cpu().numpy(), sv=sv, codes=codes, grads=grads, ref=ref, recs=recs,
                E=ops.odetrain_evals(cfg))


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=CASE_IDS)
def test_forward_matches_oracle(i):
    r = _run(i)
    E, s, sv, recs = r["E"], r["stats"], r["sv"], r["recs"]
    assert len(recs) == E == G.n_evals(G.CASES[i][1])
    assert s[0] == E and s[1] == E // 4 and s[3] == 0
    err = float(np.abs(r["y"].numpy() - r["ref"]).max())
    herr = max(float(np.abs(sv["h"][:, e].numpy() - recs[e][0]).max()) for e in range(E))
    a1 = max(float(np.abs(sv["a1"][:, e].numpy() - recs[e][1].mlp["a1"]).max()) for e in range(E))
    a2 = max(float(np.abs(sv["a2"][:, e].numpy() - recs[e][1].mlp["a2"]).max()) for e in range(E))
    print(f"{CASE_IDS[i]}: y {err:.3e} stage inputs {herr:.3e} a1 {a1:.3e} a2 {a2:.3e}")
    assert err <= 2e-4, err
    assert herr <= 2e-4, herr
    assert a1 <= 2e-4 and a2 <= 2e-4, (a1, a2)


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=CASE_IDS)
def test_pair_codes_follow_the_reference_order(i):
    r = _run(i)
    B, step, sn, p, seed = G.CASES[i]
    masks = G.make_case(B, step, p, seed)[4]
    order, tie = r["codes"]["order"].numpy(), r["codes"]["tie"].numpy()
    assert order.shape == tie.shape == (B, r["E"], 2, 64)
    assert not (order & tie).any()
    checked = flipped = 0
    for e, (_, res) in enumerate(r["recs"]):
        for l, key in enumerate(("d1", "d2")):
            d = res.mlp[key].astype(np.float64)
            a, b = d[:, :64], d[:, 64:]
            sep = np.abs(a - b) >= R.MIN_SEPARATION
            checked += int(sep.sum())
            flipped += int((order[:, e, l][sep] != (a > b)[sep]).sum()) + int(tie[:, e, l][sep].sum())
            if masks is not None:
                dropped = (masks[e, l][:, :64] == 0) & (masks[e, l][:, 64:] == 0)
                assert dropped.any() and tie[:, e, l][dropped].all(), (e, l)
    print(f"{CASE_IDS[i]}: {checked} separated pairs, {flipped} with another order on the device")
    assert checked > 0 and flipped == 0


@pytest.mark.parametrize("i", range(len(G.CASES)), ids=CASE_IDS)
def test_backward_matches_pinned_autograd(i, monkeypatch):
    r = _run(i)
    B, step, sn, p, seed = G.CASES[i]
    P, x, h0, labels, masks = G.make_case(B, step, p, seed)
    sv, E = r["sv"], r["E"]
    act = ((sv["v"] - sv["nominal"]) + sv["mu"][..., None] > 0)            # [B,E,C]
    acts = [act[:, e] for e in range(E)]
    mus = [sv["mu"][:, e].double() for e in range(E)]
    _, yy, ref, _ = G.solve_with_grads(monkeypatch, P, x, h0, labels, masks, step, sn, p, acts=acts, mus=mus,
                                       order=r["codes"]["order"], tie=r["codes"]["tie"])
    assert float((yy - r["y"].double()).abs().max()) <= 2e-4
    worst = {}
    for k in KEYS + ("x_feat",):
        g = r["grads"][k].double()
        scale = float(ref[k].abs().max()) + 1e-12
        worst[k] = float((g - ref[k]).abs().max()) / scale
    print(f"{CASE_IDS[i]}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, err in worst.items():
        assert err <= 2e-4, (k, err)


def test_dropout_off_equals_the_inference_solve():
    """Train mode with dropout off = the rk4 inference solve fiode_odeint_act(GROUPSORT) on the same
    inputs (same tile code, keep words all ones and scale 1)."""
    i = 4
    ops, dev, P, x, h0, labels, masks, cfg, w, dyn, mk = _setup(i)
    assert masks is None
    xt, h0t = torch.from_numpy(x).to(dev), torch.from_numpy(h0).to(dev)
    ts = torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev)
    sol, st, _ = ops.odeint_dyn(xt, h0t, ts, w, dyn, method="rk4", step_size=G.CASES[i][1])
    y = _run(i)["y"]
    assert int(st[3]) == 0
    err = float((sol[1].cpu() - y).abs().max())
    print(f"dropout off: |train - inference| = {err:.3e}, bit-identical: {torch.equal(sol[1].cpu(), y)}")
    assert err <= 2e-4


def test_split_backward_entry_points_and_repeated_sweep():
    """backward_x + backward_weights = the one-call backward (weight gradients bit for bit, dL/dx_feat
    the same sum in another order), and a second sweep on the same forward workspace reproduces the
    first bit for bit (the sweep reads the codes and keep words, it writes neither)."""
    i = 2
    ops, dev, P, x, h0, labels, masks, cfg, w, dyn, mk = _setup(i)
    B = G.CASES[i][0]
    xt, h0t = torch.from_numpy(x).to(dev), torch.from_numpy(h0).to(dev)
    gy = torch.randn(B, 10, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)
    with ops.groupsort_train_ode():
        y, st, ws = ops.odetrain_forward(xt, h0t, w, dyn, cfg, masks=mk)
        one, _ = ops.odetrain_backward(gy, xt, w, dyn, cfg, ws)
        one = {k: v.clone() for k, v in one.items()}
        gx = ops.odetrain_backward_x(gy, xt, w, dyn, cfg, ws)
        wg = ops.odetrain_backward_weights(xt, w, dyn, cfg, ws)
        gx2 = ops.odetrain_backward_x(gy, xt, w, dyn, cfg, ws)
        two, _ = ops.odetrain_backward(gy, xt, w, dyn, cfg, ws)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(wg[k], one[k]), k
        assert torch.equal(two[k], one[k]), k
    assert torch.equal(gx2, gx) and torch.equal(two["x_feat"], one["x_feat"])
    torch.testing.assert_close(gx, one["x_feat"], rtol=1e-5, atol=1e-6 * float(one["x_feat"].abs().max()))


def test_philox_masks_fresh_per_offset():
    from fiode_amd import _lib as L
    ops, dev, P, x, h0, labels, masks, cfg, w, dyn, mk = _setup(2)
    B, step = G.CASES[2][0], G.CASES[2][1]
    xt, h0t = torch.from_numpy(x).to(dev), torch.from_numpy(h0).to(dev)
    outs, kws = [], []
    with ops.groupsort_train_ode():
        for off in (0, 0, 1):
            c = ops.odetrain_config(B, 0.0, 1.0, step, L.FIODE_DROPOUT_PHILOX, seed=9, offset=off)
            y, _, ws = ops.odetrain_forward(xt, h0t, w, dyn, c)
            outs.append(y.cpu())
            kws.append(ops.odetrain_saved(ws, c)["keep_words"].cpu().clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(kws[0], kws[1])
    assert not torch.equal(kws[0], kws[2]) and not torch.equal(outs[0], outs[2])
    assert torch.isfinite(outs[2]).all()
    assert torch.allclose(outs[2].sum(-1), torch.ones(B), atol=1e-3)


def _train_ode_module(dev, seed=0):
    from tests.test_groupsort_dyn import build_module
    mod = build_module("GroupSort", seed=seed).to(dev).train()
    mod.train_ode, mod.train_ode_solver, mod.train_ode_tol = True, "rk4", 0.25
    assert mod.ode_branch_active()
    return mod


def test_groupsort_module_trains_through_the_rk4_branch_eager_and_captured():
    """LyapunovLearning with GroupSort dynamics and the rk4 train_ode branch active: compute_loss +
    backward reach every parameter; the captured step replays the eager step (the comparison of
    test_groupsort_module_trains_eager_and_captured); with the switch off, or with dopri5, both
    refuse as before."""
    from fiode_amd import ops
    from fiode_amd.graph_step import GraphTrainStep
    dev = _dev()
    B = 8
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.rand(B, 3, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    mod = _train_ode_module(dev)
    for ctx in (ops.groupsort_train_ode(False), ops.groupsort_training()):
        with ctx:
            with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
                mod.compute_loss(x, y)
            with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
                GraphTrainStep(mod, mod.configure_optimizers(capturable=True)[0][0], x, y, warmup=1)
    with ops.groupsort_train_ode():
        mod.train_ode_solver = "dopri5"
        with pytest.raises(NotImplementedError, match="evaluation, ODE solves and certification"):
            mod.compute_loss(x, y)
        mod.train_ode_solver = "rk4"
        mod.compute_loss(x, y).backward()
        torch.cuda.synchronize()
        s = mod.last_ode_plan["stats"].cpu()
        assert int(s[0]) == 16 and int(s[1]) == 4 and int(s[3]) == 0
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
        twin = _train_ode_module(dev, seed=1)
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


@pytest.mark.parametrize("reuse", [True, False])
def test_fused_loss_node_equals_three_nodes(reuse):
    """LyapODELossFn = LyapunovLossFn + ODETrainFn + ODELossMixFn with GroupSort dynamics: the same
    loss and gradients bit for bit (tests/test_gpu_odetrain.py's comparison), features reused or the
    backbone re-run for the solve."""
    from fiode_amd import ops, lyapunov as LY
    dev = _dev()
    x = torch.rand(8, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    yb = torch.randint(0, 10, (8,), device=dev, generator=torch.Generator(device=dev).manual_seed(6))
    out = {}
    LY.DYN_WGRAD_SIDE = False
    try:
        with ops.groupsort_train_ode():
            for variant in ("fused", "three"):
                mod = _train_ode_module(dev)
                mod.parallel_cayley = False
                mod.ode_reuse_features = reuse
                mod.fused_ode_loss = variant != "three"
                mod._rng_offset = 0
                loss = mod.compute_loss(x, yb, 8, "relu")
                loss.backward()
                torch.cuda.synchronize()
                out[variant] = (loss.detach().clone(),
                                {n: p.grad.detach().clone() for n, p in mod.named_parameters() if p.requires_grad})
    finally:
        LY.DYN_WGRAD_SIDE = True
    assert torch.equal(out["fused"][0], out["three"][0])
    for n in out["fused"][1]:
        assert torch.equal(out["fused"][1][n], out["three"][1][n]), n
