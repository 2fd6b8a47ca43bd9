"""GPU tests of the fused Lyapunov step with a loss config (fiode_lyap_step_loss; k_lyap_bwd<A, true>):
every Lyapunov candidate, the ELU / identity hinges and the margin cap, for ReLU and GroupSort dynamics,
against tests/_lyap_loss_ref.py with the QP inputs pinned to the device's (as test_gpu_lyap.py).

Bounds: f and the QP exit iterations bit-equal; V / Vdot bit-equal to the float32 reference for
DecisionBoundary and OnemEtay (sums of exact products), else within 1e-6 * max(1, max|array|) of the
float64 closed form (the float32-per-op form is within 1.6e-7 on these inputs: about 6x left for the
device's logf / expf / division); the sign of pre and eff equal (no row of the inputs is near pre = 0 or
near the cap: test_lyap_loss_ref.py, asserted again here on the pinned reference); loss within
1e-5 * max(1, |loss|); the nine gradients and g_ftilde within 2e-4 of their max
(test_lyap_step_matches_oracle's bounds).
"""
import ctypes as ct

import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _groupsort_train_ref as G
from tests import _lyap_loss_ref as R
from tests._util import make_params, make_step_inputs

pytestmark = pytest.mark.gpu
GRAD_KEYS = ("Q3", "b3", "Q2", "b2", "Q1", "b1", "Qx", "bx", "x_feat")
BIT_EQUAL = ("DecisionBoundary", "OnemEtay")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda:0")


def _wt(P, dev):
    from fiode_amd import ops
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}


def _dyn(scale_nominal, activation="ReLU"):
    from fiode_amd import ops
    c = O.DynConfig()
    return ops.DynCfg(alpha_1=c.alpha_1, alpha_2=c.alpha_2, sigma_1=c.sigma_1, scale_nominal=scale_nominal,
                      dropout=c.dropout, activation=activation)


def _cfg(loss: R.Loss):
    from fiode_amd import ops
    return ops.LossCfg(loss.candidate, loss.hinge, loss.cap)


def _run(P, inp, scale_nominal, loss, activation="ReLU"):
    """One GIVEN step (samples and, when the inputs carry them, dropout masks given), debug outputs on."""
    from fiode_amd import ops, _lib as L
    dev = _dev()
    masks, mode = None, L.FIODE_DROPOUT_OFF
    if inp.mask1 is not None:
        masks = torch.from_numpy(np.stack([inp.mask1, inp.mask2, inp.lmask1, inp.lmask2])).to(dev)
        mode = L.FIODE_DROPOUT_GIVEN
    with ops.groupsort_training(activation == "GroupSort"):
        sc, gr, dbg = ops.lyap_step(torch.from_numpy(inp.x_feat).to(dev), torch.from_numpy(inp.y).to(dev),
                                    _wt(P, dev), _dyn(scale_nominal, activation), sample_size=inp.S, n_uniform=inp.S,
                                    sampler=L.FIODE_SAMPLER_GIVEN, dropout_mode=mode, kappa=inp.kappa,
                                    h=torch.from_numpy(inp.h).to(dev), masks=masks, debug=True,
                                    loss=None if loss is None else _cfg(loss))
    torch.cuda.synchronize()
    return sc, gr, dbg


_DEFAULT = {}


def _default_loss(key, P, inp, sn, activation="ReLU"):
    """The default config's loss on the same inputs, once per case (the wrong-candidate yardstick)."""
    if key not in _DEFAULT:
        _DEFAULT[key] = float(_run(P, inp, sn, None, activation)[0][0])
    return _DEFAULT[key]


def _check_against_reference(P, inp, cfg, loss, sc, gr, dbg, tag):
    sc = sc.cpu().numpy()
    g = {k: v.cpu().numpy() for k, v in gr.items()}
    d = {k: v.cpu().numpy() for k, v in dbg.items()}
    # the QP on the device's own inputs: bit-exact, the same global exit iterations
    q = O.qp_forward(d["qp_lower"], d["qp_nominal"][0], cfg.qp_max_iter, cfg.qp_tol)
    ql = O.qp_forward(d["qp_lower"], d["qp_nominal"][1], cfg.qp_max_iter, cfg.qp_tol)
    assert int(sc[3]) == q.iters and int(sc[4]) == ql.iters
    assert np.array_equal(d["f"], q.v) and np.array_equal(d["f_log"], ql.v)
    # the whole step with the QP inputs pinned to the device's
    inp.qp_inputs = (d["qp_lower"], d["qp_nominal"][0])
    inp.qp_inputs_log = (d["qp_lower"], d["qp_nominal"][1])
    out = R.lyapunov_step(inp, P, cfg, loss)
    print(tag, R.check_input_conditions(out, loss))
    for k, r32, r64 in (("V", out.V, out.V64), ("Vdot", out.Vdot, out.Vdot64)):
        if loss.candidate in BIT_EQUAL:
            assert np.array_equal(d[k], r32), (k, float(np.abs(d[k] - r32).max()))
        else:
            err, mx = float(np.abs(d[k] - r64).max()), float(np.abs(r64).max())
            print(f"{tag} {k}: err {err:.3e} of max {mx:.3e} ({err / max(1.0, mx):.2e} of the scale)")
            assert err <= 1e-6 * max(1.0, mx), (k, err, mx)
    kV = (np.float32(inp.kappa) * d["V"]).astype(np.float32)
    margin = kV if loss.cap is None else np.minimum(kV, np.float32(loss.cap))
    pre = (d["Vdot"] + margin).astype(np.float32)
    assert np.array_equal(pre > 0, out.pre > 0)
    if loss.cap is not None:
        assert np.array_equal(kV > np.float32(loss.cap), out.kV > np.float32(loss.cap))
    assert int(sc[1]) == out.eff
    print(f"{tag} loss {sc[0]:.6f} ref {out.loss:.6f} (diff {abs(sc[0] - out.loss):.2e}), eff {out.eff}")
    assert abs(sc[0] - out.loss) <= 1e-5 * max(1.0, abs(out.loss))
    assert abs(sc[2] - out.mean_active) <= 1e-7
    for k, a, b in [("g_ftilde", d["g_ftilde"], out.g_ftilde)] + [(k, g[k], out.grads[k]) for k in GRAD_KEYS]:
        err, mx = float(np.abs(a - b).max()), float(np.abs(b).max())
        print(f"{tag} {k}: err {err:.3e} of max {mx:.3e} ({err / max(mx, 1e-30):.2e})")
        assert err <= 2e-4 * max(1e-6, mx), (k, err, mx)
    return sc, out


# ---- 1. parity, ReLU dynamics --------------------------------------------------------------------
@pytest.mark.parametrize("loss", R.RELU_LOSSES, ids=R.loss_id)
@pytest.mark.parametrize("B,S,sn", R.RELU_CASES)
def test_loss_step_matches_reference(B, S, sn, loss):
    P = make_params(seed=0)
    inp = make_step_inputs(B=B, S=S, seed=1, kappa=R.KAPPA)
    sc, gr, dbg = _run(P, inp, sn, loss)
    sc, out = _check_against_reference(P, inp, O.DynConfig(scale_nominal=sn), loss, sc, gr, dbg,
                                       f"[{B}x{S} sn={int(sn)} {R.loss_id(loss)}]")
    # a kernel computing the default loss instead lands outside every bound above
    assert abs(sc[0] - _default_loss((B, S, sn), P, inp, sn)) > 1e-3


# ---- 2. parity, GroupSort dynamics ---------------------------------------------------------------
@pytest.mark.parametrize("loss", R.GROUPSORT_LOSSES, ids=R.loss_id)
@pytest.mark.parametrize("B,S,seed,sn", R.GROUPSORT_CASES)
def test_groupsort_loss_step_matches_reference(B, S, seed, sn, loss, monkeypatch):
    monkeypatch.setattr(O, "mlp_forward", G.mlp_forward)
    monkeypatch.setattr(O, "mlp_backward", G.mlp_backward)
    P = make_params(seed=seed)
    inp = make_step_inputs(B=B, S=S, seed=seed + 1, kappa=R.KAPPA)
    cfg = O.DynConfig(scale_nominal=sn)
    # the near-tie condition of test_groupsort_train.py on the reference for these inputs
    ev = O.eval_dot(inp.h, np.repeat(O.static_projection(inp.x_feat, P), S, 0), P, cfg, inp.mask1, inp.mask2)
    assert G.pair_separation(ev.mlp, inp.mask1, inp.mask2) >= G.MIN_SEPARATION
    sc, gr, dbg = _run(P, inp, sn, loss, "GroupSort")
    sc, out = _check_against_reference(P, inp, cfg, loss, sc, gr, dbg, f"[GroupSort {B}x{S} {R.loss_id(loss)}]")
    assert abs(sc[0] - _default_loss(("gs", B, S, sn), P, inp, sn, "GroupSort")) > 1e-3


# ---- 3. the default config through fiode_lyap_step_loss --------------------------------------------
@pytest.mark.parametrize("activation", ["ReLU", "GroupSort"])
def test_default_config_through_loss_entry_point_equals_act(activation):
    """fiode_lyap_step_loss with {DECISION_BOUNDARY, RELU, +inf, 0} (and with NULL) against ops.lyap_step
    (fiode_lyap_step_act): scalars, gradients and debug outputs torch.equal."""
    from fiode_amd import ops, _lib as L
    B, S, seed = 3, 37, 337
    P = make_params(seed=seed)
    inp = make_step_inputs(B=B, S=S, seed=seed + 1)
    sc, gr, dbg = _run(P, inp, True, None, activation)
    dev = sc.device
    w = _wt(P, dev)
    masks = torch.from_numpy(np.stack([inp.mask1, inp.mask2, inp.lmask1, inp.lmask2])).to(dev)
    x, y, h = (torch.from_numpy(t).to(dev) for t in (inp.x_feat, inp.y, inp.h))
    cfg = L.LyapConfig(B, S, S, L.FIODE_SAMPLER_GIVEN, L.FIODE_DROPOUT_GIVEN, float(inp.kappa), 0, 0)
    dc = _dyn(True, activation).to_c()
    cw = L.DynWeights(*[w[k].data_ptr() for k in ops.WEIGHT_KEYS])
    lib = L.lib()
    ws = torch.empty(lib.fiode_lyap_workspace_bytes(ct.byref(cfg), ct.byref(dc)), dtype=torch.uint8, device=dev)
    for loss in (L.LyapLoss(L.FIODE_CAND_DECISION_BOUNDARY, L.FIODE_HINGE_RELU, float("inf"), 0), None):
        sc2 = torch.empty(8, device=dev)
        gr2 = {k: torch.empty_like(v) for k, v in gr.items()}
        dbg2 = {k: torch.empty_like(v) for k, v in dbg.items()}
        io = L.LyapIO(x.data_ptr(), y.data_ptr(), h.data_ptr(), masks.data_ptr(), sc2.data_ptr(),
                      *[dbg2[k].data_ptr() for k in ("h", "V", "Vdot", "f", "f_log", "qp_lower", "qp_nominal",
                                                     "g_ftilde")],
                      None, 0, None, None, None, dbg2["keep_words"].data_ptr(), None)
        cg = L.LyapGrads(*[gr2[k].data_ptr() for k in ops.WEIGHT_KEYS + ("x_feat",)])
        rc = lib.fiode_lyap_step_loss(ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream), ct.byref(cfg),
                                      ct.byref(dc), ct.byref(cw), ct.byref(io), ct.byref(cg),
                                      ct.c_void_p(ws.data_ptr()), ct.c_size_t(ws.numel()),
                                      ops.ACTIVATIONS[activation], ct.byref(loss) if loss is not None else None)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(sc, sc2)
        for k in gr:
            assert torch.equal(gr[k], gr2[k]), k
        assert set(dbg) == set(dbg2)
        for k in dbg:
            assert torch.equal(dbg[k], dbg2[k]), k


# ---- 4. edge rows ----------------------------------------------------------------------------------
def _edge_inputs():
    """B = 2, S = 32, dropout off: the rows of make_step_inputs with h = e_y, h = e_j (j != y) and
    h_y = 0 (the rest renormalised) written over the first three rows of each image."""
    inp = make_step_inputs(B=2, S=32, seed=11, dropout=False, kappa=R.KAPPA)
    h = inp.h.copy()
    for b in range(2):
        y = int(inp.y[b])
        r = b * 32
        h[r] = 0.0
        h[r, y] = 1.0
        h[r + 1] = 0.0
        h[r + 1, (y + 3) % 10] = 1.0
        h[r + 2, y] = 0.0
        h[r + 2] = h[r + 2] / h[r + 2].sum(dtype=np.float32)
    inp.h = h.astype(np.float32)
    return inp


@pytest.mark.parametrize("loss", [R.Loss("DynCrossEntropy", "elu"), R.Loss("OnemEtay", "elu"),
                                  R.Loss("CompositeL1", "relu"), R.Loss("CompositeL2", "identity", R.CAP)],
                         ids=R.loss_id)
def test_edge_rows_are_finite_and_match(loss):
    """Rows on the clamps (lc(0), lc' = 0): finite everywhere, V in its bound, g_ftilde as the reference."""
    P = make_params(seed=10)
    inp = _edge_inputs()
    # (without the nominal scaling: with it the sigmoid factor rounds g_ftilde of these inputs to 0 for the
    # candidates whose gradient has the label's entry alone)
    cfg = O.DynConfig(scale_nominal=False)
    sc, gr, dbg = _run(P, inp, False, loss)
    assert torch.isfinite(sc).all()
    for k, v in list(gr.items()) + [(k, v) for k, v in dbg.items() if v.dtype == torch.float32]:
        assert torch.isfinite(v).all(), k
    d = {k: v.cpu().numpy() for k, v in dbg.items()}
    inp.qp_inputs = (d["qp_lower"], d["qp_nominal"][0])
    inp.qp_inputs_log = (d["qp_lower"], d["qp_nominal"][1])
    out = R.lyapunov_step(inp, P, cfg, loss)
    assert np.isfinite(out.V64).all()
    if loss.candidate in BIT_EQUAL:
        assert np.array_equal(d["V"], out.V) and np.array_equal(d["Vdot"], out.Vdot)
    else:
        for k, r64 in (("V", out.V64), ("Vdot", out.Vdot64)):
            err, mx = float(np.abs(d[k] - r64).max()), float(np.abs(r64).max())
            print(f"edge {R.loss_id(loss)} {k}: err {err:.3e} of max {mx:.3e}")
            assert err <= 1e-6 * max(1.0, mx), (k, err, mx)
    if loss.hinge == "relu":
        # the one hinge whose derivative jumps at pre = 0 (on the edge rows OnemEtay and CompositeL2 have
        # pre = 0 exactly: they run with elu / identity here)
        assert not (np.abs(out.pre) <= R.PRE_BAND * np.maximum(1.0, np.abs(out.Vdot))).any()
    err = float(np.abs(d["g_ftilde"] - out.g_ftilde).max())
    mx = float(np.abs(out.g_ftilde).max())
    print(f"edge {R.loss_id(loss)} g_ftilde: err {err:.3e} of max {mx:.3e}")
    assert mx > 0 and err <= 2e-4 * mx


# ---- 5. module level ---------------------------------------------------------------------------------
CAP_KW = dict(relax_exp_stable=True, scaleLeps=0.05, eps=0.1)      # cap = 0.05 * 100 * 0.1 = 0.5


def _module(dev, seed=0, **kw):
    from fiode_amd.lyapunov import CompositeDynCrossEntropy
    from tests.test_lyap_loss_abi import build_module
    args = dict(lya_cand=CompositeDynCrossEntropy(on_simplex=True, norm_type="L1"), act="elu", **CAP_KW)
    args.update(kw)
    return build_module(seed=seed, **args).to(dev).train()


def _batch(dev, B=8):
    g = torch.Generator(device="cpu").manual_seed(5)
    return torch.rand(B, 3, 32, 32, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


def test_module_eager_step_equals_direct_call(monkeypatch):
    """LyapunovLearning (CompositeDynCrossEntropy L1, elu, relax_exp_stable) at B = 8, S = 32: the eager
    step's scalars and the dynamics' bias gradients are those of ops.lyap_step called directly with the
    tensors the module passed (the features and effective weights of its own forward) and this config."""
    from fiode_amd import ops
    dev = _dev()
    x, y = _batch(dev)
    mod = _module(dev)
    mod._rng_offset = 0
    cfg = mod.loss_cfg()
    assert cfg == ops.LossCfg("CompositeL1", "elu", 0.5)
    step, seen = ops.lyap_step, []

    def recorder(*a, **kw):
        seen.append((a, dict(kw)))
        return step(*a, **kw)
    monkeypatch.setattr(ops, "lyap_step", recorder)
    loss = mod.training_step((x, y))
    loss.backward()
    monkeypatch.setattr(ops, "lyap_step", step)
    plan = mod.last_plan
    assert len(seen) == 1 and seen[0][1]["loss"] == plan["loss"] == cfg
    (feat, yy, w, dyn), kw = seen[0]
    assert kw["seed"] == mod.seed and kw["offset"] == 0 and kw["kappa"] == plan["kappa"]
    direct = dict(sample_size=plan["S"], n_uniform=plan["S1"], sampler=plan["sampler"],
                  dropout_mode=plan["dropout_mode"], kappa=plan["kappa"], seed=mod.seed, offset=0)
    sc, gr, dbg = ops.lyap_step(feat, yy, w, dyn, debug=True, loss=cfg, **direct)
    torch.cuda.synchronize()
    assert torch.equal(plan["scalars"], sc) and torch.equal(loss.detach(), sc[0])
    d = mod.dyn_fun
    for name, p in (("b1", d.hidden_to_mlp.bias), ("bx", d.U_x.bias), ("b2", d.mlp_to_mlp.bias),
                    ("b3", d.mlp_to_hidden.bias)):
        assert torch.equal(p.grad, gr[name]), name
    # the cap binds on some rows and not on all
    capped = (plan["kappa"] * dbg["V"] > 0.5).float().mean().item()
    print(f"capped share {capped:.3f}, eff {int(sc[1])} of {dbg['V'].numel()}")
    assert 0.0 < capped < 1.0
    # the same step with the default loss is another loss
    sc0, _, _ = ops.lyap_step(feat, yy, w, dyn, **direct)
    assert abs(float(sc0[0]) - float(sc[0])) > 1e-3


def test_module_graph_replay_equals_eager_step():
    """The comparison of test_gpu_graph.py with the loss config on: the captured step follows it."""
    from fiode_amd.graph_step import GraphTrainStep
    dev = _dev()
    x, y = _batch(dev)
    mod = _module(dev)
    opt = mod.configure_optimizers(capturable=True)[0][0]
    gs = GraphTrainStep(mod, opt, x, y, warmup=2, act="elu")
    twin = _module(dev, seed=1)
    twin.load_state_dict(mod.state_dict())
    twin.rng_counter = mod.rng_counter.clone()
    twin.seed = mod.seed
    loss = gs.step()
    torch.cuda.synchronize()
    graph_grads = [p.grad.clone() for p in mod.parameters() if p.requires_grad]
    l2 = twin.compute_loss(x, y, 8, "elu")
    l2.backward()
    eager_grads = [p.grad for p in twin.parameters() if p.requires_grad]
    torch.testing.assert_close(loss, l2, rtol=1e-5, atol=1e-6)
    for a, b in zip(graph_grads, eager_grads):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    # the twin with the default hinge and no cap is another loss: the capture did not drop the config
    twin.relax_exp_stable = False                # (same device counter: an eager compute_loss does not advance it)
    l3 = twin.compute_loss(x, y, 8, "relu")
    assert abs(float(l3.detach()) - float(l2.detach())) > 1e-3
    gs.close()


def test_module_train_ode_fused_node_equals_three_nodes():
    """train_ode past train_ode_epoch (rk4, step 0.25) with the loss config on: LyapODELossFn = the
    three-node graph bit for bit (the comparison of test_gpu_odetrain.py)."""
    from fiode_amd import lyapunov as LY
    dev = _dev()
    x, y = _batch(dev)
    out = {}
    LY.DYN_WGRAD_SIDE = False
    try:
        for variant in ("fused", "three", "three-default"):
            kw = dict(act="relu", relax_exp_stable=False, lya_cand=None) if variant == "three-default" else {}
            mod = _module(dev, train_ode=True, **kw)
            assert mod.ode_branch_active()
            mod.parallel_cayley = False
            mod.fused_ode_loss = variant == "fused"
            mod._rng_offset = 0
            loss = mod.training_step((x, y))
            loss.backward()
            torch.cuda.synchronize()
            assert mod.last_plan["loss"] == mod.loss_cfg()
            out[variant] = (loss.detach().clone(), float(mod.logged["loss_ode"]),
                            {n: p.grad.detach().clone() for n, p in mod.named_parameters() if p.requires_grad})
    finally:
        LY.DYN_WGRAD_SIDE = True
    (la, oa, ga), (lb, ob, gb) = out["fused"], out["three"]
    assert torch.equal(la, lb) and oa == ob
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    assert abs(float(la) - float(out["three-default"][0])) > 1e-4      # (p = 0.2: the Lyapunov term moved)


def test_decision_boundary_log_mode_trains_as_log_mode():
    from fiode_amd.lyapunov import DecisionBoundary
    dev = _dev()
    x, y = _batch(dev)
    losses = []
    for log_mode in (False, True):
        mod = _module(dev, lya_cand=DecisionBoundary(on_simplex=True, log_mode=log_mode), act="relu",
                      relax_exp_stable=False)
        mod._rng_offset = 0
        losses.append(float(mod.training_step((x, y))))
    print("DecisionBoundary losses (log_mode False, True):", losses)
    assert np.isfinite(losses).all() and abs(losses[0] - losses[1]) > 1e-3


# ---- 6. reproducibility -------------------------------------------------------------------------------
def test_loss_step_is_bit_reproducible():
    B, S, sn = R.RELU_CASES[-1]
    P = make_params(seed=0)
    inp = make_step_inputs(B=B, S=S, seed=1, kappa=R.KAPPA)
    runs = []
    for _ in range(2):
        sc, gr, dbg = _run(P, inp, sn, R.Loss("CompositeL2", "elu", R.CAP))
        runs.append((sc.clone(), {k: v.clone() for k, v in gr.items()}, {k: v.clone() for k, v in dbg.items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
