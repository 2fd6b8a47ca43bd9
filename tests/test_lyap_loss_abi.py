"""CPU checks of the loss config of the fused Lyapunov step: the additive C-ABI (fiode_lyap_step_loss,
fiode_lyap_loss, FIODE_CAND_* / FIODE_HINGE_*), ``ops.LossCfg`` / ``ops.lyap_step(loss=...)`` and the module
surface (the candidate classes, ``LyapunovLearning``'s act / relax_exp_stable / scaleLeps, ``loss_cfg``)."""
import ctypes as ct
import math
import pathlib
import re

import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
CANDS = ("DECISION_BOUNDARY", "DECISION_BOUNDARY_LOG", "DYN_CROSS_ENTROPY", "ONEM_ETAY", "COMPOSITE_L1", "COMPOSITE_L2")
HINGES = ("RELU", "ELU", "IDENTITY")


def build_module(seed=0, h_sample_size=32, **kw):
    """A LyapunovLearning as bench.build_module builds it (host tensors), S = 32, with ``kw`` on top."""
    from fiode_amd.lyapunov import LyapunovLearning, UniformInitFun
    from fiode_amd.models import make_ortho_KWLarge_Concat
    from fiode_amd.sampling import (CompositeSampler, CompositeSamplerScheduler, CorrectConeSampling,
                                    LinearScheduler, UniformSimplexSampling)
    from tests.test_groupsort_dyn import _dyn
    torch.manual_seed(seed)
    backbone = make_ortho_KWLarge_Concat(out_dim=10, act="GroupSort")
    sampler = CompositeSampler((10,), [UniformSimplexSampling(), CorrectConeSampling()])
    sched = CompositeSamplerScheduler([LinearScheduler(-0.02, 1.0, "min", 0.02, 10),
                                       LinearScheduler(0.02, 0.0, "max", 0.98, 10)], [1.0, 1.0])
    args = dict(order=1, h_sample_size=h_sample_size, h_dist_lim=15.0, sampler=sampler, sampler_scheduler=sched,
                dynamics=_dyn(kw.pop("activation", "ReLU")), init_fun=UniformInitFun((10,), backbone), t_max=1.0,
                opt_name="Adam", lr=5e-3, train_ode=False, train_ode_epoch=10, train_ode_solver="rk4",
                train_ode_tol=0.25, val_ode_solver="dopri5", val_ode_tol=1e-3, weight_decay=0.0, warmup=-1,
                max_epochs=300, simplex=True, act="relu", val_adv=False, seed=seed)
    args.update(kw)
    mod = LyapunovLearning(**args)
    mod.current_epoch = 20
    mod.dyn_fun.scale_nominal = False
    return mod


# ---- the C-ABI ------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_loss_entry_point():
    from fiode_amd import _lib as L
    text = (ROOT / "include" / "fiode.h").read_text()
    syms = re.findall(r"FIODE_API\s+[\w\s\*]+?\b(fiode_\w+)\s*\(", text)
    assert "fiode_lyap_step_loss" in syms and hasattr(L.lib(), "fiode_lyap_step_loss")
    assert "typedef struct fiode_lyap_loss" in text
    for i, n in enumerate(CANDS):
        assert re.search(rf"FIODE_CAND_{n}\s*=\s*{i}\b", text), n
        assert getattr(L, f"FIODE_CAND_{n}") == i
    for i, n in enumerate(HINGES):
        assert re.search(rf"FIODE_HINGE_{n}\s*=\s*{i}\b", text), n
        assert getattr(L, f"FIODE_HINGE_{n}") == i
    assert ct.sizeof(L.LyapLoss) == 16
    assert [f[0] for f in L.LyapLoss._fields_] == ["candidate", "hinge", "margin_cap", "reserved"]
    assert L.lib().fiode_abi_version() == 5 == L.ABI_VERSION


def _call(lib, L, loss, *, act=0, nbytes=0):
    d = ct.c_void_p(1)
    dyn = L.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
    cfg = L.LyapConfig(4, 8, 8, L.FIODE_SAMPLER_COMPOSITE, L.FIODE_DROPOUT_PHILOX, 2.0, 0, 0)
    w = L.DynWeights(*([d] * 8))
    io = L.LyapIO(*([d] * 5 + [None] * 9 + [0] + [None] * 5))
    g = L.LyapGrads(*([d] * 9))
    return lib.fiode_lyap_step_loss(None, ct.byref(cfg), ct.byref(dyn), ct.byref(w), ct.byref(io), ct.byref(g), d,
                                    nbytes, act, ct.byref(loss) if loss is not None else None)


def test_loss_entry_point_host_argument_checks():
    """Every argument check (the loss config included) runs before the workspace-size check and nothing
    is launched on an error: dummy non-NULL pointers and a zero-byte workspace give FIODE_EWORKSPACE for
    every valid config and FIODE_EINVAL for every invalid one."""
    from fiode_amd import _lib as L
    lib = L.lib()
    inf = math.inf
    assert _call(lib, L, None) == L.FIODE_EWORKSPACE
    for c in range(6):
        for h in range(3):
            for cap in (inf, 1.0, 0.0, -inf):
                for act in (0, 1):
                    assert _call(lib, L, L.LyapLoss(c, h, cap, 0), act=act) == L.FIODE_EWORKSPACE, (c, h, cap, act)
    for bad in (L.LyapLoss(6, 0, inf, 0), L.LyapLoss(-1, 0, inf, 0), L.LyapLoss(0, 3, inf, 0),
                L.LyapLoss(0, -1, inf, 0), L.LyapLoss(0, 0, math.nan, 0), L.LyapLoss(0, 0, inf, 1),
                L.LyapLoss(5, 2, 1.0, -7)):
        assert _call(lib, L, bad) == L.FIODE_EINVAL, (bad.candidate, bad.hinge, bad.margin_cap, bad.reserved)
    assert _call(lib, L, L.LyapLoss(0, 0, inf, 0), act=2) == L.FIODE_EINVAL      # the activation, as _act


# ---- ops ------------------------------------------------------------------------------------------
def test_loss_cfg_maps_to_the_struct():
    from fiode_amd import ops, _lib as L
    c = ops.LossCfg("CompositeL2", "elu", 0.25).to_c()
    assert (c.candidate, c.hinge, c.margin_cap, c.reserved) == (L.FIODE_CAND_COMPOSITE_L2, L.FIODE_HINGE_ELU, 0.25, 0)
    c = ops.LossCfg("OnemEtay").to_c()
    assert (c.candidate, c.hinge, c.margin_cap, c.reserved) == (L.FIODE_CAND_ONEM_ETAY, L.FIODE_HINGE_RELU, math.inf, 0)
    assert ops.LossCfg("DecisionBoundary").is_default and ops.LossCfg("DecisionBoundary", "relu", math.inf).is_default
    assert not ops.LossCfg("DecisionBoundary", "relu", 1.0).is_default
    assert not ops.LossCfg("DecisionBoundary", "identity").is_default
    assert not ops.LossCfg("DecisionBoundaryLog").is_default
    assert sorted(ops.CANDIDATES.values()) == list(range(6)) and sorted(ops.HINGES.values()) == [0, 1, 2]
    for bad in (dict(candidate="MSELoss"), dict(candidate="DecisionBoundary", hinge="gelu"),
                dict(candidate="OnemEtay", margin_cap=math.nan)):
        with pytest.raises(ValueError):
            ops.LossCfg(**bad)


class _FakeLib:
    """Records which step symbol ops.lyap_step calls (nothing runs)."""

    def __init__(self, symbols):
        self.calls = []
        for s in symbols:
            setattr(self, s, self._recorder(s))

    def _recorder(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn

    def fiode_lyap_workspace_bytes(self, *a):
        return 256


def _lyap_step_on_host(monkeypatch, fake, loss):
    from fiode_amd import ops, _lib as L
    monkeypatch.setattr(L, "lib", lambda: fake)
    monkeypatch.setattr(ops, "_need", lambda t, *a: t.contiguous())
    monkeypatch.setattr(ops, "_stream", lambda dev: None)
    monkeypatch.setattr(ops._Workspace, "get", classmethod(lambda cls, dev, n, tag, zero=False:
                                                           torch.empty(n, dtype=torch.uint8)))
    w = {k: torch.zeros(ops.WEIGHT_SHAPES[k]) for k in ops.WEIGHT_KEYS}
    kw = {} if loss == "absent" else {"loss": loss}
    ops.lyap_step(torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64), w, ops.DynCfg(), sample_size=4,
                  n_uniform=4, **kw)
    return fake.calls


def test_default_loss_takes_the_old_symbol(monkeypatch):
    from fiode_amd import ops
    all_syms = ("fiode_lyap_step", "fiode_lyap_step_act", "fiode_lyap_step_loss")
    for loss in ("absent", None, ops.LossCfg("DecisionBoundary"), ops.LossCfg("DecisionBoundary", "relu", math.inf)):
        calls = _lyap_step_on_host(monkeypatch, _FakeLib(all_syms), loss)
        assert [c[0] for c in calls] == ["fiode_lyap_step_act"], loss
        assert len(calls[0][1]) == 9
    # an older library under an A/B (no _act, no _loss): the default still runs, through fiode_lyap_step
    calls = _lyap_step_on_host(monkeypatch, _FakeLib(all_syms[:1]), None)
    assert [c[0] for c in calls] == ["fiode_lyap_step"]
    # a non-default config: the new symbol, the struct last
    calls = _lyap_step_on_host(monkeypatch, _FakeLib(all_syms), ops.LossCfg("CompositeL1", "elu", 0.5))
    assert [c[0] for c in calls] == ["fiode_lyap_step_loss"]
    assert len(calls[0][1]) == 10 and calls[0][1][8] == 0
    from fiode_amd import _lib as L
    with pytest.raises(L.FiodeLibraryError, match="fiode_lyap_step_loss"):
        _lyap_step_on_host(monkeypatch, _FakeLib(all_syms[:2]), ops.LossCfg("OnemEtay"))
    with pytest.raises(TypeError):
        _lyap_step_on_host(monkeypatch, _FakeLib(all_syms), "CompositeL1")


# ---- the module surface ---------------------------------------------------------------------------
def _candidates():
    from fiode_amd import lyapunov as ly
    return [(ly.DecisionBoundary(on_simplex=True), "DecisionBoundary"),
            (ly.DecisionBoundary(on_simplex=False), "DecisionBoundary"),
            (ly.DecisionBoundary(on_simplex=True, log_mode=True), "DecisionBoundaryLog"),
            (ly.DynCrossEntropy(on_simplex=True), "DynCrossEntropy"),
            (ly.OnemEtay(on_simplex=True), "OnemEtay"),
            (ly.CompositeDynCrossEntropy(on_simplex=True), "CompositeL1"),
            (ly.CompositeDynCrossEntropy(on_simplex=True, norm_type="L1"), "CompositeL1"),
            (ly.CompositeDynCrossEntropy(on_simplex=True, norm_type="L2"), "CompositeL2")]


def test_candidate_modules_work_as_plain_modules():
    """Constructor fields and defaults of lya_cands.py; forward on the eval path (host tensors)."""
    from fiode_amd import lyapunov as ly
    h = torch.softmax(torch.randn(5, 10, generator=torch.Generator().manual_seed(0)), 1)
    y = torch.tensor([0, 3, 9, 3, 1])
    for cls in (ly.DynCrossEntropy, ly.OnemEtay, ly.CompositeDynCrossEntropy, ly.MSELoss, ly.DecisionBoundary):
        assert cls().on_simplex is False
    assert ly.CompositeDynCrossEntropy().norm_type == "L1" and ly.MSELoss().num_class == 10
    with pytest.raises(AssertionError):
        ly.CompositeDynCrossEntropy(norm_type="L3")
    for m, _ in _candidates():
        v = m(h, y)
        assert v.shape == (5,) and torch.isfinite(v).all()
    assert ly.MSELoss(on_simplex=True)(h, y).shape == (5, 10)
    hy = h[torch.arange(5), y]
    torch.testing.assert_close(ly.OnemEtay(on_simplex=True)(h, y), -hy)
    torch.testing.assert_close(ly.DynCrossEntropy(on_simplex=True)(h, y), -torch.log(hy))
    # off the simplex: logits through softmax / cross entropy
    z = torch.randn(5, 10, generator=torch.Generator().manual_seed(1))
    torch.testing.assert_close(ly.DynCrossEntropy()(z, y), torch.nn.functional.cross_entropy(z, y, reduction="none"))
    torch.testing.assert_close(ly.CompositeDynCrossEntropy(norm_type="L2")(z, y),
                               ly.CompositeDynCrossEntropy(True, "L2")(torch.softmax(z, 1), y))


def test_loss_cfg_of_the_module():
    from fiode_amd import ops
    for cand, name in _candidates():
        mod = build_module(lya_cand=cand)
        assert mod.loss_cfg() == ops.LossCfg(name, "relu", None)
        assert mod.loss_cfg("elu") == ops.LossCfg(name, "elu", None)
        assert mod.loss_cfg("none").hinge == "identity" and mod.loss_cfg("linear").hinge == "identity"
    mod = build_module(act="elu")
    assert mod.act == "elu" and mod.loss_cfg() == ops.LossCfg("DecisionBoundary", "elu", None)
    assert mod.loss_cfg("relu").is_default
    assert build_module(act="identity").loss_cfg().hinge == "identity"
    # relax_exp_stable: cap = scaleLeps * alpha_1 * eps in Python floats (pl_modules.py:453)
    mod = build_module(relax_exp_stable=True)
    assert mod.loss_cfg().margin_cap == 3.0 * 100.0 * (36 / 255)
    mod = build_module(relax_exp_stable=True, scaleLeps=0.5, eps=0.01)
    assert mod.loss_cfg() == ops.LossCfg("DecisionBoundary", "relu", 0.5 * 100.0 * 0.01)
    assert build_module(scaleLeps=0.5, eps=0.01).loss_cfg().margin_cap is None
    # step_plan carries it to every ops.lyap_step call
    mod = build_module(lya_cand=_candidates()[7][0], relax_exp_stable=True, scaleLeps=0.01, eps=1.0)
    y = torch.zeros(4, dtype=torch.int64)
    assert mod.step_plan(y, act="elu")["loss"] == ops.LossCfg("CompositeL2", "elu", 0.01 * 100.0 * 1.0)
    assert mod.step_plan(y)["loss"] == ops.LossCfg("CompositeL2", "relu", 1.0)


class _Other(torch.nn.Module):
    on_simplex = True

    def forward(self, h, y):
        return h.sum(1)


def test_refusals_come_before_any_tensor_is_touched():
    from fiode_amd import lyapunov as ly

    class Sub(ly.DecisionBoundary):
        pass

    bad = [ly.MSELoss(on_simplex=True), _Other(), Sub(on_simplex=True), ly.DynCrossEntropy(), ly.OnemEtay(),
           ly.CompositeDynCrossEntropy(norm_type="L2"), ly.DecisionBoundary(on_simplex=False, log_mode=True)]
    for cand in bad:
        with pytest.raises(NotImplementedError):
            build_module(lya_cand=cand)
    with pytest.raises(NotImplementedError, match="MSELoss"):
        ly.fused_candidate(bad[0])
    with pytest.raises(NotImplementedError, match="on_simplex=False"):
        ly.fused_candidate(bad[3])
    with pytest.raises(NotImplementedError, match="barrier_loss"):
        build_module(barrier_loss=True)
    for kw in (dict(lips_train=True), dict(adv_train=True)):
        with pytest.raises(NotImplementedError):
            build_module(**kw)
    # a candidate swapped in after construction: compute_loss refuses with x and y never read
    mod = build_module()
    for cand in bad:
        mod.lya_cand = cand
        with pytest.raises(NotImplementedError):
            mod.compute_loss(None, None)
        with pytest.raises(NotImplementedError):
            mod.training_step((torch.zeros(2, 3, 32, 32), None))      # (reads the batch size only)
