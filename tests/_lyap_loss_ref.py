"""Reference of the fused Lyapunov step with a loss config (fiode_lyap_step_loss; test_lyap_loss_ref.py,
test_lyap_loss_abi.py, test_gpu_lyap_loss.py).

Per row, with h on the simplex, y the label, f the QP output of the loss pass, C = 10:

    Vdot = <grad V(h), f>,  margin = min(kappa V, cap),  pre = Vdot + margin,  viol = hinge(pre),
    loss = mean(viol),  eff = #(viol > 0),  d loss / d f = hinge'(pre) / N * grad V(h)

The candidates (lya_cands.py, on_simplex=True), with lc(x) = log(max(x, 1e-12)) and lc'(x) = 1 / x for
x >= 1e-12, 0 below (torch.clamp's gradient), j* = the first index of max_{j != y} h_j:

    DecisionBoundary      V = (1 + h_j*) - h_y                              grad = e_j* - e_y
    DecisionBoundaryLog   V = log(V_lin)                                    grad = (e_j* - e_y) / V_lin
    DynCrossEntropy       V = -lc(h_y)                                      grad = -lc'(h_y) e_y
    OnemEtay              V = -h_y                                          grad = -e_y
    CompositeL1           V = (-sum_j lc(1-h_j) + lc(1-h_y) - lc(h_y)) / C  j != y: lc'(1-h_j) / C;  y: -lc'(h_y) / C
    CompositeL2           V = (sum_j lc(1-h_j)^2 - lc(1-h_y)^2 + lc(h_y)^2) / C
                                              j != y: -2 lc(1-h_j) lc'(1-h_j) / C;  y: 2 lc(h_y) lc'(h_y) / C

Two forms: ``cand_f64`` (the table in float64) and ``cand_f32`` (float32 after every operation, in the
kernel's order: the label's lc(1 - h_y) terms cancel, so the Composite sums run over the wrong classes,
left to right).  ``lyapunov_step`` is ``oracle.fiode_oracle.lyapunov_step`` with the loss as a parameter,
built from the oracle's eval_dot / qp_backward / mlp_backward (looked up on the module at call time, so a
test that installs the GroupSort MLP of tests/_groupsort_train_ref.py gets a GroupSort step); with the
default config it is that function bit for bit.
"""
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from oracle import fiode_oracle as O

F32 = np.float32
NC = 10
CANDIDATES = ("DecisionBoundary", "DecisionBoundaryLog", "DynCrossEntropy", "OnemEtay", "CompositeL1", "CompositeL2")
HINGES = ("relu", "elu", "identity")
CLAMP = 1e-12


@dataclass(frozen=True)
class Loss:
    candidate: str = "DecisionBoundary"
    hinge: str = "relu"
    cap: Optional[float] = None     # None: no cap


# ---- float64: the table ---------------------------------------------------------------------------

def _lc(x):
    return np.log(np.maximum(x, CLAMP))


def _dlc(x):
    with np.errstate(divide="ignore"):
        return np.where(x >= CLAMP, 1.0 / np.where(x >= CLAMP, x, 1.0), 0.0)


def cand_f64(name, h, y_rows):
    """(V [N], grad V [N, C]) in float64 of float32 rows h."""
    h = np.asarray(h, np.float64)
    N = h.shape[0]
    r = np.arange(N)
    y = np.asarray(y_rows, np.int64)
    hy = h[r, y]
    g = np.zeros_like(h)
    if name in ("DecisionBoundary", "DecisionBoundaryLog"):
        js = O.runner_up(np.asarray(h, F32), y)
        lin = (1.0 + h[r, js]) - hy
        with np.errstate(divide="ignore"):
            s = 1.0 / lin if name == "DecisionBoundaryLog" else np.ones(N)
            V = np.log(lin) if name == "DecisionBoundaryLog" else lin
        g[r, js] = s
        g[r, y] = -s
        return V, g
    if name == "DynCrossEntropy":
        g[r, y] = -_dlc(hy)
        return -_lc(hy), g
    if name == "OnemEtay":
        g[r, y] = -1.0
        return -hy, g
    om = 1.0 - h
    if name == "CompositeL1":
        V = (-_lc(om).sum(1) + _lc(1.0 - hy) - _lc(hy)) / NC
        g = _dlc(om) / NC
        g[r, y] = -_dlc(hy) / NC
        return V, g
    if name == "CompositeL2":
        V = ((_lc(om) ** 2).sum(1) - _lc(1.0 - hy) ** 2 + _lc(hy) ** 2) / NC
        g = -2.0 * _lc(om) * _dlc(om) / NC
        g[r, y] = 2.0 * _lc(hy) * _dlc(hy) / NC
        return V, g
    raise KeyError(name)


# ---- float32 per operation, the kernel's order ----------------------------------------------------

def _lc32(x):
    return np.log(np.maximum(x, F32(CLAMP))).astype(F32)


def _dlc32(x):
    ok = x >= F32(CLAMP)
    return np.where(ok, F32(1) / np.where(ok, x, F32(1)), F32(0)).astype(F32)


def cand_f32(name, h, y_rows):
    """(V [N], grad V [N, C]) rounded to float32 after every operation."""
    h = np.asarray(h, F32)
    N = h.shape[0]
    r = np.arange(N)
    y = np.asarray(y_rows, np.int64)
    hy = h[r, y]
    g = np.zeros_like(h)
    if name in ("DecisionBoundary", "DecisionBoundaryLog"):
        js = O.runner_up(h, y)
        lin = ((F32(1) + h[r, js]).astype(F32) - hy).astype(F32)
        if name == "DecisionBoundaryLog":
            with np.errstate(divide="ignore"):
                s, V = (F32(1) / lin).astype(F32), np.log(lin).astype(F32)
        else:
            s, V = np.ones(N, F32), lin
        g[r, js] = s
        g[r, y] = -s
        return V, g
    if name == "DynCrossEntropy":
        g[r, y] = -_dlc32(hy)
        return (-_lc32(hy)).astype(F32), g
    if name == "OnemEtay":
        g[r, y] = F32(-1)
        return (-hy).astype(F32), g
    if name not in ("CompositeL1", "CompositeL2"):
        raise KeyError(name)
    l2 = name == "CompositeL2"
    om = (F32(1) - h).astype(F32)
    l, d = _lc32(om), _dlc32(om)
    ly, dy = _lc32(hy), _dlc32(hy)
    term = (l * l).astype(F32) if l2 else (-l).astype(F32)
    term[r, y] = F32(0)
    acc = O.row_sum_seq(term)
    acc = (acc + ((ly * ly).astype(F32) if l2 else (-ly).astype(F32))).astype(F32)
    gw = ((F32(-2) * l).astype(F32) * d).astype(F32) if l2 else d
    gy = ((F32(2) * ly).astype(F32) * dy).astype(F32) if l2 else (-dy).astype(F32)
    gw = gw.copy()
    gw[r, y] = gy
    return (acc / F32(NC)).astype(F32), (gw / F32(NC)).astype(F32)


def hinge(name, pre):
    """(viol, d viol / d pre) in the dtype of ``pre``: th.relu, F.elu (alpha 1), identity."""
    pre = np.asarray(pre)
    one, zero = pre.dtype.type(1), pre.dtype.type(0)
    if name == "relu":
        return np.maximum(pre, zero), np.where(pre > 0, one, zero)
    if name == "elu":
        neg = np.minimum(pre, zero)          # (the branch not taken must not overflow)
        return (np.where(pre > 0, pre, np.expm1(neg)).astype(pre.dtype),
                np.where(pre > 0, one, np.exp(neg)).astype(pre.dtype))
    if name == "identity":
        return pre.copy(), np.ones_like(pre)
    raise KeyError(name)


@dataclass
class LossStepOutputs:
    loss: float
    eff: int
    mean_active: float
    V: np.ndarray            # float32 per op
    Vdot: np.ndarray
    V64: np.ndarray          # float64 closed form of the same float32 h and f
    Vdot64: np.ndarray
    kV: np.ndarray           # kappa * V (float32): the uncapped margin
    pre: np.ndarray
    viol: np.ndarray
    f: np.ndarray
    f_log: np.ndarray
    g_ftilde: np.ndarray
    qp_iters: int
    qp_iters_log: int
    grads: Dict[str, np.ndarray] = field(default_factory=dict)


def lyapunov_step(inp: O.StepInputs, P: O.DynParams, cfg: O.DynConfig, loss: Loss = Loss()) -> LossStepOutputs:
    """``O.lyapunov_step`` with the loss of ``loss``; QP inputs can be pinned through ``inp`` as there."""
    N, C = inp.h.shape
    B, S = inp.x_feat.shape[0], inp.S
    assert N == B * S and C == NC
    y_rows = np.repeat(np.asarray(inp.y, np.int64), S)
    u_rows = np.repeat(O.static_projection(inp.x_feat, P), S, axis=0)
    ev = O.eval_dot(inp.h, u_rows, P, cfg, inp.mask1, inp.mask2, qp_inputs=inp.qp_inputs)
    V, gv = cand_f32(loss.candidate, inp.h, y_rows)
    Vd = O.row_sum_seq((gv * ev.f).astype(F32))
    V64, gv64 = cand_f64(loss.candidate, inp.h, y_rows)
    Vd64 = (gv64 * ev.f.astype(np.float64)).sum(1)
    kV = (F32(inp.kappa) * V).astype(F32)
    margin = kV if loss.cap is None else np.minimum(kV, F32(loss.cap))
    pre = (Vd + margin).astype(F32)
    viol, dh = hinge(loss.hinge, pre)
    viol = viol.astype(F32)
    total = float(np.sum(viol, dtype=np.float64) / N)
    eff = int((viol > 0).sum())

    evl = O.eval_dot(inp.h, u_rows, P, cfg, inp.lmask1, inp.lmask2, qp_inputs=inp.qp_inputs_log)
    lin_lower = (F32(-cfg.alpha_1) * np.asarray(inp.h, F32)).astype(F32)
    upper = O.barrier_upper(inp.h, cfg)
    act = (np.abs((evl.f - lin_lower).astype(F32)) <= F32(1e-6)) | (np.abs((evl.f - upper).astype(F32)) <= F32(1e-6))
    mean_active = float(act.mean())

    g_pre = (dh.astype(F32) * F32(1.0 / N)).astype(F32)
    g_f = (g_pre[:, None] * gv).astype(F32)
    _, g_nom = O.qp_backward(g_f, ev.f, ev.qp.mu, ev.lower, ev.nominal)
    if cfg.scale_nominal:
        span = (O.barrier_upper(inp.h, cfg) - ev.lower).astype(F32)
        g_ft = ((g_nom * span).astype(F32) * ((F32(1) - ev.sig) * ev.sig).astype(F32)).astype(F32)
    else:
        g_ft = g_nom
    grads = O.mlp_backward(g_ft, inp.h, inp.x_feat, S, P, ev.mlp, inp.mask1, inp.mask2, cfg.dropout)
    return LossStepOutputs(loss=total, eff=eff, mean_active=mean_active, V=V, Vdot=Vd, V64=V64, Vdot64=Vd64, kV=kV,
                           pre=pre, viol=viol, f=ev.f, f_log=evl.f, g_ftilde=g_ft, qp_iters=ev.qp.iters,
                           qp_iters_log=evl.qp.iters, grads=grads)


# ---- the parity cases of test_gpu_lyap_loss.py and the conditions they need -------------------------
# (B, S, scale_nominal) with make_params(seed=0), make_step_inputs(B, S, seed=1, kappa=1.0), given masks
RELU_CASES = [(4, 8, True), (4, 8, False), (3, 37, True), (16, 64, False)]
KAPPA = 1.0
CAP = 1.0
RELU_LOSSES = ([Loss(c, "relu") for c in CANDIDATES[1:]] +
               [Loss("DecisionBoundaryLog", "elu"), Loss("DecisionBoundaryLog", "identity"),
                Loss("DecisionBoundary", "relu", CAP), Loss("CompositeL2", "relu", CAP)])
# GroupSort dynamics: (B, S, seed, scale_nominal) of tests/_groupsort_train_ref.PARITY_CASES (no pre-sort pair
# closer than 2e-5 on the loss pass), kappa 1.0
GROUPSORT_CASES = [(3, 37, 337, True), (16, 64, 1692, False)]
GROUPSORT_LOSSES = [Loss("DynCrossEntropy", "elu"), Loss("CompositeL2", "relu")]
PRE_BAND = 1e-4      # no row with |pre| <= PRE_BAND * max(1, |Vdot|): device and reference agree on its sign
CAP_BAND = 1e-5      # no row with |kappa V - cap| <= CAP_BAND: both cap the same rows


def loss_id(loss: Loss) -> str:
    return f"{loss.candidate}-{loss.hinge}" + ("" if loss.cap is None else f"-cap{loss.cap:g}")


def input_conditions(out: LossStepOutputs, loss: Loss) -> dict:
    """The figures the parity tests' input conditions are about (asserted by ``check_input_conditions``)."""
    band = np.abs(out.pre) <= PRE_BAND * np.maximum(1.0, np.abs(out.Vdot))
    res = dict(in_pre_band=int(band.sum()), positive=float((out.pre > 0).mean()))
    if loss.cap is not None:
        res["in_cap_band"] = int((np.abs(out.kV - F32(loss.cap)) <= CAP_BAND).sum())
        res["capped"] = float((out.kV > F32(loss.cap)).mean())
    return res


def check_input_conditions(out: LossStepOutputs, loss: Loss) -> dict:
    c = input_conditions(out, loss)
    assert c["in_pre_band"] == 0, c
    if not (loss.candidate == "DecisionBoundary"):
        assert 0.0 < c["positive"] < 1.0, c         # both hinge branches present
    if loss.cap is not None:
        assert c["in_cap_band"] == 0, c
        assert 0.10 <= c["capped"] <= 0.90, c
    return c
