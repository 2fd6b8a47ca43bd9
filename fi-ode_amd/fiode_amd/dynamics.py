"""OrthoClassDynProjectSimplexLips with its per-sample work on the GPU (libfiode.so).

Mirror of dynamics/classification.py:31-132: same constructor fields, same submodule names and
state_dict keys (hidden_to_mlp / mlp_to_mlp / mlp_to_hidden / U_x with weight, bias, alpha;
buffer static_state), same methods.  ``eval_dot`` / ``eval_dot_light`` / ``ode_forward`` run the
fused HIP kernels (MLP + barrier + bisection QP with the reference's batch-global exit) for
``activation`` 'ReLU' or 'GroupSort'.  In eval mode (or with dropout 0) they are differentiable like
the reference's: with grad enabled and ``h``, ``x`` or a parameter requiring grad, the call goes
through ``_EvalDotFn``, whose backward is the fused HIP vector-Jacobian product
(``ops.dyn_eval_backward``) for both activations, and the gradients reach the parameters through
``effective_weights()``' own autograd (the Cayley maps).  One derivative only: a double backward
raises.  The training-mode eval_dot with dropout is fused, with its backward, into the Lyapunov
step and the train_ode solve (``fiode_amd.lyapunov``).  The Lyapunov step implements both
activations, GroupSort behind the opt-in switch ``ops.GROUPSORT_TRAINING``; so does the rk4
train_ode solve, GroupSort behind the second switch ``ops.GROUPSORT_TRAIN_ODE`` (on the 16-row-tile
kernels for every batch size); the dopri5 train_ode solve implements 'ReLU' only.  Training a
GroupSort module raises NotImplementedError with the switches off; with only the first on, once the
train_ode branch is active; with both on, only when ``train_ode_solver`` is 'dopri5'.
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops
from .cayley import CayleyLinear, GroupSort, cayley_scaled
from .streams import prefetch, take


class _EvalDotFn(torch.autograd.Function):
    """eval_dot in eval mode over (h, x, effective weights): forward ``ops.dyn_eval``, backward
    ``ops.dyn_eval_backward``.  It saves its inputs and the forward's device exit iteration only (the
    backward recomputes the rest), so nothing depends on a workspace surviving in between."""

    @staticmethod
    def forward(ctx, dyn, rows, h, x, *ws):
        w = dict(zip(ops.WEIGHT_KEYS, ws))
        f, it = ops.dyn_eval(h, x, w, dyn, rows_per_image=rows)
        ctx.save_for_backward(h, x, it, *ws)
        ctx.dyn, ctx.rows = dyn, rows
        return f

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise RuntimeError("eval_dot is differentiable once: its backward is a fused kernel with no "
                               "derivative of its own (double backward / create_graph=True is not supported)")
        return _EvalDotFn._vjp(ctx, g)

    @staticmethod
    @once_differentiable
    def _vjp(ctx, g):
        h, x, it, *ws = ctx.saved_tensors
        g_h, grads = ops.dyn_eval_backward(g.contiguous().float(), h, x, dict(zip(ops.WEIGHT_KEYS, ws)), ctx.dyn,
                                           rows_per_image=ctx.rows, exit_iter=it)
        return (None, None, g_h, grads["x_feat"]) + tuple(grads[k] for k in ops.WEIGHT_KEYS)


class LipsLinear(nn.Linear):
    """nn.Linear with a ``singular_u`` buffer (classification.py:25-28)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.register_buffer("singular_u", None)

    def effective_weight(self):
        return self.weight


class OrthoClassDynProjectSimplexLips(nn.Module):
    def __init__(self, n_hidden=10, activation="ReLU", dropout=0.5, mlp_size=128, kappa=5.0, kappa_length=3e4,
                 alpha_1=100.0, alpha_2=5.0, sigma_1=0.02, scale_nominal=False, x_dim=10, cayley=True):
        super().__init__()
        if (n_hidden, mlp_size, x_dim) != (ops.C, ops.M, ops.X):
            raise NotImplementedError(f"libfiode is built for n_hidden=10, mlp_size=128, x_dim=10 "
                                      f"(got {n_hidden}, {mlp_size}, {x_dim})")
        if activation == "ReLU":
            self.activation = nn.ReLU()
        elif activation == "GroupSort":
            # classification.py:44-48 (the reference's config default): no parameters or buffers, so
            # the state_dict keys are the ReLU module's.  Evaluation, ODE solves, certification and,
            # with ops.GROUPSORT_TRAINING on, the Lyapunov training step; with ops.GROUPSORT_TRAIN_ODE
            # on, the rk4 train_ode solve; the dopri5 train_ode solve refuses it (ops.require_relu)
            self.activation = GroupSort()
        else:
            raise NotImplementedError(f"activation {activation!r}: the fused dynamics kernels implement 'ReLU' "
                                      "and, for evaluation, ODE solves and certification, 'GroupSort'")
        self.activation_name = activation
        self.dropout = nn.Dropout(dropout)
        self.mlp_size = mlp_size
        self.n_hidden = n_hidden
        self.kappa = kappa
        self.kappa_length = kappa_length
        self.register_buffer("static_state", None)
        self.alpha_1 = alpha_1
        self.alpha_2 = alpha_2
        self.sigma_1 = sigma_1
        self.qp_max_iter = 30          # FastBarrierProjectionNoUpper(max_iter=30, tol=1e-4), classification.py:63
        self.qp_tol = 1e-4
        self.scale_nominal = scale_nominal
        self.cayley = cayley
        lin = CayleyLinear if cayley else LipsLinear
        self.hidden_to_mlp = lin(n_hidden, mlp_size, bias=True)
        self.mlp_to_mlp = lin(mlp_size, mlp_size)
        self.mlp_to_hidden = lin(mlp_size, n_hidden)
        self.U_x = lin(x_dim, mlp_size)

    # -- parameters as the kernels take them ---------------------------------------------------
    def prefetch(self, stream) -> None:
        """Compute the next effective_weights() on a side stream (joined at the next call)."""
        self._pre = prefetch(stream, self._effective_weights)

    def effective_weights(self) -> Dict[str, torch.Tensor]:
        pre = getattr(self, "_pre", None)
        if pre is not None:
            self._pre = None
            return take(pre)
        return self._effective_weights()

    def _effective_weights(self) -> Dict[str, torch.Tensor]:
        """Q = cayley(alpha W / ||W||) for each layer (differentiable), with the biases.  The three
        128x10-shaped maps (hidden_to_mlp, U_x and the transpose of mlp_to_hidden) run as one
        batched Cayley map (per-matrix norms and alphas); mlp_to_mlp on its own."""
        if self.cayley:
            l1, lx, l3 = self.hidden_to_mlp, self.U_x, self.mlp_to_hidden
            Wb = torch.stack([l1.weight, lx.weight, l3.weight.t()])
            ab = torch.cat([l1.alpha, lx.alpha, l3.alpha])
            Qb = cayley_scaled(Wb, ab, per_matrix=True)
            # Q3 made contiguous here (on the maps' prefetch stream): the solve and the fan-out read
            # it contiguous, and the copy otherwise ran on the step's chain right before the solve
            Q3 = Qb[2].t().contiguous()
            return {"Q1": Qb[0], "b1": l1.bias, "Qx": Qb[1], "bx": lx.bias,
                    "Q2": self.mlp_to_mlp.effective_weight(), "b2": self.mlp_to_mlp.bias,
                    "Q3": Q3, "b3": l3.bias}
        return {"Q1": self.hidden_to_mlp.effective_weight(), "b1": self.hidden_to_mlp.bias,
                "Qx": self.U_x.effective_weight(), "bx": self.U_x.bias,
                "Q2": self.mlp_to_mlp.effective_weight(), "b2": self.mlp_to_mlp.bias,
                "Q3": self.mlp_to_hidden.effective_weight(), "b3": self.mlp_to_hidden.bias}

    def dyn_cfg(self) -> ops.DynCfg:
        return ops.DynCfg(alpha_1=self.alpha_1, alpha_2=self.alpha_2, sigma_1=self.sigma_1,
                          scale_nominal=bool(self.scale_nominal), dropout=float(self.dropout.p),
                          qp_max_iter=self.qp_max_iter, qp_tol=self.qp_tol, activation=self.activation_name)

    # -- reference methods ----------------------------------------------------------------------
    def _h_dot_raw(self, h, x):
        """classification.py:96-102 (used by the optional barrier loss; PyTorch ops on device)."""
        w = self.effective_weights()
        z = F.linear(h, w["Q1"], w["b1"]) + F.linear(x, w["Qx"], w["bx"])
        z = self.activation(self.dropout(z))
        z = self.activation(self.dropout(F.linear(z, w["Q2"], w["b2"])))
        return F.linear(z, w["Q3"], w["b3"])

    def _eval(self, h: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        if self.training and self.dropout.p > 0:
            raise NotImplementedError("training-mode eval_dot (dropout) is fused into LyapunovLearning.compute_loss")
        if torch.is_grad_enabled() and (h.requires_grad or x.requires_grad or
                                        any(p.requires_grad for p in self.parameters())):
            n = h.shape[0]
            rows = n // x.shape[0]
            if rows * x.shape[0] != n:
                raise ValueError("h rows must be a multiple of x rows")
            w = self.effective_weights()
            return _EvalDotFn.apply(self.dyn_cfg(), rows, h.contiguous().float(), x.contiguous().float(),
                                    *[w[k].contiguous().float() for k in ops.WEIGHT_KEYS])
        with torch.no_grad():
            w = {k: v.detach().contiguous().float() for k, v in self.effective_weights().items()}
            n = h.shape[0]
            rows = n // x.shape[0]
            if rows * x.shape[0] != n:
                raise ValueError("h rows must be a multiple of x rows")
            f, _ = ops.dyn_eval(h.contiguous().float(), x.contiguous().float(), w, self.dyn_cfg(), rows_per_image=rows)
        return f

    def eval_dot(self, t, h_tuple, x):
        """classification.py:104-115."""
        return self._eval(h_tuple[0], x)

    def eval_dot_light(self, h, x):
        """classification.py:117-126."""
        return self._eval(h, x)

    def ode_forward(self, t, h_tuple):
        """classification.py:128-132."""
        assert self.static_state is not None, "[ERROR] You forgot to set static state before calling forward."
        return self.eval_dot(t, h_tuple, self.static_state)
