"""CPU checks of the differentiable eval_dot (fiode_dyn_eval_backward, ops.dyn_eval_backward): the
C-ABI boundary, the host-side argument checks, and the reference of the GPU parity tests
(tests/_dyn_grad_ref.py) against finite differences of a float64 eval_dot with the exact projection."""
import ctypes as ct
import pathlib
import re

import numpy as np
import pytest
import torch

from oracle import fiode_oracle as O
from tests import _dyn_grad_ref as G
from tests._util import make_params, make_step_inputs

ROOT = pathlib.Path(__file__).resolve().parents[1]
GPU_TOL = 2e-4          # the gradient tolerance of tests/test_gpu_dyn_backward.py (of the tensor's max)


# ---- the C-ABI ------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_backward():
    from fiode_amd import _lib
    text = (ROOT / "include" / "fiode.h").read_text()
    syms = re.findall(r"FIODE_API\s+[\w\s\*]+?\b(fiode_\w+)\s*\(", text)
    lib = _lib.lib()
    for s in ("fiode_dyn_eval_backward", "fiode_dyn_eval_backward_workspace_bytes"):
        assert s in syms, s
        assert hasattr(lib, s), s
    assert "typedef struct fiode_dyn_eval_debug" in text
    assert lib.fiode_abi_version() == 5 == _lib.ABI_VERSION


def _call(lib, L, *, dyn=None, act=0, batch=4, rows=3, g_f=1, exit_iter=1, g_h=1, grads="full", nbytes=0):
    d = ct.c_void_p(1)
    dyn = dyn or L.DynConfig(10, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)
    w = L.DynWeights(*([d] * 8))
    g = L.LyapGrads(*([d] * 9))
    if grads != "full":
        setattr(g, grads, None)
    p = lambda x: d if x else None
    return lib.fiode_dyn_eval_backward(None, ct.byref(dyn), ct.byref(w), batch, rows, d, d, p(g_f), p(exit_iter),
                                       p(g_h), ct.byref(g), None, d, nbytes, act)


def test_backward_host_argument_checks():
    """Every argument check runs on the host before the workspace-size check, and nothing is launched
    on an error (dummy non-NULL pointers, a zero-byte workspace)."""
    from fiode_amd import _lib as L
    lib = L.lib()
    assert _call(lib, L, act=0) == 3 and _call(lib, L, act=1) == 3         # FIODE_EWORKSPACE
    assert _call(lib, L, act=2) == 1 and _call(lib, L, act=-1) == 1        # FIODE_EINVAL
    assert _call(lib, L, dyn=L.DynConfig(12, 128, 10, 100.0, 20.0, 0.02, 1, 0.5, 30, 1e-4)) == 2
    assert _call(lib, L, g_f=0) == 1
    assert _call(lib, L, exit_iter=0) == 1
    assert _call(lib, L, g_h=0) == 1
    for member in ("Q1", "b2", "x_feat"):
        assert _call(lib, L, grads=member) == 1, member
    assert _call(lib, L, batch=0) == 0
    assert _call(lib, L, rows=0) == 1 and _call(lib, L, rows=-2) == 1
    assert _call(lib, L, batch=-1) == 1
    # the workspace holds a1, a2, gz2, gz1 [N][M] for the weight-gradient chain
    assert lib.fiode_dyn_eval_backward_workspace_bytes(128, 256) >= 4 * 128 * 256 * 128 * 4
    assert lib.fiode_dyn_eval_backward_workspace_bytes(0, 1) == 256


def test_ops_backward_refuses_mismatched_shapes():
    """ops.dyn_eval_backward checks shapes before any library call (host tensors: nothing can launch)."""
    from fiode_amd import ops
    P = make_params(seed=1)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))) for k in ops.WEIGHT_KEYS}
    dyn = ops.DynCfg(dropout=0.0)
    h, x, g = torch.zeros(12, 10), torch.zeros(4, 10), torch.zeros(12, 10)
    with pytest.raises(ValueError, match="g_f"):
        ops.dyn_eval_backward(torch.zeros(11, 10), h, x, w, dyn, rows_per_image=3, exit_iter=0)
    with pytest.raises(ValueError, match="rows_per_image"):
        ops.dyn_eval_backward(g, h, x, w, dyn, rows_per_image=2, exit_iter=0)
    with pytest.raises(ValueError, match="x_feat"):
        ops.dyn_eval_backward(g, h, torch.zeros(4, 9), w, dyn, rows_per_image=3, exit_iter=0)
    with pytest.raises(ValueError, match="h:"):
        ops.dyn_eval_backward(g, torch.zeros(12, 9), x, w, dyn, rows_per_image=3, exit_iter=0)
    with pytest.raises(ValueError, match="exit_iter"):
        ops.dyn_eval_backward(g, h, x, w, dyn, rows_per_image=3)
    with pytest.raises(ValueError, match="activation"):
        ops.dyn_eval_backward(g, h, x, w, ops.DynCfg(dropout=0.0, activation="Tanh"), rows_per_image=3, exit_iter=0)


# ---- the reference helper -------------------------------------------------------------------------
B, S = 16, 64


@pytest.fixture(scope="module")
def case():
    P = make_params(seed=11)
    inp = make_step_inputs(B=B, S=S, seed=12, dropout=False)
    g_f = np.random.default_rng(13).normal(size=(B * S, 10)).astype(np.float32)
    return P, inp, g_f


def test_helper_relu_branch_is_the_oracles_mlp_backward(case):
    P, inp, g_f = case
    cfg = O.DynConfig(scale_nominal=True)
    ref = G.eval_dot_backward(g_f, inp.h, inp.x_feat, S, P, cfg, "ReLU")
    u_rows = np.repeat(O.static_projection(inp.x_feat, P), S, 0)
    mlp = O.mlp_forward(inp.h, u_rows, P, None, None, 0.0)
    own = O.mlp_backward(ref["g_ft"], inp.h, inp.x_feat, S, P, mlp, None, None, 0.0)
    for k in G.KEYS:
        assert np.array_equal(ref[k], own[k]), k
    # and the QP part is the oracle's: f at the batch-global exit
    ev = O.eval_dot(inp.h, u_rows, P, cfg)
    assert ref["K"] == ev.qp.iters and np.array_equal(ref["f"], ev.f)


@pytest.mark.parametrize("activation", ["ReLU", "GroupSort"])
@pytest.mark.parametrize("scale_nominal", [True, False])
def test_helper_matches_finite_differences(case, activation, scale_nominal):
    """g_h and a directional derivative in u (the per-row layer-1 offset U_x x + bx) of the helper
    against central differences (step 1e-6) of f64_eval_dot, whose projection is exact.  Rows within
    1e-4 of a kink (a ReLU unit's zero / a GroupSort pair's tie, or a change of the QP's active set)
    are left out: at most 15 % of them.  Kept rows agree to 1e-6 of max |g_h|.

    The helper runs with ``bound_active`` (its docstring): with the reference's own active-set test,
    rounding noise for coordinates off their bound, 381 / 292 of the ~930 / ~990 kept rows (ReLU /
    GroupSort, scale_nominal False) differ from the exact projection's gradient by O(1) -- the stated
    deviation of DESIGN.md "Parity", not a property of the formulas checked here.
    Measured: 9.1 / 9.4 % (ReLU) and 3.2 / 3.6 % (GroupSort) of the rows left out for scale_nominal
    True / False; largest error on the kept rows 8.2e-8 of max |g_h|."""
    P, inp, g_f = case
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    ref = G.eval_dot_backward(g_f, inp.h, inp.x_feat, S, P, cfg, activation, bound_active=True)
    u_rows = np.repeat(O.static_projection(inp.x_feat, P), S, 0).astype(np.float64)
    h64 = inp.h.astype(np.float64)
    _, qp_margin = G.f64_eval_dot(h64, u_rows, P, cfg, activation)
    keep = (ref["margin"] >= 1e-4) & (qp_margin >= 1e-4)
    left_out = 1.0 - keep.mean()
    d = 1e-6
    fd = np.zeros_like(h64)
    for j in range(10):
        e = np.zeros(10)
        e[j] = d
        fp, _ = G.f64_eval_dot(h64 + e, u_rows, P, cfg, activation)
        fm, _ = G.f64_eval_dot(h64 - e, u_rows, P, cfg, activation)
        fd[:, j] = ((fp - fm) * g_f).sum(1) / (2 * d)
    D = np.random.default_rng(14).normal(size=u_rows.shape) / np.sqrt(u_rows.shape[1])
    fp, _ = G.f64_eval_dot(h64, u_rows + d * D, P, cfg, activation)
    fm, _ = G.f64_eval_dot(h64, u_rows - d * D, P, cfg, activation)
    fd_u = ((fp - fm) * g_f).sum(1) / (2 * d)
    scale = float(np.abs(ref["g_h"]).max())
    err_h = float(np.abs(fd - ref["g_h"])[keep].max())
    err_u = float(np.abs(fd_u - (ref["g_z1"] * D).sum(1))[keep].max())
    print(f"{activation} scale_nominal={scale_nominal}: left out {left_out:.3f}, g_h err {err_h / scale:.2e}, "
          f"u err {err_u / scale:.2e} of max|g_h| {scale:.3f}")
    assert left_out <= 0.15, left_out
    assert err_h <= 1e-6 * scale, (err_h, scale)
    assert err_u <= 1e-6 * scale, (err_u, scale)


@pytest.mark.parametrize("scale_nominal", [True, False])
def test_groupsort_and_relu_references_differ(case, scale_nominal):
    """A kernel applying the wrong activation's backward cannot pass the GPU parity test: the two
    references differ by more than 100 x its tolerance in every gradient array."""
    P, inp, g_f = case
    cfg = O.DynConfig(scale_nominal=scale_nominal)
    a = G.eval_dot_backward(g_f, inp.h, inp.x_feat, S, P, cfg, "ReLU")
    b = G.eval_dot_backward(g_f, inp.h, inp.x_feat, S, P, cfg, "GroupSort")
    for k in G.KEYS + ("g_h",):
        diff = float(np.abs(a[k] - b[k]).max())
        assert diff > 100 * GPU_TOL * float(np.abs(b[k]).max()), (k, diff)


def test_groupsort_backward_splits_ties():
    z = np.array([[1.0, 2.0, 3.0, 1.0, 5.0, 0.0]])
    g = np.array([[10.0, 20.0, 30.0, 1.0, 2.0, 3.0]])          # d/d max | d/d min
    # pairs (1, 1) tie, (2, 5) second larger, (3, 0) first larger
    assert np.array_equal(G.groupsort_backward(g, z), [[5.5, 2.0, 30.0, 5.5, 20.0, 3.0]])
