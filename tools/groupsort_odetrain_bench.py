"""GroupSort against ReLU in the rk4 train_ode solve, on one box in one process (not a test).

python tools/groupsort_odetrain_bench.py [--blocks 5] [--calls 50] [--batch 128] [--step 0.1]  ->  one JSON line

HIP-event time per call of ``ops.odetrain_forward`` (k_ot_masks + the forward kernel) and of
``ops.odetrain_backward_x`` (the sweep kernel + k_ot_gx) at scale_nominal, Philox masks, for three
variants alternated in ``blocks`` blocks of ``calls`` back-to-back calls after 10 warm-up calls each
(median and range over the blocks):

* ``relu4``:       ReLU as launched by default at this batch (k_ot_fwd4 / k_ot_bwd4 up to B = 1024);
* ``relu16``:      ReLU on the 16-row kernels (k_ot_fwd<RELU> / k_ot_bwd<SN, RELU>), through the
                   library's measuring hook FIODE_DEBUG_OT_TILE16;
* ``groupsort16``: GroupSort (k_ot_fwd<GROUPSORT> / k_ot_bwd<SN, GROUPSORT>, 16-row for every batch).

The yardsticks are the ReLU columns of the same run: relu16 - groupsort16 is what the activation
costs, relu4 - relu16 what a 4-row port of the GroupSort kernels would buy.
"""
import argparse
import json
import os
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "fi-ode_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fiode_amd import ops, _lib as L  # noqa: E402
from tests._util import make_params  # noqa: E402

VARIANTS = (("relu4", "ReLU", ""), ("relu16", "ReLU", "1"), ("groupsort16", "GroupSort", ""))


def stat(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--step", type=float, default=0.1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B = a.batch
    P = make_params(seed=7)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, 10, generator=g).to(dev)
    h0 = torch.full((B, 10), 0.1, device=dev)
    gy = torch.randn(B, 10, generator=g).to(dev)
    fwd = {v[0]: [] for v in VARIANTS}
    bwd = {v[0]: [] for v in VARIANTS}
    with ops.groupsort_train_ode():
        for blk in range(a.blocks):
            for name, act, env in VARIANTS:
                os.environ["FIODE_DEBUG_OT_TILE16"] = env
                dyn = ops.DynCfg(scale_nominal=True, dropout=0.5, activation=act)
                state = {}

                def forward(i):
                    cfg = ops.odetrain_config(B, 0.0, 1.0, a.step, L.FIODE_DROPOUT_PHILOX, seed=3, offset=i)
                    state["cfg"], state["ws"] = cfg, ops.odetrain_forward(x, h0, w, dyn, cfg)[2]

                def sweep(i):
                    ops.odetrain_backward_x(gy, x, w, dyn, state["cfg"], state["ws"])
                for i in range(10):
                    forward(i)
                fwd[name].append(timed(forward, a.calls))
                for i in range(10):
                    sweep(i)
                bwd[name].append(timed(sweep, a.calls))
    os.environ["FIODE_DEBUG_OT_TILE16"] = ""
    res = {"B": B, "step": a.step, "evals": ops.odetrain_evals(state["cfg"]),
           "forward_us": {k: stat(v) | {"blocks": [round(t, 1) for t in v]} for k, v in fwd.items()},
           "backward_x_us": {k: stat(v) | {"blocks": [round(t, 1) for t in v]} for k, v in bwd.items()}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
