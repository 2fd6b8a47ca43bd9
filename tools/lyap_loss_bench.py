"""The general-loss fused Lyapunov step against the default loss, on one box in one process (not a test).

python tools/lyap_loss_bench.py [--blocks 7] [--calls 200]  ->  one JSON line

``lyap_step_us``: HIP-event time per ``ops.lyap_step`` call (B = 128, S = 256, ReLU dynamics, scale_nominal,
composite sampler, Philox masks) for the default loss (DecisionBoundary, relu, no cap: fiode_lyap_step_act,
k_lyap_bwd<RELU, false>) and for CompositeDynCrossEntropy L2 + elu + cap 1.0 (fiode_lyap_step_loss,
k_lyap_bwd<RELU, true>), alternated in ``blocks`` blocks of ``calls`` back-to-back calls after 20 warm-up
calls each: median and range over the blocks.  The protocol of tools/groupsort_step_bench.py; the yardstick
is the default column of the same run.
"""
import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "fi-ode_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fiode_amd import ops, _lib as L  # noqa: E402
from tests._util import make_params  # noqa: E402

B, S, S1 = 128, 256, 204
LOSSES = {"default": None, "CompositeL2-elu-cap1": ops.LossCfg("CompositeL2", "elu", 1.0)}


def stat(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def lyap_calls(dev):
    P = make_params(seed=7)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, 10, generator=g).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    out = {n: {} for n in LOSSES}
    dyn = ops.DynCfg(scale_nominal=True, dropout=0.5)

    def call(name, offset):
        return ops.lyap_step(x, y, w, dyn, sample_size=S, n_uniform=S1, sampler=L.FIODE_SAMPLER_COMPOSITE,
                             dropout_mode=L.FIODE_DROPOUT_PHILOX, seed=3, offset=offset, out=out[name],
                             loss=LOSSES[name])
    return call


def time_lyap(dev, blocks, calls):
    call = lyap_calls(dev)
    times = {n: [] for n in LOSSES}
    for _ in range(blocks):
        for name in LOSSES:
            for i in range(20):
                call(name, i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(calls):
                call(name, 100 + i)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls * 1e3)
    return {n: stat(v) | {"blocks": [round(t, 2) for t in v]} for n, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    print(json.dumps({"B": B, "S": S, "lyap_step_us": time_lyap(dev, a.blocks, a.calls)}), flush=True)


if __name__ == "__main__":
    main()
