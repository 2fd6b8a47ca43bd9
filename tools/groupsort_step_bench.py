"""GroupSort against ReLU in the fused Lyapunov training step, on one box in one process (not a test).

python tools/groupsort_step_bench.py [--blocks 7] [--calls 200] [--no-graph]  ->  one JSON line

* ``lyap_step_us``: HIP-event time per ``ops.lyap_step`` call (B = 128, S = 256, scale_nominal, composite
  sampler, Philox masks), the two activations alternated in ``blocks`` blocks of ``calls`` back-to-back
  calls after 20 warm-up calls each: median and range over the blocks.
* ``graph_step_ms``: the captured Lyapunov-only training step (bench.build_module, train_ode False) of
  a ReLU and a GroupSort module, replayed round-robin as tools/ab_step.py does.
* ``--profile N``: only N calls of each activation and nothing else, for a
  ``rocprofv3 --kernel-trace --stats -- python tools/groupsort_step_bench.py --profile 50`` run of its
  own (kernel times of k_lyap_fwd / k_lyap_bwd per instantiation).

The yardstick is the ReLU column of the same run.
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "fi-ode_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fiode_amd import ops, _lib as L  # noqa: E402
from tests._util import make_params  # noqa: E402

B, S, S1 = 128, 256, 204
ACTS = ("ReLU", "GroupSort")


def stat(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def lyap_calls(dev):
    P = make_params(seed=7)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, 10, generator=g).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    out = {a: {} for a in ACTS}

    def call(act, offset):
        return ops.lyap_step(x, y, w, ops.DynCfg(scale_nominal=True, dropout=0.5, activation=act), sample_size=S,
                             n_uniform=S1, sampler=L.FIODE_SAMPLER_COMPOSITE, dropout_mode=L.FIODE_DROPOUT_PHILOX,
                             seed=3, offset=offset, out=out[act])
    return call


def time_lyap(dev, blocks, calls):
    call = lyap_calls(dev)
    times = {a: [] for a in ACTS}
    for blk in range(blocks):
        for act in ACTS:
            for i in range(20):
                call(act, i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(calls):
                call(act, 100 + i)
            e1.record()
            torch.cuda.synchronize()
            times[act].append(e0.elapsed_time(e1) / calls * 1e3)
    return {a: stat(v) | {"blocks": [round(t, 2) for t in v]} for a, v in times.items()}


def time_graph(dev, rounds=6):
    import bench
    from fiode_amd.cayley import GroupSort
    from fiode_amd.graph_step import GraphTrainStep
    steps = {}
    for act in ACTS:
        mod = bench.build_module(dev, train_ode=False)
        if act == "GroupSort":
            mod.dyn_fun.activation, mod.dyn_fun.activation_name = GroupSort(), "GroupSort"
        opt = mod.configure_optimizers(capturable=True)[0][0]
        g = torch.Generator(device="cpu").manual_seed(1234)
        x = torch.rand(B, 3, 32, 32, generator=g).to(dev)
        y = torch.randint(0, 10, (B,), generator=g).to(dev)
        steps[act] = GraphTrainStep(mod, opt, x, y)
    times = {a: [] for a in ACTS}
    for _ in range(rounds):
        for act, gs in steps.items():
            for _ in range(3):
                gs.step()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(20):
                gs.step()
            torch.cuda.synchronize()
            times[act].append((time.perf_counter() - t) / 20 * 1e3)
    return {a: {"median": round(statistics.median(v), 4), "all": [round(t, 4) for t in v]} for a, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--profile", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with ops.groupsort_training():
        if a.profile:
            call = lyap_calls(dev)
            for act in ACTS:
                for i in range(a.profile):
                    call(act, i)
            torch.cuda.synchronize()
            return
        res = {"B": B, "S": S, "lyap_step_us": time_lyap(dev, a.blocks, a.calls)}
        if not a.no_graph:
            res["graph_step_ms"] = time_graph(dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
