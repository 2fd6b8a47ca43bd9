"""Time of one image's CROWN certification (fiode_certify_crown) on one MI355X -- not a test, not bench.py.

HIP events around one image at T = 40, batches = 400, stop off (every batch runs); the median of
``--runs`` (5) timed runs after ``--warmup`` (1).  Prints one JSON line with the time, the FLOP model
of the bound kernel and the fraction of the f32 matrix peak (157.3 TFLOP/s).

FLOP model per grid row (multiply-accumulates, the useful ones -- the kernel's padded MFMA tiles do
more: DESIGN.md 7e):
    two 128 x 128 x 12 products (layer-2 pre-activation bounds)      393,216
    one  20 x 128 x 128 product (the outputs' coefficient rows)       327,680
    small 128 x 11 products                                            ~30,000
    total ~750,000 MAC = 1.5 MFLOP.

The measurement runs in a child process under its own time limit (``--timeout`` seconds), so a hang ends
with the child and the parent reports it.
"""
import argparse
import json
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
MAC_PER_ROW = 2 * 128 * 128 * 12 + 20 * 128 * 128 + 30_000
PEAK_TFLOPS = 157.3


def child(a):
    sys.path[:0] = [str(ROOT), str(ROOT / "fi-ode_amd")]
    import numpy as np
    import torch
    from fiode_amd import ops
    from tests._util import make_params
    dev = torch.device("cuda:0")
    P = make_params(0)
    w = {k: torch.from_numpy(np.ascontiguousarray(getattr(P, k))).to(dev) for k in ops.WEIGHT_KEYS}
    grid = ops.certify_grid(a.T, device=dev)
    x = torch.from_numpy(np.random.default_rng(1).normal(size=10).astype(np.float32)).to(dev)
    dyn = ops.DynCfg(scale_nominal=bool(a.scale_nominal), dropout=0.0)
    times, out = [], None
    for r in range(a.warmup + a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, it = ops.certify_crown_image(x, a.label, grid, w, dyn, T=a.T, batches=a.batches, stop_on_violation=False)
        e1.record()
        torch.cuda.synchronize(dev)
        if r >= a.warmup:
            times.append(e0.elapsed_time(e1) * 1e-3)
    G = int(grid.shape[0])
    t = float(np.median(times))
    flop = 2.0 * MAC_PER_ROW * G
    o = out.cpu().numpy()
    print(json.dumps({"T": a.T, "batches": a.batches, "rows": G, "seconds_per_image": round(t, 4),
                      "runs": [round(v, 4) for v in times], "mflop_per_row": round(2e-6 * MAC_PER_ROW, 3),
                      "tflop_per_image": round(flop * 1e-12, 2), "tflops": round(flop / t * 1e-12, 2),
                      "fraction_of_f32_peak": round(flop / t * 1e-12 / PEAK_TFLOPS, 3),
                      "max_violation": float(o.max()), "exit_iters_lower_upper": [int(it[:, 0].max()), int(it[:, 1].max())]}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--T", type=int, default=40)
    ap.add_argument("--batches", type=int, default=400)
    ap.add_argument("--label", type=int, default=3)
    ap.add_argument("--scale-nominal", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, str(pathlib.Path(__file__).resolve())] + [v for v in sys.argv[1:]] + ["--child"]
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
        return 124


if __name__ == "__main__":
    sys.exit(main())
