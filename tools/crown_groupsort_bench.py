"""GroupSort against ReLU: time of one image's CROWN certification on one MI355X -- not a test, not bench.py.

Two measurements, each in a child process under its own time limit (``--timeout`` seconds):

  default     HIP events around one image at T = 40, batches = 400, stop off (every batch runs), the two
              activations alternated (ReLU, GroupSort, ReLU, ...): per activation the median of ``--runs``
              (3) timed runs after ``--warmup`` (1).  One JSON line.
  --profile   the same child (one run per activation, no warm-up) under ``rocprofv3 --kernel-trace --stats``,
              in a run of its own: the total time of every k_crown_* kernel over one image, from the kernel
              trace.  k_crown_bounds is the ReLU bound kernel, k_crown_bounds_gs the GroupSort one (with
              k_crown_fold_gs, once per image); the QP kernels serve both.  One JSON line.

MFMA issued per two grid rows: ReLU 512 + 2 x 320 = 1,152; GroupSort 128 + 2 x (96 + 32) = 384.
"""
import argparse
import csv
import json
import pathlib
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[1]
ACTS = ("ReLU", "GroupSort")


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
    times = {k: [] for k in ACTS}
    res = {}
    with ops.groupsort_crown():
        for r in range(a.warmup + a.runs):
            for act in ACTS:
                dyn = ops.DynCfg(scale_nominal=bool(a.scale_nominal), dropout=0.0, activation=act)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out, it = ops.certify_crown_image(x, a.label, grid, w, dyn, T=a.T, batches=a.batches,
                                                  stop_on_violation=False)
                e1.record()
                torch.cuda.synchronize(dev)
                if r >= a.warmup:
                    times[act].append(e0.elapsed_time(e1) * 1e-3)
                res[act] = (float(out.max()), [int(it[:, 0].max()), int(it[:, 1].max())])
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"T": a.T, "batches": a.batches, "rows": int(grid.shape[0]),
                      "seconds_per_image": {k: round(v, 4) for k, v in med.items()},
                      "runs": {k: [round(t, 4) for t in v] for k, v in times.items()},
                      "groupsort_over_relu": round(med["GroupSort"] / med["ReLU"], 3),
                      "max_violation": {k: v[0] for k, v in res.items()},
                      "exit_iters_lower_upper": {k: v[1] for k, v in res.items()}}), flush=True)


def kernel_totals(outdir: pathlib.Path):
    """{kernel: [calls, total ms]} of the k_crown_* kernels from rocprofv3's kernel-trace CSV."""
    tot = {}
    for f in sorted(outdir.rglob("*kernel_trace*.csv")):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name") or row.get("Name") or ""
                if "k_crown_" not in name:
                    continue
                short = name[name.index("k_crown_"):].split("(")[0].split("E")[0] if name.startswith("_Z") else \
                    name[name.index("k_crown_"):].split("(")[0]
                dt = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
                c = tot.setdefault(short, [0, 0.0])
                c[0] += 1
                c[1] += dt
    return {k: [v[0], round(v[1], 3)] for k, v in sorted(tot.items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--T", type=int, default=40)
    ap.add_argument("--batches", type=int, default=400)
    ap.add_argument("--label", type=int, default=3)
    ap.add_argument("--scale-nominal", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=float, default=240.0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-dir", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    me = str(pathlib.Path(__file__).resolve())
    keep = [v for v in sys.argv[1:] if v != "--profile"]
    try:
        if not a.profile:
            return subprocess.run([sys.executable, me] + keep + ["--child"], timeout=a.timeout).returncode
        outdir = pathlib.Path(a.profile_dir or tempfile.mkdtemp(prefix="crown_gs_prof_"))
        outdir.mkdir(parents=True, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(outdir), "-o", "crown_gs",
               "--", sys.executable, me] + keep + ["--child", "--runs", "1", "--warmup", "0"]
        p = subprocess.run(cmd, timeout=a.timeout, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            print(p.stdout[-2000:])
            return p.returncode
        print(json.dumps({"T": a.T, "batches": a.batches, "kernel_calls_and_total_ms_per_image": kernel_totals(outdir),
                          "trace_dir": str(outdir)}), flush=True)
        return 0
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"no result within {a.timeout} s"}), flush=True)
        return 124


if __name__ == "__main__":
    sys.exit(main())
