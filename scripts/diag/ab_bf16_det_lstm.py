"""bf16 + deterministic + LSTM (the reference preset at the bench shape): ms per update of the fused csrc/lstm.hip
path with the ordered weight gradient against the hybrid autograd path (PATHNET_BF16_DET_LSTM=0), and, for context,
of the atomic fused bf16 path (deterministic=False).  The trainers live in one process and their timed windows
alternate, each window ending in a device synchronise.

Without --child this is a driver that never opens the GPU itself: it starts the measuring process under
`timeout -k 10 <--limit seconds>`, stops at the first step that fails, and writes the result and a two-line README
next to it.  --arms fused runs one arm alone (for a kernel trace).

    python scripts/diag/ab_bf16_det_lstm.py --out profiles/bf16_det_lstm/ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--arms", default="fused,hybrid,atomic")
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--updates", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--paths", type=int, default=64)
ap.add_argument("--envs", type=int, default=32)
ap.add_argument("--tmax", type=int, default=20)
ap.add_argument("--limit", type=int, default=420, help="seconds the measuring process may take")
ap.add_argument("--out", default="profiles/bf16_det_lstm/ab.json")
ap.add_argument("--child", action="store_true", help="measure in this process (the driver starts it)")
args = ap.parse_args()

README = """# bf16 + deterministic + LSTM: fused `csrc/lstm.hip` (ordered weight gradient) against the hybrid autograd path

`ab.json`: `scripts/diag/ab_bf16_det_lstm.py`, `preset("reference")`, bf16, `deterministic=True`, {paths} paths x {envs} envs, T = {tmax}, one MI355X; ms per update of the arms, {windows} alternated windows of {updates} updates each (`docs/PERF.md`, "bf16 + deterministic + LSTM"). `kernel_stats.md`, `kernel_stats.csv`: rocprofv3 `--kernel-trace --stats` of the fused arm alone (`--child --arms fused`, 5 warm-up + 10 timed updates), summarised by `scripts/prof_summary.py`.
"""


def driver():
    from pathnet_gym_amd import _build
    _build.build()
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child"]
    for k in ("arms", "windows", "updates", "warmup", "paths", "envs", "tmax"):
        cmd += [f"--{k}", str(getattr(args, k))]
    cmd += ["--out", out]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        sys.exit(f"measuring process ended with status {rc}; nothing further is started")
    with open(os.path.join(os.path.dirname(out), "README.md"), "w") as f:
        f.write(README.format(paths=args.paths, envs=args.envs, tmax=args.tmax, windows=args.windows,
                              updates=args.updates))


def child():
    import torch
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.config import preset

    def make(arm):
        os.environ["PATHNET_BF16_DET_LSTM"] = "0" if arm == "hybrid" else "1"
        cfg = preset("reference")
        cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = args.paths, args.envs, args.tmax
        cfg.compute_dtype = "bf16"
        cfg.deterministic = arm != "atomic"
        cfg.frame_ring = False
        cfg.use_graph = True
        cfg.ga.backend = "device"
        tr = PathNetTrainer(cfg, device="cuda:0")
        eng = tr.engine
        assert eng.lstm_hip == (arm != "hybrid") and eng.hybrid == (arm == "hybrid")
        assert tr.model.hip.deterministic == (arm != "atomic")
        return tr

    arms = args.arms.split(",")
    trs = {a: make(a) for a in arms}
    info = {a: {"use_graph": bool(t.engine.use_graph), "pipelined": bool(getattr(t, "pipelined", False)),
                "deterministic": bool(t.model.hip.deterministic)} for a, t in trs.items()}
    for a, tr in trs.items():
        for _ in range(args.warmup):
            tr.update()
        tr.flush()
        torch.cuda.synchronize()
        print("warm", a, info[a], flush=True)
    win = {a: [] for a in arms}
    for w in range(args.windows):
        for a in arms:
            tr = trs[a]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.updates):
                tr.update()
            tr.flush()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.updates
            win[a].append(round(ms, 3))
            print("window", w, a, f"{ms:.3f} ms/update", flush=True)
    out = {"config": {"preset": "reference", "dtype": "bf16", "paths": args.paths, "envs_per_path": args.envs,
                      "t_max": args.tmax, "updates_per_window": args.updates, "warmup": args.warmup}, "arms": {}}
    for a in arms:
        med = statistics.median(win[a])
        out["arms"][a] = dict(info[a], windows_ms=win[a], median_ms=round(med, 3),
                              spread_pct=round(100 * (max(win[a]) - min(win[a])) / med, 2),
                              finite=bool(torch.isfinite(trs[a].model.store.flat).all()))
    if "fused" in arms and "hybrid" in arms:
        out["fused_over_hybrid"] = round(out["arms"]["fused"]["median_ms"] / out["arms"]["hybrid"]["median_ms"], 4)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    child() if args.child else driver()
