"""fp32 + LSTM (the reference preset at the bench shape): ms per update of the fused csrc/lstm_f32.hip path against
the hybrid autograd path (PATHNET_F32_LSTM=0).  Both trainers live in one process and their timed windows
alternate, each window ending in a device synchronise.  --arms fused runs one arm alone (for a kernel trace).

    python scripts/diag/ab_f32_lstm.py --out profiles/f32_lstm/ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
from pathnet_gym_amd import _build  # noqa: E402

_build.build()
from pathnet_gym_amd.algo.trainer import PathNetTrainer  # noqa: E402
from pathnet_gym_amd.config import preset  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--arms", default="fused,hybrid")
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--updates", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--paths", type=int, default=64)
ap.add_argument("--envs", type=int, default=32)
ap.add_argument("--tmax", type=int, default=20)
ap.add_argument("--out", default="f32_lstm_ab.json")
args = ap.parse_args()


def make(arm):
    os.environ["PATHNET_F32_LSTM"] = "1" if arm == "fused" else "0"
    cfg = preset("reference")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = args.paths, args.envs, args.tmax
    cfg.compute_dtype = "fp32"
    cfg.frame_ring = False
    cfg.use_graph = True
    cfg.ga.backend = "device"
    tr = PathNetTrainer(cfg, device="cuda:0")
    eng = tr.engine
    assert eng.lstm_hip == (arm == "fused") and eng.hybrid == (arm != "fused")
    return tr


arms = args.arms.split(",")
trs = {a: make(a) for a in arms}
info = {a: {"use_graph": bool(t.engine.use_graph), "pipelined": bool(getattr(t, "pipelined", False))}
        for a, t in trs.items()}
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
out = {"config": {"preset": "reference", "dtype": "fp32", "paths": args.paths, "envs_per_path": args.envs,
                  "t_max": args.tmax, "updates_per_window": args.updates, "warmup": args.warmup}, "arms": {}}
for a in arms:
    med = statistics.median(win[a])
    out["arms"][a] = dict(info[a], windows_ms=win[a], median_ms=round(med, 3),
                          spread_pct=round(100 * (max(win[a]) - min(win[a])) / med, 2),
                          finite=bool(torch.isfinite(trs[a].model.store.flat).all()))
if len(arms) == 2:
    out["fused_over_hybrid"] = round(out["arms"]["fused"]["median_ms"] / out["arms"]["hybrid"]["median_ms"], 4)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
