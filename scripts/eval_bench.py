"""Time the evaluation paths on one GPU: the torch backend (today's default) against the forward-only HIP engine.

  A. evaluate_path on Pong with the ``pong`` preset net: 64 episodes, one fixed randomly initialised path,
     max_steps 3000 -- backend torch on the GPU (the solve criterion's held-out confirmation as it runs today), hip in
     bf16 and in fp32x;
  B. evaluate_checkpoint of a 64-path Pong checkpoint: torch on the CPU (today's ``cli eval``) for --cpu_steps steps
     against hip for --ckpt_steps steps (both 2000 in the committed record; a smaller --cpu_steps shortens a rehearsal,
     the per-step times are reported next to the totals).

Every timed call ends in host reads of device results, so the wall clock covers the GPU work.  The backends are
alternated, --runs times each, after one short warm-up call per backend (it loads the code objects).  Every
evaluate_* call builds its own evaluator, so a timed hip call includes the construction, the weights' copy, the
eager first chunk and the graph capture.  The device's current shader and memory clocks are read (read-only, from
sysfs) before and after each part.  Writes one JSON file per part into --out.

    python scripts/eval_bench.py --out profiles/eval
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def device_clocks():
    """Current sclk / mclk level of every amdgpu card as sysfs reports it (the starred line of pp_dpm_*), read-only;
    {} where the files are not readable."""
    import glob
    out = {}
    for kind in ("sclk", "mclk"):
        for f in sorted(glob.glob(f"/sys/class/drm/card*/device/pp_dpm_{kind}")):
            try:
                with open(f) as fh:
                    cur = [ln.strip() for ln in fh if "*" in ln]
            except OSError:
                continue
            out.setdefault(kind, {})[f.split("/")[4]] = cur[0] if cur else None
    return out


def summary(xs):
    return {"median_s": round(statistics.median(xs), 4), "min_s": round(min(xs), 4), "max_s": round(max(xs), 4),
            "runs_s": [round(x, 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/eval")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--path_steps", type=int, default=3000)
    ap.add_argument("--ckpt_steps", type=int, default=2000)
    ap.add_argument("--cpu_steps", type=int, default=2000)
    ap.add_argument("--parts", default="A,B")
    args = ap.parse_args()
    import tempfile
    import numpy as np
    import torch
    from pathnet_gym_amd import _build
    from pathnet_gym_amd.algo import evaluate
    from pathnet_gym_amd.algo.ga import get_geopath
    from pathnet_gym_amd.config import preset
    from pathnet_gym_amd.models.pathnet import ParamStore
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU: a CPU timing says nothing about the engine")
    _build.build()
    os.makedirs(args.out, exist_ok=True)
    meta = {"gpu": torch.cuda.get_device_name(0), "torch": torch.__version__, "build": _build.build_info(),
            "argv": sys.argv[1:]}
    cfg = preset("pong")
    net = cfg.net

    if "A" in args.parts.split(","):
        flat = ParamStore(net, "cuda", seed=3).flat.detach()
        path = get_geopath(net.L, net.M, net.N, np.random.RandomState(5)).astype(np.float32)
        kw = dict(episodes=args.episodes, seed=424242, device="cuda", max_steps=args.path_steps)
        arms = {"torch": dict(backend="torch"), "hip_bf16": dict(backend="hip", compute_dtype="bf16"),
                "hip_fp32x": dict(backend="hip", compute_dtype="fp32x")}
        clk0 = device_clocks()
        for name, a in arms.items():          # warm-up: a short call of the same batch shape
            evaluate.evaluate_path(net, flat, path, "Pong", **dict(kw, max_steps=40), **a)
        times = {k: [] for k in arms}
        res = {}
        for _ in range(args.runs):
            for name, a in arms.items():
                dt, r = timed(lambda: evaluate.evaluate_path(net, flat, path, "Pong", **kw, **a))
                times[name].append(dt)
                res[name] = {k: r[k] for k in ("mean", "finished", "steps", "backend", "compute_dtype")}
                print(json.dumps({"part": "A", "arm": name, "seconds": round(dt, 4), **res[name]}), flush=True)
        out = {"part": "evaluate_path Pong, pong preset net, one random-init path", "episodes": args.episodes,
               "max_steps": args.path_steps, "arms": {k: dict(summary(v), **res[k]) for k, v in times.items()},
               "clocks_before": clk0, "clocks_after": device_clocks(), **meta}
        with open(os.path.join(args.out, "evaluate_path_pong.json"), "w") as f:
            json.dump(out, f, indent=1)

    if "B" in args.parts.split(","):
        from pathnet_gym_amd.algo.trainer import PathNetTrainer
        from pathnet_gym_amd.utils import checkpoint as ckpt
        c = preset("pong")
        c.paths, c.envs_per_path, c.a2c.t_max, c.backend, c.gc_freeze = 64, 16, 5, "hip", False
        tr = PathNetTrainer(c, device="cuda:0")
        tmp = tempfile.mkdtemp(prefix="eval_bench_")
        p = os.path.join(tmp, "pong64.safetensors")
        ckpt.save(tr, p)
        del tr
        hip = dict(backend="hip", compute_dtype="fp32x", device="cuda")
        clk0 = device_clocks()
        # warm-up; no Pong episode ends within 40 steps, and evaluate_checkpoint raises on an all-NaN result
        try:
            evaluate.evaluate_checkpoint(c, p, max_steps=40, **hip)
        except ValueError:
            pass
        times = {"hip_fp32x": [], "torch_cpu": []}
        res = {}
        for _ in range(args.runs):
            dt, r = timed(lambda: evaluate.evaluate_checkpoint(c, p, max_steps=args.ckpt_steps, **hip))
            times["hip_fp32x"].append(dt)
            res["hip_fp32x"] = {"steps": r["steps"], "finished_paths": int(np.isfinite(r["returns"]).sum())}
            print(json.dumps({"part": "B", "arm": "hip_fp32x", "seconds": round(dt, 4), **res["hip_fp32x"]}), flush=True)
            dt, r = timed(lambda: evaluate.evaluate_checkpoint(c, p, max_steps=args.cpu_steps, device="cpu"))
            times["torch_cpu"].append(dt)
            res["torch_cpu"] = {"steps": r["steps"]}
            print(json.dumps({"part": "B", "arm": "torch_cpu", "seconds": round(dt, 4), "steps": r["steps"]}), flush=True)
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
        arms = {k: dict(summary(v), **res[k]) for k, v in times.items()}
        for k, a in arms.items():
            a["seconds_per_step"] = round(a["median_s"] / max(1, a["steps"]), 6)
        out = {"part": "evaluate_checkpoint, 64 Pong paths", "hip_max_steps": args.ckpt_steps,
               "cpu_max_steps": args.cpu_steps, "cpu_threads": torch.get_num_threads(), "arms": arms,
               "clocks_before": clk0, "clocks_after": device_clocks(), **meta}
        with open(os.path.join(args.out, "evaluate_checkpoint_pong64.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
