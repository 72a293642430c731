"""Evaluation: greedy rollouts of the population / frozen path of a checkpoint.

The reference has a display path (``run_policy``, ``game_ac_network.py:458-465``,
and ``GameState(display=True)`` with a gym Monitor).  Here evaluation runs the
whole population on device, one env per path, argmax actions, until each path
finished ``episodes`` episodes or ``max_steps`` steps.

Backends: ``"torch"`` (the default) is the PyTorch oracle forward stepped from Python, on any device; ``"hip"`` runs the
forward-only HIP engine (``runtime/evaluator.py``): the training kernels at ``compute_dtype``, the env in its HIP
kernel, finished episodes accounted on the device by the episode ledger (``ledger_ref`` below is its rule);
``"auto"`` picks ``"hip"`` when a GPU is visible and the net and env are inside that engine's envelope.
"""
from __future__ import annotations

import numpy as np
import torch

from ..envs.control import obs_dim_kwargs
from ..envs.registry import make
from ..models.acnet import ACPathNet
from .ga import express


BACKENDS = ("torch", "hip", "auto")
HIP_CHUNK = 20          # steps per chunk of the hip backend (the engine's default rollout length)


def ledger_ref(dones, epret, nvalid: int, quota: int, max_steps: int, cnt, ret, endstep, clock: int):
    """The episode ledger's rule (csrc/heads.hip eval_ledger_kernel) in plain numpy, in place on cnt [B] / ret
    [B, quota] / endstep [B, quota].  dones / epret: one chunk [T, B]; ``clock``: steps played before it.  Entry
    (t, b) counts iff b < nvalid, dones[t, b], cnt[b] < quota and clock + t < max_steps; counted entries are taken
    in increasing t, each writes ret[b, cnt[b]] = epret[t, b] and endstep[b, cnt[b]] = clock + t + 1, then
    cnt[b] += 1.  -> (clock + T, pending = number of b < nvalid with cnt[b] < quota)."""
    dones = np.asarray(dones)
    epret = np.asarray(epret)
    T, B = dones.shape
    if not 0 <= nvalid <= B:
        raise ValueError(f"nvalid={nvalid} outside [0, {B}]")
    for b in range(nvalid):
        for t in range(T):
            if cnt[b] >= quota or clock + t >= max_steps:
                break
            if dones[t, b]:
                ret[b, cnt[b]] = epret[t, b]
                endstep[b, cnt[b]] = clock + t + 1
                cnt[b] += 1
    return clock + T, int(sum(1 for b in range(nvalid) if cnt[b] < quota))


def resolve_eval_backend(backend: str, net_cfg, env_id: str, compute_dtype=None) -> str:
    """"torch" | "hip" from the ``backend`` argument of the evaluate_* functions.  "hip" without a GPU raises
    RuntimeError (a net or env outside the evaluator's envelope raises NotImplementedError when it is built);
    "auto" falls back to "torch" in both cases."""
    if backend not in BACKENDS:
        raise ValueError(f"backend {backend!r}: expected one of {BACKENDS}")
    if backend == "torch":
        return "torch"
    gpu = torch.cuda.is_available()
    if backend == "hip":
        if not gpu:
            raise RuntimeError("evaluation backend 'hip' needs a GPU")
        return "hip"
    if not gpu:
        return "torch"
    from ..runtime.evaluator import min_envs_per_path, unsupported_reason
    why = unsupported_reason(net_cfg, env_id, compute_dtype, min_envs_per_path(net_cfg))
    return "torch" if why is not None else "hip"


def _hip_device(device):
    """The GPU a hip evaluation runs on: ``device`` when it names one, else the current one."""
    d = torch.device(device)
    return d if d.type == "cuda" else torch.device("cuda")


def _evaluate_model_hip(model: ACPathNet, env_id, episodes, max_steps, device, seed, frameskip, gray, sample,
                        compute_dtype, info):
    from ..runtime.evaluator import HipEvaluator, min_envs_per_path
    # one env per path, quota = episodes.  A conv trunk wants E * Ho * Wo in multiples of 16 (E = 16 on the reference
    # trunk): there every path's row is padded to E envs, all of them step, and only the row's first env (b = p * E)
    # is waited for and read, so ``episodes`` means what it means on the torch backend
    P, E = model.P, min_envs_per_path(model.cfg)
    quota = int(episodes)
    ev = HipEvaluator(model.cfg, env_id, P, E, chunk=HIP_CHUNK, device=_hip_device(device),
                      compute_dtype=compute_dtype, env_seed=seed, frameskip=frameskip, gray=gray)
    try:
        ev.load(model.store.flat, model.mask.cpu().numpy(), model.task)
        rets = ev.run(quota=quota, max_steps=max_steps, sample=sample, seed=seed, env_stride=E)
        info.update(backend="hip", compute_dtype=ev.compute_dtype, steps=ev.last["steps"])
    finally:
        ev.close()
    assert len(rets) == P
    return [float(np.mean(x)) if x else float("nan") for x in rets]


@torch.no_grad()
def evaluate_model(model: ACPathNet, env_id: str, episodes: int = 1, max_steps: int = 2000, device="cpu",
                   seed: int = 12345, frameskip: int = 4, gray: str = "rgb", sample: bool = False,
                   backend: str = "torch", compute_dtype=None, info=None):
    """Mean return per path over ``episodes`` episodes (NaN for a path that finished none in ``max_steps``).
    ``sample=False`` plays the argmax action; ``sample=True`` samples the policy with a seeded generator,
    so a repeated evaluation of unchanged parameters replays the same episodes.

    ``backend="hip"`` (module docstring) counts exactly the FIRST ``episodes`` episodes of each path's env; the torch
    loop keeps appending a fast path's later episodes until the slowest path is done, so its means can cover more.
    (Where the trunk has conv layers the kernels take envs per path in multiples of 16: the path's row is padded with
    envs that step but are neither waited for nor read.)
    ``info``: a dict that receives ``backend``, ``compute_dtype`` and ``steps`` (env steps played per path)."""
    meta = {} if info is None else info          # (the loop below has an ``info`` of its own: the env's)
    if resolve_eval_backend(backend, model.cfg, env_id, compute_dtype) == "hip":
        return _evaluate_model_hip(model, env_id, episodes, max_steps, device, seed, frameskip, gray, sample,
                                   compute_dtype, meta)
    P = model.P
    gen = torch.Generator(device=device).manual_seed(seed) if sample else None
    kw = {} if env_id.startswith("CartPole") else dict(frameskip=frameskip, gray=gray)
    kw.update(obs_dim_kwargs(env_id, model.cfg.input_shape))
    env = make(env_id, num_envs=P, device=device, seed=seed, backend="torch", **kw)
    obs = env.reset()
    state = model.init_state(P)
    returns = [[] for _ in range(P)]
    meta.update(backend="torch", compute_dtype="fp32", steps=0)
    for step in range(max_steps):
        meta["steps"] = step + 1
        logits, value, state = model.forward(obs, 1, state)
        if sample:
            a = torch.multinomial(torch.softmax(logits.float(), -1), 1, generator=gen).reshape(-1)
        else:
            a = logits.argmax(-1)
        obs, r, d, info = env.step(a)
        if state is not None:
            keep = (~d).float()[:, None]
            state = (state[0] * keep, state[1] * keep)
        for p in np.nonzero(d.cpu().numpy())[0]:
            returns[p].append(float(info["episode_return"][p]))
        if all(len(x) >= episodes for x in returns):
            break
    return [float(np.mean(x)) if x else float("nan") for x in returns]


def evaluate_checkpoint(cfg, path: str, episodes: int = 1, max_steps: int = 2000, device="cpu",
                        backend: str = "torch", compute_dtype=None, sample: bool = False, seed: int = 12345):
    """Evaluate every path of a checkpoint's population, one env per path (``cli eval``).  ``device`` places the torch
    backend's model and envs; the hip backend (evaluate_model) runs on it when it is a GPU, else on the current GPU."""
    from safetensors.torch import load_file
    d = load_file(path)
    g = d["ga.genotypes"].numpy().astype(np.float32)
    fr = d["ga.frozen"].numpy().astype(np.float32)
    P = g.shape[0]
    model = ACPathNet(cfg.net, P, device, "torch")
    st = model.store
    with torch.no_grad():
        for s in st.layout.segments:
            st.flat[s.offset:s.offset + s.numel].copy_(d[s.name].reshape(-1))
    model.set_paths(express(g, fr[None], getattr(cfg.ga, "frozen_mode", "or")))
    task = int(d["train.task_idx"][0])
    model.task = task
    env_id = cfg.tasks[min(task, len(cfg.tasks) - 1)]
    info = {}
    rets = evaluate_model(model, env_id, episodes, max_steps, device, seed=seed, frameskip=cfg.frameskip,
                          gray=cfg.gray, sample=sample, backend=backend, compute_dtype=compute_dtype, info=info)
    return {"env": env_id, "task": task, "returns": rets, "best_path": int(np.nanargmax(rets)) if rets else -1,
            "best_return": float(np.nanmax(rets)) if rets else float("nan"), **info}


@torch.no_grad()
def evaluate_path(net_cfg, flat: torch.Tensor, expressed: np.ndarray, env_id: str, task: int = 0,
                  episodes: int = 64, seed: int = 424242, device="cpu", frameskip: int = 4, gray: str = "rgb",
                  max_steps: int = 30000, check_every: int = 32, backend: str = "torch", compute_dtype=None) -> dict:
    """Held-out evaluation of ONE path of a trained super-network: ``episodes`` fresh envs (their own seed, none of
    the training envs), each playing exactly one episode under the SAMPLED policy (seeded multinomial, so a repeat
    replays the same episodes) of the path ``expressed`` [L, M] with the weights ``flat`` (copied, never trained).
    The forward is the fp32 PyTorch oracle (models/pathnet.py trunk_forward_ref): independent of the HIP kernels
    that produced the training fitness (the env steps in its HIP kernel on a GPU).  The reference's equivalent is its display path (run_policy,
    game_ac_network.py:458-465); it has no held-out check of a tournament winner.

    Returns {"mean", "min", "max", "finished", "episodes", "steps", "returns"}; an env that finished no episode in
    ``max_steps`` counts as unfinished (``finished`` < ``episodes``) and is left out of the mean.

    ``backend="hip"`` plays the same evaluation on the forward-only HIP engine (runtime/evaluator.py) at
    ``compute_dtype``: the path replicated over ceil(episodes / 32) rows of 32 envs made with the same ``seed`` (the
    first ``episodes`` of them count, the rest pad the batch to the kernels' shape), quota 1, Gumbel-max sampling
    keyed by ``seed`` (a repeat replays the same episodes; they are not the torch generator's draws, so the two
    backends agree statistically, not episode by episode).  It is the training kernels' forward, not the independent
    oracle.  Every result also carries ``backend`` and ``compute_dtype``; the hip one adds ``last_finish_step``."""
    if resolve_eval_backend(backend, net_cfg, env_id, compute_dtype) == "hip":
        return _evaluate_path_hip(net_cfg, flat, expressed, env_id, task, episodes, seed, device, frameskip, gray,
                                  max_steps, check_every, compute_dtype)
    model = ACPathNet(net_cfg, 1, device, "torch")
    model.store.flat.data.copy_(flat.detach().to(model.store.flat.device, torch.float32))
    model.set_paths(np.asarray(expressed, np.float32)[None])
    model.task = task
    gen = torch.Generator(device=device).manual_seed(seed)
    kw = {} if env_id.startswith("CartPole") else dict(frameskip=frameskip, gray=gray)
    kw.update(obs_dim_kwargs(env_id, net_cfg.input_shape))
    # on a GPU the env steps in its HIP kernel (bit-exact to the torch game, tests/test_envs.py / test_games_hip.py):
    # the torch Pong's per-sub-frame ops made a 7 K-step evaluation take 65 s
    env_backend = "hip" if torch.device(device).type == "cuda" else "torch"
    try:
        env = make(env_id, num_envs=episodes, device=device, seed=seed, backend=env_backend, **kw)
    except (NotImplementedError, ValueError, RuntimeError):
        env = make(env_id, num_envs=episodes, device=device, seed=seed, backend="torch", **kw)
    obs = env.reset()
    state = model.init_state(episodes)
    ret = torch.zeros(episodes, device=device)
    fin = torch.zeros(episodes, dtype=torch.bool, device=device)
    steps = 0
    for steps in range(1, max_steps + 1):
        logits, _, state = model.forward(obs, episodes, state)
        a = torch.multinomial(torch.softmax(logits.float(), -1), 1, generator=gen).reshape(-1)
        obs, _, d, info = env.step(a)
        d = d.bool()
        first = d & ~fin
        ret = torch.where(first, info["episode_return"].float(), ret)
        fin |= d
        if state is not None:
            keep = (~d).float()[:, None]
            state = (state[0] * keep, state[1] * keep)
        if steps % check_every == 0 and bool(fin.all()):
            break
    r = ret[fin].cpu().numpy().astype(np.float64)
    return {"mean": float(r.mean()) if r.size else float("nan"), "min": float(r.min()) if r.size else None,
            "max": float(r.max()) if r.size else None, "finished": int(r.size), "episodes": int(episodes),
            "steps": int(steps), "policy": "sampled", "seed": int(seed),
            "returns": [float(x) for x in r], "backend": "torch", "compute_dtype": "fp32"}


def _evaluate_path_hip(net_cfg, flat, expressed, env_id, task, episodes, seed, device, frameskip, gray, max_steps,
                       check_every, compute_dtype) -> dict:
    from ..runtime.evaluator import HipEvaluator, env_shape
    rows, E = env_shape(net_cfg, episodes)
    ev = HipEvaluator(net_cfg, env_id, rows, E, chunk=HIP_CHUNK, device=_hip_device(device),
                      compute_dtype=compute_dtype, env_seed=seed, nvalid=int(episodes), frameskip=frameskip, gray=gray)
    try:
        ev.load(flat, np.asarray(expressed, np.float32), task)
        rets = ev.run(quota=1, max_steps=max_steps, sample=True, seed=seed,
                      check_every=max(1, int(check_every) // HIP_CHUNK))
        last = ev.last
        dtype = ev.compute_dtype
    finally:
        ev.close()
    r = np.asarray([x[0] for x in rets if x], np.float64)
    ends = last["endstep"][:, 0][last["cnt"] > 0]
    return {"mean": float(r.mean()) if r.size else float("nan"), "min": float(r.min()) if r.size else None,
            "max": float(r.max()) if r.size else None, "finished": int(r.size), "episodes": int(episodes),
            "steps": int(last["steps"]), "policy": "sampled", "seed": int(seed),
            "returns": [float(x) for x in r], "backend": "hip", "compute_dtype": dtype,
            "last_finish_step": int(ends.max()) if ends.size else None}
