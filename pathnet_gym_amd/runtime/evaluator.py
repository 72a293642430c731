"""Forward-only HIP engine: evaluate P paths x E envs without a backward.

An evaluation is a sequence of chunks of T steps on one stream:

  for t in 0..T-1:                                   (HipEngine._rollout_only_body)
      trunk fwd layer 0..L-1 -> (fused LSTM cell) -> heads fwd, argmax or Gumbel-max sample -> env step
  episode ledger                                     (csrc/heads.hip eval_ledger_kernel)
  carry: LSTM state, frame ring, sampling counter    (HipEngine._carry_body)

The rollout goes through the training engine's own step helpers on a ``HipEngine(forward_only=True)``: the same
kernels and the same precision as training, but no gradient buffers, no optimizer tables and no bootstrap forward.
Finished episodes are accounted on the device: the ledger records, per env, the return and the end step of its
first ``quota`` episodes, advances the step clock and counts the envs still short of their quota.  A chunk is
captured once per parity as a hipGraph, so a whole evaluation is graph replays plus one 4-byte read of that count
every ``check_every`` chunks.

Envelope: the on-device envs (CartPole-v1, Acrobot-v1, MountainCar-v0 and the synthetic games of envs/registry.py),
E <= 32, feed-forward nets and LSTM nets whose widths the fused cells take (multiples of 64).  ``unsupported_reason``
names what is outside it.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

MAX_ENVS_PER_PATH = 32          # the shapes training runs (bench: 32 envs per path)
PRECISIONS = ("bf16", "fp32", "fp32x")


def resolve_compute_dtype(net_cfg, compute_dtype: Optional[str]) -> str:
    """The trainer's rule (algo/trainer.py): default bf16; fp32x falls back to the fp32 engine for a trunk that has
    no split-operand kernels."""
    dt = compute_dtype or "bf16"
    if dt not in PRECISIONS:
        raise ValueError(f"compute_dtype {dt!r}: expected one of {PRECISIONS}")
    if dt == "fp32x":
        from ..ops.pathnet_ops import x3_unsupported_reason
        if x3_unsupported_reason(net_cfg) is not None:
            dt = "fp32"
    return dt


def min_envs_per_path(net_cfg) -> int:
    """Smallest envs_per_path the trunk kernels take: every conv forward, in every precision, wants E * Ho * Wo to be
    a multiple of 16 (16 for the reference pixel trunk, whose first layer has 39 x 29 outputs; 1 for vector nets)."""
    import math
    e = 1
    for spec, (ins, outs, K, cin) in zip(net_cfg.layers, net_cfg.layer_shapes()):
        if spec.kind == "conv":
            e = max(e, 16 // math.gcd(16, outs[0] * outs[1]))
    return e


def env_shape(net_cfg, n_envs: int):
    """(rows, envs per row) that hold ``n_envs`` envs of one path: as many envs per row as training runs (up to
    MAX_ENVS_PER_PATH), rounded up to what the conv kernels take; the caller pads with envs beyond nvalid."""
    step = min_envs_per_path(net_cfg)
    E = min(MAX_ENVS_PER_PATH, -(-max(1, int(n_envs)) // step) * step)
    return -(-int(n_envs) // E), E


def unsupported_reason(net_cfg, env_id: str, compute_dtype: Optional[str] = None,
                       envs_per_path: int = 1) -> Optional[str]:
    """Why HipEvaluator cannot run this net on this env (None: it can).  Host arithmetic only, no GPU needed:
    ``backend="auto"`` (algo/evaluate.py) asks this before it picks the hip backend."""
    from ..envs.registry import is_synthetic
    from ..ops.pathnet_ops import geometry_unsupported_reason
    from ..envs.control import CONTROL_IDS, obs_dim_kwargs
    if not (is_synthetic(env_id) or env_id in CONTROL_IDS):
        return f"env {env_id!r} is stepped on the host (Gym bridge), not by a HIP kernel"
    try:
        obs_dim_kwargs(env_id, net_cfg.input_shape)
    except ValueError as e:
        return str(e)
    if envs_per_path > MAX_ENVS_PER_PATH:
        return f"envs_per_path={envs_per_path} > {MAX_ENVS_PER_PATH} (replicate the path instead)"
    if envs_per_path % min_envs_per_path(net_cfg) != 0:
        return (f"envs_per_path={envs_per_path} is not a multiple of {min_envs_per_path(net_cfg)} (the conv kernels "
                "take E * Ho * Wo in multiples of 16; pad with envs beyond nvalid)")
    if net_cfg.use_lstm and (net_cfg.feature_dim % 64 != 0 or net_cfg.lstm_size % 64 != 0):
        return (f"LSTM widths {net_cfg.feature_dim} -> {net_cfg.lstm_size} are not multiples of 64: the engine would "
                "run its hybrid autograd LSTM, which has no forward-only form")
    try:
        dt = resolve_compute_dtype(net_cfg, compute_dtype)
    except ValueError as e:
        return str(e)
    why = geometry_unsupported_reason(net_cfg, dt)
    if why is not None:
        return f"HIP trunk: {why}"
    return None


def seed_counter(seed: int) -> int:
    """First value of the sampling counter of a run with ``seed``.  The heads kernels key their Gumbel draws by
    (engine seed, counter * (T + 1) + step, global row); the engine seed is a scalar of the captured launches, the
    counter lives on the device, so the run's seed enters through the counter and a new seed needs no recapture.
    A multiplicative hash spreads neighbouring seeds over the 2^32 step keys."""
    return ((int(seed) & 0xFFFFFFFF) * 2654435761) & 0x7FFFFFFF


class HipEvaluator:
    """``paths`` paths x ``envs_per_path`` envs of ``env_id``, stepped in chunks of ``chunk`` steps.  Envs
    [0, nvalid) are accounted by the ledger; the rest only pad the batch to a full shape."""

    def __init__(self, net_cfg, env_id: str, paths: int, envs_per_path: int, chunk: int = 20, device="cuda",
                 compute_dtype: Optional[str] = None, env_seed: int = 0, nvalid: Optional[int] = None,
                 use_graph: bool = True, frameskip: int = 4, gray: str = "rgb", frame_ring: Optional[bool] = None,
                 key_seed: int = 1):
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("HipEvaluator needs a GPU device")
        if paths <= 0 or envs_per_path <= 0 or chunk <= 0:
            raise ValueError("paths, envs_per_path and chunk must be positive")
        why = unsupported_reason(net_cfg, env_id, compute_dtype, envs_per_path)
        if why is not None:
            raise NotImplementedError(f"HipEvaluator: {why}")
        from ..config import A2CConfig, TrainConfig
        from ..envs.registry import make
        from ..models.acnet import ACPathNet
        from .engine import HipEngine
        self.compute_dtype = resolve_compute_dtype(net_cfg, compute_dtype)
        self.P, self.E, self.T = int(paths), int(envs_per_path), int(chunk)
        self.B = self.P * self.E
        self.nvalid = self.B if nvalid is None else int(nvalid)
        if not 0 <= self.nvalid <= self.B:
            raise ValueError(f"nvalid={nvalid} outside [0, {self.B}]")
        self.env_id = env_id
        self.model = ACPathNet(net_cfg, self.P, self.device, "hip", compute_dtype=self.compute_dtype)
        self.model.store.flat.requires_grad_(False)          # never trained
        kw = {} if env_id.startswith("CartPole") else dict(frameskip=frameskip, gray=gray)
        from ..envs.control import obs_dim_kwargs
        kw.update(obs_dim_kwargs(env_id, net_cfg.input_shape))
        self.env = make(env_id, num_envs=self.B, device=self.device, seed=env_seed, backend="hip", **kw)
        self.env.reset()
        if frame_ring is None:
            frame_ring = self.compute_dtype == "fp32x"          # where the trainer's shipped shape picks it
        cfg = TrainConfig(env=env_id, tasks=[env_id], paths=self.P, envs_per_path=self.E, net=net_cfg,
                          a2c=A2CConfig(t_max=self.T), backend="hip", compute_dtype=self.compute_dtype,
                          use_graph=bool(use_graph), frame_ring=bool(frame_ring), rollout_groups=1)
        self.engine = HipEngine(self.model, self.env, cfg, None, seed=key_seed, forward_only=True)
        if self.engine.hybrid:
            self.close()
            raise NotImplementedError("HipEvaluator: this LSTM net runs the engine's hybrid autograd LSTM, which "
                                      "has no forward-only form")
        self.use_graph = self.engine.use_graph          # False too for an env that is not graph safe
        dev = self.device
        self.cnt = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.clock = torch.zeros(1, dtype=torch.int64, device=dev)
        self.pending = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ret = self.endstep = None
        self._key = None          # (quota, max_steps, greedy) of the captured graphs and of ret / endstep
        self._graphs = None
        self._snapshot_env()
        self.last = None

    # -- weights -----------------------------------------------------------------------------------------------
    def load(self, flat: torch.Tensor, expressed, task: int = 0):
        """Install the weights ``flat`` (copied: the caller's tensor is only read) and the expressed paths
        [P, L, M] (one [L, M] path is given to every row), then refresh the kernels' operand copies."""
        m = self.model
        with torch.no_grad():
            m.store.flat.copy_(flat.detach().to(device=self.device, dtype=torch.float32))
        ex = np.asarray(expressed, np.float32)
        if ex.ndim == 2:
            ex = np.repeat(ex[None], self.P, 0)
        m.set_paths(ex)
        m.task = int(task)
        m.hip.refresh_weights()
        if self._graphs is not None and m.cfg.per_task_heads:
            self._graphs = None          # the head's parameter offsets are scalars of the captured launches

    # -- env state: snapshot after the first reset, restored in place before every run -------------------------------
    def _snapshot_env(self):
        from ..envs.cartpole import CartPoleVec
        from ..envs.control import ControlVec
        from ..envs.pong import PongVec
        from ..ops import envs as henv
        env = self.env
        # the kernels' own state buffers exist before the snapshot (they are otherwise made by the first step)
        if isinstance(env, PongVec) and not hasattr(env, "_st32"):
            henv.pong_sync_to_device(env)
        if isinstance(env, (CartPoleVec, ControlVec)) and not hasattr(env, "_steps32"):
            henv.control_sync_to_device(env)
        self._env_obs0 = env.obs.clone() if self.engine.pixels else None
        self._env_snap = [(k, v, v.clone()) for k, v in vars(env).items()
                          if isinstance(v, torch.Tensor) and v.device.type == "cuda" and k != "obs"]

    def _restore(self, seed: int):
        env, eng = self.env, self.engine
        for k, ref, saved in self._env_snap:
            ref.copy_(saved)
            setattr(env, k, ref)
        if self._env_obs0 is not None:
            env.obs = self._env_obs0.clone()
        eng._par = 0
        eng.load_obs(env)
        if eng.lstm_hip:
            eng.hst.zero_()
            eng.cst.zero_()
        eng.dones.zero_()
        eng.ctr.fill_(seed_counter(seed))
        self.cnt.zero_()
        self.clock.zero_()
        self.pending.fill_(self.nvalid)

    # -- one chunk -----------------------------------------------------------------------------------------------------
    def _ledger(self):
        from ..ops import _lib
        quota, max_steps, _ = self._key
        eng = self.engine
        _lib.call("launch_eval_ledger", eng.dones.data_ptr(), eng.epret.data_ptr(), self.T, self.B, self.nvalid,
                  quota, max_steps, self.cnt.data_ptr(), self.ret.data_ptr(), self.endstep.data_ptr(),
                  self.clock.data_ptr(), self.pending.data_ptr(), _lib.stream())

    def _chunk_body(self, record: Optional[list] = None):
        eng = self.engine
        eng._rollout_only_body(greedy=self._key[2])
        if record is not None:
            record.append(self._record())
        self._ledger()
        eng._carry_body()

    def _record(self) -> dict:
        """Clones of one chunk's rollout buffers (taken before the carry rewrites the ring's first planes)."""
        eng, T = self.engine, self.T
        rec = dict(obs=eng.obs_stacks(T).clone(), logits=eng.logits[:T].clone(), values=eng.values[:T].clone(),
                   actions=eng.actions[:T].clone(), dones=eng.dones.clone(), epret=eng.epret.clone(),
                   ctr=int(eng.ctr.item()), feat=eng.acts[-1][:T].float().clone())
        if eng.lstm_hip:
            rec["h"] = eng.hst[:T + 1].float().clone()          # slot t: state entering step t (before its done mask)
            rec["c"] = eng.cst[:T + 1].clone()
        return rec

    def _capture(self):
        from .engine import CAPTURE_MODE
        eng = self.engine
        torch.cuda.synchronize()
        par = eng._par
        graphs = []
        for q in ((0, 1) if eng._parities else (par,)):          # one graph per parity, as the engine's rollout
            eng._par = q
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
                self._chunk_body()
            graphs.append(g)
        eng._par = par
        self._graphs = graphs
        torch.cuda.synchronize()

    def _prepare(self, quota: int, max_steps: int, greedy: bool):
        key = (int(quota), int(max_steps), bool(greedy))
        if quota <= 0 or max_steps <= 0:
            raise ValueError("quota and max_steps must be positive")
        if key == self._key:
            return
        # quota, max_steps and greedy are scalars of the launches: other values need other graphs
        self._graphs = None
        self._key = key
        if self.ret is None or self.ret.shape[1] != key[0]:
            self.ret = torch.zeros(self.B, key[0], dtype=torch.float32, device=self.device)
            self.endstep = torch.zeros(self.B, key[0], dtype=torch.int32, device=self.device)

    # -- the evaluation ------------------------------------------------------------------------------------------------
    def run(self, quota: int = 1, max_steps: int = 30000, sample: bool = True, seed: int = 0, check_every: int = 1,
            record: Optional[list] = None, env_stride: int = 1) -> List[List[float]]:
        """Play until every env in [0, nvalid) has finished ``quota`` episodes or ``max_steps`` steps have been
        played (the clock advances by whole chunks; steps past ``max_steps`` are not accounted).  ``sample`` False
        plays the argmax action, True samples the policy keyed by ``seed``: the same seed replays the same episodes
        on the same object, bit for bit, without recapturing.  Reads 4 bytes (the pending count) every
        ``check_every`` chunks.  ``record``: a list that receives one dict of buffer clones per chunk (eager).
        ``env_stride`` > 1: only envs 0, stride, 2 stride, ... of [0, nvalid) are wanted (one env per path when the
        stride is E, the others padding a path's row to the kernels' shape): the run stops once THEY hold their quota
        (one device reduction over their counts and a 1-byte read instead of the pending word) and only their lists
        are returned.
        -> per-env lists of episode returns; ``self.last`` holds cnt / ret / endstep of every env in [0, nvalid) and
        steps."""
        self._prepare(quota, max_steps, not sample)
        self._restore(seed)
        eng = self.engine
        self.ret.zero_()
        self.endstep.zero_()
        check_every = max(1, int(check_every))
        env_stride = max(1, int(env_stride))
        chunks = 0
        while True:
            capture = False
            if record is not None or not self.use_graph:
                self._chunk_body(record)
            elif self._graphs is None:
                self._chunk_body()          # first chunk eagerly (validates every launch), then capture
                capture = True
            else:
                self._graphs[eng._par if eng._parities else 0].replay()
            if eng._parities:
                eng._par ^= 1          # the next chunk starts from the buffer / ring slots this one's last step wrote
            chunks += 1
            if capture:
                self._capture()
            over = chunks * self.T >= max_steps
            if over or chunks % check_every == 0:
                if env_stride == 1:
                    done = int(self.pending.item()) == 0
                else:
                    done = bool((self.cnt[:self.nvalid:env_stride] >= quota).all().item())
                if done or over:
                    break
        if eng.hip.x3:
            eng.hip.check_x3_status()
        n = self.nvalid
        cnt = self.cnt[:n].cpu().numpy()
        ret = self.ret[:n].cpu().numpy()
        end = self.endstep[:n].cpu().numpy()
        self.last = dict(cnt=cnt, ret=ret, endstep=end, steps=int(self.clock.item()), chunks=chunks)
        return [[float(x) for x in ret[b, :cnt[b]]] for b in range(0, n, env_stride)]

    def stepkey(self, ctr: int, t: int) -> int:
        """The heads kernels' step key of step t of the chunk whose counter is ``ctr`` (a2c_math.sampling_u01)."""
        return (ctr * (self.T + 1) + t) & 0xFFFFFFFF

    def close(self):
        """Drop every GPU buffer.  The model <-> kernel-view cycle (ACPathNet.hip.model) is cut, so nothing waits for
        the cyclic collector."""
        self._graphs = None
        env = getattr(self, "env", None)
        if env is not None:
            env.close()
        model = getattr(self, "model", None)
        if model is not None and model.hip is not None:
            model.hip.model = None
            model.hip = None
        eng = getattr(self, "engine", None)
        if eng is not None:
            eng.model = eng.hip = eng.env = None
        self.engine = self.model = self.env = None
        self._env_snap = self._env_obs0 = None
        self.cnt = self.clock = self.pending = self.ret = self.endstep = None
