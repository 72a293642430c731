"""Acrobot-v1 and MountainCar-v0, vectorised on device: gym's two other discrete classic-control tasks.

Dynamics and constants follow the classic-control definitions behind gym's ``Acrobot-v1`` (the "book" dynamics, one
classical RK4 step of dt = 0.2 with the torque held, no torque noise, 500-step limit, reward -1 per step and 0 on
the terminal one, reward_threshold -100) and ``MountainCar-v0`` (200-step limit, reward -1 per step,
reward_threshold -110).  State and arithmetic are fp32.

Like ``CartPoleVec`` (envs/cartpole.py) each class is two implementations: a pure torch one (oracle, CPU) and a HIP
step kernel (``csrc/control.hip``), with the same counter-based hash RNG keyed by the global env index, so the
resets agree bit for bit and the dynamics up to float rounding.  The attribute names are CartPoleVec's (``state``,
``steps``, ``ep_ret``, ``counter``, ``seed_int``, ``set_id_base``): the checkpoint and the evaluator treat the
three envs alike.

``obs_dim`` (native width <= obs_dim <= 8) is the width of the returned observation rows; the columns past the
native width are zeros.  One network with ``input_shape=(obs_dim,)`` can therefore play all three tasks.

An action >= 3 plays action 0.
"""
from __future__ import annotations

import math

import torch

from .base import VecEnv, env_rand_u32

MAX_OBS_DIM = 8          # the bf16 trunk's vector input row (ops/envs.py obs_to_bf16_padded)

# the ids of the on-device vector (classic-control) envs
CONTROL_IDS = ("CartPole-v1", "Acrobot-v1", "MountainCar-v0")


def check_obs_dim(env_id: str, native: int, obs_dim) -> int:
    """``obs_dim`` as an int, or a ValueError that names the env when it is outside [native, 8]."""
    od = native if obs_dim is None else int(obs_dim)
    if not native <= od <= MAX_OBS_DIM:
        raise ValueError(f"{env_id}: obs_dim={obs_dim} outside [{native}, {MAX_OBS_DIM}] (the env's observation has "
                         f"{native} values; rows are zero padded up to {MAX_OBS_DIM})")
    return od


NATIVE_OBS_DIM = {"CartPole-v1": 4, "Acrobot-v1": 6, "MountainCar-v0": 2}


def obs_dim_kwargs(env_id: str, input_shape) -> dict:
    """Keyword arguments that make vector env ``env_id`` return rows as wide as a net's ``input_shape``: ``{}`` for
    any other env and for CartPole-v1 at its own width 4, else ``{"obs_dim": width}``.  A net the env cannot feed (a
    pixel input, or a width outside [native, 8]) is refused here, by the env's name."""
    if env_id not in CONTROL_IDS:
        return {}
    shape = tuple(input_shape)
    if len(shape) != 1:
        raise ValueError(f"{env_id}: a vector env cannot feed a net with input_shape={shape}")
    if env_id == "CartPole-v1" and shape[0] == 4:
        return {}
    return {"obs_dim": check_obs_dim(env_id, NATIVE_OBS_DIM[env_id], shape[0])}


def pad_obs(obs: torch.Tensor, obs_dim: int) -> torch.Tensor:
    """[B, d] -> a new [B, obs_dim] tensor, columns d.. zero."""
    B, d = obs.shape
    if d == obs_dim:
        return obs.clone()
    out = torch.zeros(B, obs_dim, dtype=obs.dtype, device=obs.device)
    out[:, :d] = obs
    return out


class ControlVec(VecEnv):
    """Shared plumbing of the two envs: RNG, reset, step limit, auto-reset, padding.  Subclasses give the dynamics."""
    native_obs_dim = 0
    state_dim = 0
    hip_launcher = ""              # csrc/control.hip launcher of this game
    reset_scale = 0.0
    reset_offset = 0.0
    reset_streams = 0              # state values drawn at a reset (the rest start at 0)

    def __init__(self, num_envs: int, device="cpu", seed: int = 0, backend: str = "torch", obs_dim=None):
        self.obs_dim = check_obs_dim(self.id, self.native_obs_dim, obs_dim)
        self.num_envs = num_envs
        self.num_actions = 3
        self.obs_shape = (self.obs_dim,)
        self.obs_dtype = torch.float32
        self.device = torch.device(device)
        self.backend = backend
        self.state = torch.zeros(num_envs, self.state_dim, device=self.device)
        self.steps = torch.zeros(num_envs, dtype=torch.int32, device=self.device)
        self.ep_ret = torch.zeros(num_envs, device=self.device)
        self.counter = torch.zeros(num_envs, dtype=torch.int64, device=self.device)
        self.env_id = torch.arange(num_envs, dtype=torch.int64, device=self.device)
        self.seed(seed)

    def seed(self, seed: int):
        self.seed_int = seed & 0xFFFFFFFF
        self._seed = torch.tensor(self.seed_int, dtype=torch.int64, device=self.device)
        self.counter.zero_()

    # -- subclass hooks ------------------------------------------------------------------------------------------
    def _dynamics(self, state: torch.Tensor, a: torch.Tensor):
        """-> (new state [B, state_dim], terminal [B] bool, reward [B])."""
        raise NotImplementedError

    def _native_obs(self, state: torch.Tensor) -> torch.Tensor:
        return state

    # -- shared --------------------------------------------------------------------------------------------------
    def observe(self) -> torch.Tensor:
        """The current observation, [B, obs_dim] fp32, zero padded (a new tensor).  The HIP backend asks the step
        kernel's own row writer (csrc/control.hip), so it is bit-equal to what a step hands out."""
        if self.backend == "hip" and self.state.device.type == "cuda":
            from ..ops import envs as henv
            return henv.control_observe(self)
        return pad_obs(self._native_obs(self.state.float()), self.obs_dim)

    def _rand_state(self, mask):
        # separately rounded multiply and subtract: csrc/control.hip computes the same two roundings
        cols = []
        for s in range(self.state_dim):
            if s < self.reset_streams:
                u = (env_rand_u32(self._seed, self.env_id, self.counter, s) >> 8).float() * (1.0 / 16777216.0)
                cols.append(u * self.reset_scale - self.reset_offset)
            else:
                cols.append(torch.zeros(self.num_envs, device=self.device))
        init = torch.stack(cols, 1)
        self.counter += mask.long()
        return torch.where(mask[:, None], init, self.state)

    def reset(self):
        allm = torch.ones(self.num_envs, dtype=torch.bool, device=self.device)
        self.reset_where(allm)
        return self.observe()

    def reset_where(self, mask):
        hip_state = hasattr(self, "_steps32")
        if hip_state:
            self.steps = self._steps32.long()
            self.counter = self._ctr32.long() & 0xFFFFFFFF
        self.state = self._rand_state(mask)
        self.steps = torch.where(mask, torch.zeros_like(self.steps), self.steps)
        self.ep_ret = torch.where(mask, torch.zeros_like(self.ep_ret), self.ep_ret)
        if hip_state:
            from ..ops import envs as henv
            henv.control_sync_to_device(self)

    def step(self, actions: torch.Tensor):
        if self.backend == "hip":
            from ..ops import envs as henv
            return henv.control_step(self, actions)
        a = actions.long()
        a = torch.where((a >= 3) | (a < 0), torch.zeros_like(a), a)
        self.state, term, reward = self._dynamics(self.state, a)
        self.steps = self.steps + 1
        done = term | (self.steps >= self.max_episode_steps)
        self.ep_ret = self.ep_ret + reward
        ep_return = torch.where(done, self.ep_ret, torch.zeros_like(self.ep_ret))
        self.reset_where(done)
        return self.observe(), reward, done, {"episode_return": ep_return}


class MountainCarVec(ControlVec):
    id = "MountainCar-v0"
    reward_threshold = -110.0
    max_episode_steps = 200
    native_obs_dim = 2
    state_dim = 2
    hip_launcher = "launch_mountaincar_step"
    reset_scale, reset_offset, reset_streams = 0.2, 0.6, 1

    MIN_POS, MAX_POS, MAX_SPEED, GOAL_POS = -1.2, 0.6, 0.07, 0.5
    FORCE, GRAVITY = 0.001, 0.0025

    def _dynamics(self, state, a):
        p, v = state.unbind(1)
        v = v + ((a - 1).to(state.dtype) * self.FORCE + torch.cos(3.0 * p) * (-self.GRAVITY))
        v = v.clamp(-self.MAX_SPEED, self.MAX_SPEED)
        p = (p + v).clamp(self.MIN_POS, self.MAX_POS)
        lo = torch.tensor(self.MIN_POS, dtype=state.dtype, device=state.device)
        v = torch.where((p == lo) & (v < 0), torch.zeros_like(v), v)
        goal = torch.tensor(self.GOAL_POS, dtype=state.dtype, device=state.device)
        term = (p >= goal) & (v >= 0)
        reward = torch.full((self.num_envs,), -1.0, device=self.device)
        return torch.stack([p, v], 1), term, reward


class AcrobotVec(ControlVec):
    id = "Acrobot-v1"
    reward_threshold = -100.0
    max_episode_steps = 500
    native_obs_dim = 6
    state_dim = 4
    hip_launcher = "launch_acrobot_step"
    reset_scale, reset_offset, reset_streams = 0.2, 0.1, 4

    DT = 0.2
    M1 = M2 = 1.0
    L1 = 1.0
    LC1 = LC2 = 0.5
    I1 = I2 = 1.0
    G = 9.8
    MAX_VEL_1 = 4 * math.pi
    MAX_VEL_2 = 9 * math.pi

    def _dsdt(self, s, tau):
        m1, m2, l1, lc1, lc2, I1, I2, g = self.M1, self.M2, self.L1, self.LC1, self.LC2, self.I1, self.I2, self.G
        th1, th2, w1, w2 = s.unbind(1)
        c2, s2 = torch.cos(th2), torch.sin(th2)
        d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + 2.0 * l1 * lc2 * c2) + I1 + I2
        d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2
        phi2 = m2 * lc2 * g * torch.cos(th1 + th2 - math.pi / 2.0)
        phi1 = (-m2 * l1 * lc2 * w2 * w2 * s2 - 2.0 * m2 * l1 * lc2 * w2 * w1 * s2
                + (m1 * lc1 + m2 * l1) * g * torch.cos(th1 - math.pi / 2.0) + phi2)
        a2 = (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 * w1 * s2 - phi2) / (m2 * lc2 * lc2 + I2 - d2 * d2 / d1)
        a1 = -(d2 * a2 + phi1) / d1
        return torch.stack([w1, w2, a1, a2], 1)

    @staticmethod
    def _wrap(x):
        for _ in range(3):
            x = torch.where(x > math.pi, x - 2.0 * math.pi, x)
        for _ in range(3):
            x = torch.where(x < -math.pi, x + 2.0 * math.pi, x)
        return x

    def _dynamics(self, state, a):
        tau = (a - 1).to(state.dtype)
        dt = self.DT
        k1 = self._dsdt(state, tau)
        k2 = self._dsdt(state + (dt * 0.5) * k1, tau)
        k3 = self._dsdt(state + (dt * 0.5) * k2, tau)
        k4 = self._dsdt(state + dt * k3, tau)
        y = state + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        th1 = self._wrap(y[:, 0])
        th2 = self._wrap(y[:, 1])
        w1 = y[:, 2].clamp(-self.MAX_VEL_1, self.MAX_VEL_1)
        w2 = y[:, 3].clamp(-self.MAX_VEL_2, self.MAX_VEL_2)
        term = (-torch.cos(th1) - torch.cos(th1 + th2)) > 1.0
        reward = torch.where(term, torch.zeros_like(th1), torch.full_like(th1, -1.0))
        return torch.stack([th1, th2, w1, w2], 1), term, reward

    def _native_obs(self, state):
        th1, th2, w1, w2 = state.unbind(1)
        return torch.stack([torch.cos(th1), torch.sin(th1), torch.cos(th2), torch.sin(th2), w1, w2], 1)
