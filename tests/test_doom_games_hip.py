"""Synthetic Doom scenarios: HIP game logic (csrc/games.hip, game ids 5-7) vs the torch oracle
(envs/doom_games.py), bit-exact; the frame ring, the global-index RNG identity and the engine on ``doom-basic``."""
import math

import pytest
import torch

from pathnet_gym_amd.envs.atari_games import GAMES

NAMES = ["DoomBasic", "DoomDefendCenter", "DoomTakeCover"]
SEED, ACTION_SEED = 11, 3


def _state(env):
    return {name: getattr(env, name).clone() for name, _ in env._fields()}


class Events:
    """Counts, from the torch oracle's state before and after a step, the events that make each game."""

    def __init__(self, env):
        self.env = env
        self.count = {}
        self.snap()

    def snap(self):
        e = self.env
        self.prev = {k: getattr(e, k).clone() for k in ("alive", "health", "fact") if hasattr(e, k)}

    def add(self, key, n):
        self.count[key] = self.count.get(key, 0) + int(n)

    def step(self, reward, done):
        e, p = self.env, self.prev
        run = ~done                                            # a finished env shows the next episode's state
        if e.id == "DoomBasic":
            self.add("kill", (reward > 0).sum())
            self.add("miss", (run & (reward == e.SHOT + e.frameskip * e.LIVING)).sum())
        elif e.id == "DoomDefendCenter":
            self.add("kill", (reward > 0).sum())
            self.add("respawn", (run[:, None] & ~p["alive"] & e.alive).sum())
            self.add("bite", (run & (e.health < p["health"])).sum())
        else:
            gone = (p["fact"] & ~e.fact).sum(1)
            hits = (p["health"] - e.health) // e.DAMAGE
            self.add("hit", (hits * run).sum())
            self.add("dodge", ((gone - hits) * run).sum())
        self.snap()


def play(name, device, hip, N=96, steps=300, cap=60):
    """The oracle (and, with ``hip``, the HIP env next to it, compared at every step) under random actions with a
    quarter of the envs forced to action 1 every 5th step; returns the oracle's event counts."""
    et = GAMES[name](N, device=device, seed=SEED, backend="torch")
    eh = GAMES[name](N, device=device, seed=SEED, backend="hip") if hip else None
    envs = [e for e in (et, eh) if e is not None]
    if hip:
        assert eh._hip and not et._hip
    for e in envs:
        e.max_episode_steps = cap                      # time-limit resets on top of the games' own endings
    obs = [e.reset() for e in envs]
    assert all(torch.equal(obs[0], o) for o in obs)
    ev = Events(et)
    g = torch.Generator().manual_seed(ACTION_SEED)
    ndone = 0
    for i in range(steps):
        a = torch.randint(0, et.num_actions, (N,), generator=g).to(device)
        if i % 5 == 0:
            a[: N // 4] = 1
        if hip:
            ot, rt, dt, it = et.step(a)
            oh, rh, dh, ih = eh.step(a)
            assert torch.equal(rt, rh), i
            assert torch.equal(dt, dh), i
            assert torch.equal(it["episode_return"], ih["episode_return"]), i
            assert torch.equal(ot, oh), i
        else:
            rt, dt, _ = et._advance(a)
        ev.step(rt, dt)
        ndone += int(dt.sum())
    ev.add("done", ndone)
    return et, eh, ev.count


# what the oracle alone shows on the CPU with these seeds (N = 96, 300 steps, episodes capped at 60 steps):
EXPECTED = {
    "DoomBasic": {"kill": 369, "miss": 6059, "done": 679},
    "DoomDefendCenter": {"kill": 1459, "respawn": 1323, "bite": 4374, "done": 1152},
    "DoomTakeCover": {"hit": 3141, "dodge": 9250, "done": 745},
}
NEEDED = {"DoomBasic": ("kill", "miss"), "DoomDefendCenter": ("kill", "respawn", "bite"),
          "DoomTakeCover": ("hit", "dodge")}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_run_contains_the_games_events(name):
    """CPU: the seeds of the bit-exact comparison give a run with every event of the game in it."""
    _, _, count = play(name, "cpu", hip=False)
    print(name, count)
    for k in NEEDED[name]:
        assert count[k] >= 1, (k, count)
    assert count == EXPECTED[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_doom_game_matches_torch(hip_lib, name):
    et, eh, count = play(name, "cuda", hip=True)
    for k in NEEDED[name]:
        assert count[k] >= 1, (k, count)
    assert count == EXPECTED[name], count                 # the same run as the CPU oracle's
    st = _state(et)
    eh.sync_from_device()
    for k, v in st.items():
        assert torch.equal(getattr(eh, k), v), k
    m = torch.zeros(et.num_envs, dtype=torch.bool, device="cuda")          # reset_where through the kernel
    m[::3] = True
    et.reset_where(m)
    eh.reset_where(m)
    assert torch.equal(et.obs, eh.obs)


@pytest.mark.gpu
def test_hip_doom_frame_ring_matches_packed_stacks(hip_lib):
    """step_ring_into reconstructs, through the engine's stack rule, exactly the packed 4-frame stacks of step()
    (one game: the rasteriser is shared; DefendCenter has the most moving rectangles)."""
    name = "DoomDefendCenter"
    N, T = 64, 60
    ep = GAMES[name](N, device="cuda", seed=7, backend="hip")
    er = GAMES[name](N, device="cuda", seed=7, backend="hip")
    assert er.supports_ring
    for e in (ep, er):
        e.max_episode_steps = 25
    o0 = ep.reset()
    assert torch.equal(o0, er.reset())
    frames = torch.zeros(N, T + 4, 160 * 120, dtype=torch.uint8, device="cuda")
    st = o0.reshape(N, 160 * 120, 4)
    for c in range(4):
        frames[:, c].copy_(st[:, :, c])
    fc = torch.zeros(T + 1, N, dtype=torch.uint8, device="cuda")
    rw, dn, eret = (torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"),
                    torch.zeros(N, device="cuda"))
    g = torch.Generator().manual_seed(5)
    ndone = 0
    ar = torch.arange(N, device="cuda")[:, None]
    c4 = torch.arange(4, device="cuda")[None, :]
    for t in range(T):
        a = torch.randint(0, ep.num_actions, (N,), generator=g).cuda()
        obs, r, d, _ = ep.step(a)
        er.step_ring_into(a.to(torch.int32), frames, t + 4, fc[t], fc[t + 1], rw, dn, eret)
        assert torch.equal(rw, r.float()), t
        assert torch.equal(dn.bool(), d.bool()), t
        idx = (t + 1) + torch.maximum(c4, fc[t + 1].long()[:, None])
        stack = frames[ar, idx].permute(0, 2, 1).reshape(N, 160, 120, 4)
        assert torch.equal(stack, obs), t
        ndone += int(d.sum())
    assert ndone > 0
    assert obs.float().std() > 0


@pytest.mark.gpu
def test_hip_doom_basic_two_ranks_worth_of_envs(hip_lib):
    """The second half of 96 envs as its own env object with id_base = 48 reproduces the one-process run: the RNG
    identity is the global env index (the monster's x at every reset)."""
    N, H = 96, 48
    full = GAMES["DoomBasic"](N, device="cuda", seed=SEED, backend="hip")
    half = GAMES["DoomBasic"](H, device="cuda", seed=SEED, backend="hip")
    half.set_id_base(H)
    for e in (full, half):
        e.max_episode_steps = 20
    assert torch.equal(full.reset()[H:], half.reset())
    g = torch.Generator().manual_seed(ACTION_SEED)
    ndone = 0
    for i in range(80):
        a = torch.randint(0, 4, (N,), generator=g).cuda()
        of, rf, df, inf = full.step(a)
        oh, rh, dh, inh = half.step(a[H:].contiguous())
        assert torch.equal(of[H:], oh) and torch.equal(rf[H:], rh) and torch.equal(df[H:], dh), i
        assert torch.equal(inf["episode_return"][H:], inh["episode_return"]), i
        ndone += int(dh.sum())
    assert ndone > H                                      # every env of the half was reset at least once
    full.sync_from_device()
    half.sync_from_device()
    assert torch.equal(full.mx[H:], half.mx) and torch.equal(full.counter[H:], half.counter)
    assert not torch.equal(full.mx[:H], half.mx)          # and the first half draws other monsters


def _doom_basic_trainer(seed=1):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.config import preset
    cfg = preset("doom-basic")
    # 16 envs per path is the engine's smallest: its conv kernels tile 16 output rows per path, and conv1's 39 x 29
    # output plane is odd, so envs_per_path * Ho * Wo is a multiple of 16 only from 16 envs up (4 envs per path is
    # rejected: "envs_per_path*Ho*Wo must be a multiple of 16", ops/pathnet_ops.py)
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 4, 16, 5
    cfg.backend = "hip"
    cfg.compute_dtype = "fp32x"
    cfg.frame_ring = True
    cfg.use_graph = True
    cfg.deterministic = True
    cfg.seed = cfg.ga.seed = seed
    cfg.gc_freeze = False
    return PathNetTrainer(cfg, device="cuda:0")


@pytest.mark.gpu
def test_engine_trains_doom_basic_on_the_frame_ring(hip_lib):
    """PathNetTrainer on ``doom-basic`` (4 paths x 16 envs, T = 5): HIP engine, HIP game logic on the frame ring,
    graph-captured updates; finite losses and weights, and the same seed gives the same weights."""
    flats = []
    for _ in range(2):
        tr = _doom_basic_trainer()
        assert tr.env.HIP_GAME == "DoomBasic" and tr.env._hip
        assert tr.engine.ring and tr.engine.use_graph
        for _ in range(3):
            st = tr.update()
        st = tr.flush() or st
        torch.cuda.synchronize()
        assert tr.engine.g_opt is not None, "graphs were not captured"
        for v in (st.loss_pi, st.loss_v, st.entropy):
            assert math.isfinite(v), st
        flat = tr.model.store.flat.detach().clone()
        assert torch.isfinite(flat).all()
        flats.append(flat)
        tr.env.close()
    assert torch.equal(flats[0], flats[1])
