"""The last three synthetic Doom levels: HIP game logic (csrc/games.hip, game ids 12-14) vs the torch oracle
(envs/doom_world_games.py), bit-exact under the play of tests/test_doom_world_games.py; the frame ring, the
global-index RNG identity, the launcher's contract and the engine on ``doom-deathmatch`` (the first task on the 8-way
head)."""
import ctypes
import math

import pytest
import torch

from pathnet_gym_amd.envs.atari_games import GAMES
from test_doom_world_games import ACTION_SEED, EXPECTED, NAMES, NEEDED, SEED, _state, play


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_world_game_matches_torch(hip_lib, name):
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
    st = _state(et)
    eh.sync_from_device()
    for k, v in st.items():
        assert torch.equal(getattr(eh, k), v), k


@pytest.mark.gpu
def test_hip_deathmatch_frame_ring_matches_packed_stacks(hip_lib):
    """step_ring_into reconstructs, through the engine's stack rule, exactly the packed 4-frame stacks of step()
    (DoomDeathmatch: posts, pickups, monsters and fireballs all move with the player's position and heading)."""
    name = "DoomDeathmatch"
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
def test_hip_my_way_home_two_ranks_worth_of_envs(hip_lib):
    """The second half of 96 envs as its own env object with id_base = 48 reproduces the one-process run: the RNG
    identity is the global env index (the start room, place and heading of every reset)."""
    N, H = 96, 48
    full = GAMES["DoomMyWayHome"](N, device="cuda", seed=SEED, backend="hip")
    half = GAMES["DoomMyWayHome"](H, device="cuda", seed=SEED, backend="hip")
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
    for k in ("px", "pz", "th", "tic", "counter"):
        assert torch.equal(getattr(full, k)[H:], getattr(half, k)), k
    assert not torch.equal(full.px[:H], half.px)          # and the first half draws other starts
    assert not torch.equal(full.th[:H], half.th)


@pytest.mark.gpu
def test_launcher_contract_for_the_new_ids(hip_lib):
    from pathnet_gym_amd.ops import envs as henv
    for name, gid in zip(NAMES, (12, 13, 14)):
        assert henv.GAME_IDS[name] == gid
        env = GAMES[name](4, device="cpu", seed=1)
        env.reset()
        ns, nr = henv.game_layout(name)
        assert ns == env._hip_pack().shape[1] and nr == len(env.scene().colors) <= 40
    ns, nr = ctypes.c_int(0), ctypes.c_int(0)
    assert hip_lib.game_layout(14, ctypes.byref(ns), ctypes.byref(nr)) == 0
    assert hip_lib.game_layout(15, ctypes.byref(ns), ctypes.byref(nr)) == -1
    assert hip_lib.game_layout(11, ctypes.byref(ns), ctypes.byref(nr)) == -1


def _doom_deathmatch_trainer(seed=1):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.config import preset
    cfg = preset("doom-deathmatch")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 4, 16, 5       # 16 envs per path is the engine's smallest
    cfg.backend = "hip"
    cfg.compute_dtype = "fp32x"
    cfg.frame_ring = True
    cfg.use_graph = True
    cfg.deterministic = True
    cfg.seed = cfg.ga.seed = seed
    cfg.gc_freeze = False
    return PathNetTrainer(cfg, device="cuda:0")


@pytest.mark.gpu
def test_engine_trains_doom_deathmatch_on_the_frame_ring(hip_lib):
    """PathNetTrainer on ``doom-deathmatch`` (4 paths x 16 envs, T = 5): HIP engine, HIP game logic on the frame
    ring, graph-captured updates on the 8-way head; finite losses and weights, and the same seed gives the same
    weights."""
    flats = []
    for _ in range(2):
        tr = _doom_deathmatch_trainer()
        assert tr.env.HIP_GAME == "DoomDeathmatch" and tr.env._hip and tr.env.num_actions == 8
        assert tr.cfg.net.num_actions == 8
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
