"""Synthetic Doom scenarios (envs/doom_games.py) on the CPU: packed state, the games' rules, scene coordinates,
rendering, scripted experts and the presets."""
import os
import re
import sys

import pytest
import torch

from pathnet_gym_amd.config import preset
from pathnet_gym_amd.envs import doom_games as dg
from pathnet_gym_amd.envs import registry
from pathnet_gym_amd.envs.atari_games import GAMES
from pathnet_gym_amd.envs.doom.scenarios import SCENARIOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["DoomBasic", "DoomDefendCenter", "DoomTakeCover"]
NOOP = 0


def make(name, n=2, seed=3):
    env = GAMES[name](n, device="cpu", seed=seed)
    env.reset()
    return env


def act(env, a):
    return env._advance(torch.full((env.num_envs,), a, dtype=torch.int64))


def test_games_are_registered_with_the_scenario_tables_constants():
    for name in NAMES:
        assert registry.is_synthetic(name) and registry.is_synthetic("Synth" + name + "-v0")
        env = registry.make(name, num_envs=1)
        assert isinstance(env, GAMES[name]) and env.HIP_GAME == name
    b, d, t = make("DoomBasic"), make("DoomDefendCenter"), make("DoomTakeCover")
    assert (b.LIVING, b.TIMEOUT) == (SCENARIOS["basic.cfg"]["living_reward"], SCENARIOS["basic.cfg"]["episode_timeout"])
    assert (d.DEATH_PENALTY, d.TIMEOUT) == (SCENARIOS["defend_the_center.cfg"]["death_penalty"],
                                            SCENARIOS["defend_the_center.cfg"]["episode_timeout"])
    assert (t.LIVING, t.TIMEOUT) == (SCENARIOS["take_cover.cfg"]["living_reward"],
                                     SCENARIOS["take_cover.cfg"]["episode_timeout"])
    assert b.BUTTONS == ["ATTACK", "MOVE_RIGHT", "MOVE_LEFT"] and d.BUTTONS == ["ATTACK", "TURN_RIGHT", "TURN_LEFT"]
    assert t.BUTTONS == ["MOVE_RIGHT", "MOVE_LEFT"]
    assert (b.num_actions, d.num_actions, t.num_actions) == (4, 4, 3)
    # the engine-backed ids still mean the real engine
    with pytest.raises(Exception) as ei:
        registry.make("gym_doom/DoomBasic-v0")
    assert type(ei.value).__name__ == "DependencyNotInstalled"


@pytest.mark.parametrize("name", NAMES)
def test_hip_constants_mirror_the_python_classes(name):
    """Every ``static constexpr int`` of the game's struct in csrc/games.hip equals the class constant of the same
    name (LIVING / DEATH_PENALTY / TIMEOUT: the scenario table's value the class imported)."""
    src = open(os.path.join(ROOT, "csrc", "games.hip")).read()
    view = src[src.index("struct DoomView {"):]
    body = src[src.index("struct %s : DoomView {" % name):]
    env = make(name)
    seen = 0
    for text, owner in ((view[:view.index("\n};")], dg), (body[:body.index("\n};")], env)):
        for line in re.findall(r"static constexpr int ([^;]*);", text):
            for k, v in re.findall(r"(\w+) = (-?\d+)(?=,|$)", line):
                if k in ("NBACK",):
                    continue
                want = owner.PILLARS[1] if k == "PILLAR" else getattr(owner, k)
                assert int(v) == want, (name, k)
                seen += 1
    assert seen >= 15


@pytest.mark.parametrize("name", NAMES)
def test_state_pack_roundtrip(name):
    """HIP_FIELDS round-trips every state tensor after 40 random steps: negative px / fvx, vec and mask fields."""
    env = GAMES[name](8, device="cpu", seed=5)
    env.reset()
    g = torch.Generator().manual_seed(0)
    neg = False
    for _ in range(40):
        env.step(torch.randint(0, env.num_actions, (8,), generator=g))
        neg |= any(bool((getattr(env, k) < 0).any()) for k, _ in env.HIP_FIELDS if getattr(env, k).dtype != torch.bool)
    kinds = {kind for _, kind in env.HIP_FIELDS}
    assert name == "DoomBasic" or {"vec", "mask"} <= kinds
    assert neg or name == "DoomDefendCenter"             # DefendCenter has no signed field
    ref = {k: getattr(env, k).clone() for k, _ in env._fields()}
    packed = env._hip_pack()
    other = GAMES[name](8, device="cpu", seed=5)
    other._hip, other._st32 = True, packed               # unpack path without a GPU
    other.sync_from_device()
    for k, v in ref.items():
        assert torch.equal(getattr(other, k), v), k


# ------------------------------------------------------------------------------------------------ DoomBasic
def test_basic_aligned_attack_kills_and_ends_the_episode():
    env = make("DoomBasic")
    env.mx[:], env.px[:] = 30, 30 - env.MON_HALF
    r, d, ep = act(env, 1)
    # the kill ends the episode at the first tic: one tic of living reward
    assert r.tolist() == [env.KILL + env.SHOT + env.LIVING] * 2 and d.all()
    assert ep.tolist() == [float(env.KILL + env.SHOT + env.LIVING)] * 2
    assert (env.tic == 0).all() and not env.killed.any()                       # auto-reset


def test_basic_missed_attack_costs_the_shot_and_cooldown_blocks_the_next():
    env = make("DoomBasic")
    env.mx[:], env.px[:] = 30, 30 - env.MON_HALF - 1
    fs = env.frameskip
    r, d, _ = act(env, 1)
    assert r.tolist() == [env.SHOT + fs * env.LIVING] * 2 and not d.any()
    assert (env.ammo == env.AMMO - 1).all()
    r, d, _ = act(env, 1)                                                      # tics 5..8: cooldown 4..1
    assert env.COOLDOWN == 2 * fs and r.tolist() == [fs * env.LIVING] * 2 and not d.any()
    r, d, _ = act(env, 1)                                                      # tic 9: ready again
    assert r.tolist() == [env.SHOT + fs * env.LIVING] * 2 and (env.ammo == env.AMMO - 2).all()


def test_basic_timeout_ends_the_episode_at_the_tables_tics():
    env = make("DoomBasic")
    env.mx[:] = env.XMAX                                                        # never hit: nobody shoots
    timeout = SCENARIOS["basic.cfg"]["episode_timeout"]
    steps = -(-timeout // env.frameskip)
    for i in range(steps):
        assert int(env.tic[0]) == i * env.frameskip
        r, d, ep = act(env, NOOP)
        assert bool(d[0]) == (i == steps - 1), i
    assert ep.tolist() == [float(timeout * env.LIVING)] * 2                     # no tic is played after the timeout


def test_basic_strafe_is_clamped_to_the_room():
    env = make("DoomBasic")
    env.mx[:] = 0
    for _ in range(10):
        act(env, 2)
    assert (env.px == env.XMAX).all()
    env.px[:] = -env.XMAX + 1
    act(env, 3)
    assert (env.px == -env.XMAX).all()


# ------------------------------------------------------------------------------------------------ DoomDefendCenter
def _dc(behind=True):
    env = make("DoomDefendCenter")
    if behind:
        env.ma[:] = 128                                                         # everyone behind the player
    return env


def test_defend_center_kill_pays_one_and_the_slot_respawns_at_the_rim():
    env = _dc()
    env.ma[:, 2] = 3                                                            # inside TOL0 of heading 0
    r, d, _ = act(env, 1)
    assert r.tolist() == [1, 1] and not d.any()
    assert not env.alive[:, 2].any() and env.alive[:, [0, 1, 3, 4]].all()
    assert (env.ammo == env.AMMO - 1).all()
    steps = env.RESPAWN // env.frameskip
    for i in range(1, steps):
        assert not env.alive[:, 2].any(), i
        act(env, NOOP)
    assert env.alive[:, 2].all() and (env.md[:, 2] == env.DMAX).all()
    assert (env.md[:, 0] == env.DMAX - env.RESPAWN).all()                       # the others kept walking


def test_defend_center_shot_takes_the_nearest_monster_in_tolerance():
    env = _dc()
    env.ma[:, 1], env.ma[:, 3] = 0, 0
    env.md[:, 1], env.md[:, 3] = 60, 40
    act(env, 1)
    assert env.alive[:, 1].all() and not env.alive[:, 3].any()
    # the tolerance widens as a monster gets closer
    env = _dc()
    off = env.TOL0 + 5
    env.ma[:, 0], env.ma[:, 1] = off, -off % 256
    env.md[:, 0], env.md[:, 1] = env.DMAX, env.DMAX - 5 * env.TOLDIV
    r, _, _ = act(env, 1)
    assert r.tolist() == [1, 1] and env.alive[:, 0].all() and not env.alive[:, 1].any()


def test_defend_center_ammo_runs_out_and_stops_the_firing():
    env = _dc()
    env.ammo[:] = 1
    env.ma[:, 0], env.ma[:, 1] = 0, 0
    r, d, _ = act(env, 1)
    assert r.tolist() == [1, 1] and (env.ammo == 0).all() and not d.any()       # the last round's cooldown runs
    r, d, _ = act(env, 1)
    assert r.tolist() == [0, 0] and (env.ammo == 0).all() and not d.any()
    assert not env.alive[:, 1].any() and env.alive[:, 0].all()               # the nearer one fell; 0 is in the sights
    r, d, ep = act(env, 1)                # cooldown over, a monster in the sights, ATTACK held: no shot, episode over
    assert r.tolist() == [0, 0] and d.all() and ep.tolist() == [1.0, 1.0]
    assert (env.ammo == env.AMMO).all()                                         # reset


def test_defend_center_bite_and_death_penalty():
    env = _dc()
    env.md[:, 4] = 0
    steps = env.BITE // env.frameskip
    for _ in range(steps):
        r, d, _ = act(env, NOOP)
    assert (env.health == env.HEALTH - env.DAMAGE).all() and r.tolist() == [0, 0]
    env.health[:] = env.DAMAGE
    for _ in range(steps):
        r, d, ep = act(env, NOOP)
    penalty = SCENARIOS["defend_the_center.cfg"]["death_penalty"]
    assert r.tolist() == [-penalty] * 2 and d.all() and ep.tolist() == [-float(penalty)] * 2
    assert (env.health == env.HEALTH).all()


def test_defend_center_heading_wraps_both_ways():
    env = _dc()
    turn = env.TURN * env.frameskip
    act(env, 3)                                                                 # TURN_LEFT
    assert (env.th == 256 - turn).all()
    act(env, 2)
    act(env, 2)                                                                 # TURN_RIGHT twice
    assert (env.th == turn).all()
    assert env.offsets(torch.tensor([[250, turn + 128, turn + 127]])).tolist() == [[-6 - turn, -128, 127]] * 2


# ------------------------------------------------------------------------------------------------ DoomTakeCover
def test_take_cover_fireball_hits_who_stays_and_misses_who_moved():
    env = make("DoomTakeCover")
    fs = env.frameskip
    for _ in range(env.FIRE // fs):
        act(env, NOOP)
    assert env.fact[:, 0].all() and (env.fz[:, 0] == dg.ZFAR).all()             # launched at tic FIRE, aimed at x = 0
    flight = dg.ZFAR // env.FSPEED
    a = torch.tensor([NOOP, 1])                                                 # env 1 strafes right
    for _ in range(flight // fs):
        assert (env.health == env.HEALTH).all()
        r, d, _ = env._advance(a)
    assert int(env.px[1]) == env.SPEED * flight > env.HIT_W
    assert env.health.tolist() == [env.HEALTH - env.DAMAGE, env.HEALTH] and not env.fact[:, 0].any()
    assert r.tolist() == [fs * env.LIVING] * 2 and not d.any()


def test_take_cover_fireball_is_aimed_at_the_players_x():
    env = make("DoomTakeCover")
    env.px[:] = 64
    for _ in range(env.FIRE // env.frameskip):
        act(env, NOOP)
    sx = env.fx[:, 0] // env.U
    flight = dg.ZFAR // env.FSPEED
    arrival = (env.fx[:, 0] + flight * env.fvx[:, 0]) // env.U
    assert (sx == env.SHOOTER_X[0]).all() and ((arrival - 64).abs() <= 1).all()
    assert (env.fvx[:, 0] > 0).all()


def test_take_cover_shooters_grow_with_tic_and_living_reward_is_per_tic():
    env = make("DoomTakeCover")
    assert env.shooters().tolist() == [1, 1]
    env.tic[:] = env.GROW - env.frameskip
    r, _, _ = act(env, NOOP)
    assert env.shooters().tolist() == [2, 2]
    assert r.tolist() == [env.frameskip * SCENARIOS["take_cover.cfg"]["living_reward"]] * 2
    env.tic[:] = 5 * env.GROW
    assert env.shooters().tolist() == [env.NSH] * 2
    env.tic[:] = SCENARIOS["take_cover.cfg"]["episode_timeout"] - 2             # two tics left: two living rewards
    r, d, _ = act(env, NOOP)
    assert r.tolist() == [2 * env.LIVING] * 2 and d.all()
    vis = env.scene().geometry()[:, 7:7 + env.NSH, 2] > 0
    assert vis.sum(1).tolist() == [1, 1]                                        # a fresh episode shows one shooter


def test_take_cover_death_ends_the_episode():
    env = make("DoomTakeCover")
    env.health[:] = env.DAMAGE
    done = torch.zeros(2, dtype=torch.bool)
    for _ in range((env.FIRE + dg.ZFAR // env.FSPEED) // env.frameskip):
        assert not done.any()
        _, done, ep = act(env, NOOP)
    assert done.all() and ep.tolist() == [float(env.FIRE + dg.ZFAR // env.FSPEED)] * 2


# ------------------------------------------------------------------------------------------------ scene
def _luma(c):
    return (c[0] * 4899 + c[1] * 9617 + c[2] * 1868 + 8192) >> 14


def test_colour_kinds_are_24_gray_levels_apart():
    kinds = [dg.CEIL, dg.SIDE, dg.FLOOR, dg.HUD, dg.WALL, dg.GUN, dg.PILLAR, dg.SHOOTER, dg.MONSTER, dg.FIREBALL]
    lum = sorted(_luma(c) for c in kinds)
    assert min(b - a for a, b in zip(lum, lum[1:])) >= 24, lum
    for bar in (dg.HBAR, dg.ABAR):                                              # the bars lie on the HUD strip only
        assert abs(_luma(bar) - _luma(dg.HUD)) >= 24


@pytest.mark.parametrize("name", NAMES)
def test_scene_coordinates_fit_int16_and_far_objects_are_3px_wide(name):
    env = GAMES[name](8, device="cpu", seed=9)
    env.max_episode_steps = 120
    env.reset()
    g = torch.Generator().manual_seed(4)
    nrect = len(env.scene().colors)
    assert nrect < 40
    bars = torch.tensor([c in (dg.HBAR, dg.ABAR) for c in env.scene().colors])
    lo, hi, wmin = 0, 0, 1 << 20
    for _ in range(300):
        env._advance(torch.randint(0, env.num_actions, (8,), generator=g))
        geo = env.scene().geometry()
        assert geo.shape == (8, nrect, 4)
        lo, hi = min(lo, int(geo.min())), max(hi, int(geo.max()))
        shown = (geo[..., 2] > 0) & ~bars[None]
        wmin = min(wmin, int(geo[..., 3][shown].min()))
    assert -2048 < lo and hi < 2048                                             # int16 with room to spare
    assert wmin >= 3
    # the farthest objects: at depth ZFAR every object kind is at least 3 px wide
    for w in (8, getattr(env, "MON_W", 8), getattr(env, "SH_W", 8), getattr(env, "FB_W", 8)):
        assert w * dg.K // (dg.ZFAR + dg.Z0) >= 3


@pytest.mark.parametrize("name", NAMES)
def test_view_moves_with_the_player_when_no_monster_is_in_view(name):
    """Two envs that differ only in the player's x (heading): the frames differ above the far objects' heads
    (rows 55..84 hold the far wall, its pillars and the side walls only)."""
    env = make(name)
    if name == "DoomDefendCenter":
        env.th[0], env.th[1] = 0, 12
        env.ma[0], env.ma[1] = 128, 140                                         # behind the player in both
        rows = slice(0, 210)
    else:
        env.px[0], env.px[1] = -env.XMAX, -env.XMAX + 16
        if name == "DoomBasic":
            env.mx[:] = env.XMAX                                                # off screen to the right
        rows = slice(dg.WALL_Y0, dg.HORIZON + dg.FH * dg.K // (dg.ZFAR + dg.Z0) - 40 * dg.K // (dg.ZFAR + dg.Z0))
    img = env.render()[:, rows]
    if name == "DoomBasic":
        geo = env.scene().geometry()[:, 7]
        assert (geo[:, 1] >= 160).all()                                         # the monster is out of view
    assert not torch.equal(img[0], img[1])
    gray = env.frame()
    assert not torch.equal(gray[0], gray[1])                                    # and the network sees it
    pillar = torch.tensor(dg.PILLAR, dtype=torch.uint8)
    assert (img == pillar).all(-1).any()


# ------------------------------------------------------------------------------------------------ experts
def _mean_return(name, policy, steps=400, n=8, seed=3):
    """Mean return per episode over ``steps`` agent steps (the running episodes included)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from calibrate_thresholds import EXPERTS
    env = GAMES[name](n, device="cpu", seed=seed)
    env.reset()
    g = torch.Generator().manual_seed(0)
    total, episodes = 0, n
    for _ in range(steps):
        a = torch.randint(0, env.num_actions, (n,), generator=g) if policy == "random" else EXPERTS[name](env)
        r, d, _ = env._advance(a)
        total += int(r.sum())
        episodes += int(d.sum())
    return total / episodes


# margins observed on the CPU (8 envs, seed 3, 400 agent steps; expert - random, mean return per episode):
#   DoomBasic        -31.9 - -1854.3 = 1822
#   DoomDefendCenter  9.62 -   0.21  = 9.4
#   DoomTakeCover     1600 -  145.5  = 1454 (the expert's episodes are still running after 400 steps)
# the test asserts half of each
@pytest.mark.parametrize("name,margin", [("DoomBasic", 1822.0), ("DoomDefendCenter", 9.4), ("DoomTakeCover", 1454.0)])
def test_expert_beats_random(name, margin):
    rand, expert = _mean_return(name, "random"), _mean_return(name, "expert")
    print(name, "random", rand, "expert", expert)
    assert expert > rand + margin / 2, (rand, expert)


# ------------------------------------------------------------------------------------------------ presets
def test_doom_presets_build_and_their_tasks_resolve():
    cfg = preset("doom3")
    assert cfg.tasks == ["DoomBasic", "DoomDefendCenter", "DoomTakeCover"]
    assert cfg.net.num_actions == 4 and cfg.net.num_tasks == 3
    ref = preset("atari4")
    assert (cfg.ga.fitness, cfg.net.trunk_scale) == (ref.ga.fitness, ref.net.trunk_scale)
    pong = preset("pong")
    assert [(l.kind, l.out, l.kernel, l.stride) for l in cfg.net.layers] == \
           [(l.kind, l.out, l.kernel, l.stride) for l in pong.net.layers]
    assert (cfg.net.L, cfg.net.M, cfg.net.N) == (pong.net.L, pong.net.M, pong.net.N)
    for task in cfg.tasks:
        env = registry.make(task, num_envs=1, frameskip=cfg.frameskip, gray=cfg.gray)
        assert env.num_actions <= cfg.net.num_actions and env.obs_shape == tuple(cfg.net.input_shape)
        assert env.reward_threshold == registry.reward_threshold(task) < float("inf")
    one = preset("doom-basic")
    assert one.tasks == ["DoomBasic"] and one.env == "DoomBasic" and one.net.num_tasks == 1
    assert one.net.num_actions == 4


def test_continual_script_accepts_the_doom_preset():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import argparse
    import continual
    args = argparse.Namespace(preset="doom3", paths=None, envs=None, tmax=None, N=4, trunk_scale=None, lr=None,
                              frozen_mode="or", frames=1000, seed=1, dtype=None, ring=False)
    cfg = continual.build_cfg(args, ["DoomBasic", "DoomTakeCover"])
    assert cfg.tasks == ["DoomBasic", "DoomTakeCover"] and cfg.net.num_tasks == 2 and cfg.net.num_actions == 4
