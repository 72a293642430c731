"""Free-view synthetic Doom scenarios (envs/doom_games.py: DoomDefendLine, DoomHealthGathering, DoomCorridor) on the
CPU: the integer trig and view transform, packed state, the games' rules, scene coordinates, palette, scripted
experts, presets, and the oracle run that the HIP comparison (tests/test_doom_nav_hip.py) replays."""
import argparse
import math
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
NAMES = ["DoomDefendLine", "DoomHealthGathering", "DoomCorridor"]
CFG = {"DoomDefendLine": "defend_the_line.cfg", "DoomHealthGathering": "health_gathering.cfg",
       "DoomCorridor": "deadly_corridor.cfg"}
NOOP = 0
U = dg.U


def make(name, n=2, seed=3):
    env = GAMES[name](n, device="cpu", seed=seed)
    env.reset()
    return env


def act(env, a):
    return env._advance(torch.full((env.num_envs,), a, dtype=torch.int64))


def hip_source():
    with open(os.path.join(ROOT, "csrc", "games.hip")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ trig table
def test_trig_table_is_the_rounded_sine_and_has_its_symmetries():
    assert list(dg.QSIN) == [round(256 * math.sin(2 * math.pi * i / 256)) for i in range(65)]
    env = make("DoomCorridor", n=1)
    h = torch.arange(-256, 512)
    s, c = env.isin(h), env.icos(h)
    full = [round(256 * math.sin(2 * math.pi * i / 256)) for i in range(256)]
    # the quarter-wave extension reproduces the rounded sine at all 256 headings (round() is odd-symmetric here:
    # no entry of the table is a half-integer before rounding except 0)
    assert s[256:512].tolist() == full
    assert torch.equal(s[:256], s[256:512]) and torch.equal(s[512:], s[256:512])                 # period
    assert torch.equal(env.isin(-h), -s)                                                        # odd
    assert torch.equal(env.icos(-h), c)                                                         # even
    assert torch.equal(env.isin(h + 128), -s) and torch.equal(env.isin(128 - h), s)             # half-wave, mirror
    assert torch.equal(c, env.isin(h + 64)) and torch.equal(env.icos(h + 64), -s)               # quarter shift
    assert int(s.abs().max()) == 256 and int(c.abs().max()) == 256


def test_hip_trig_table_is_the_python_table():
    src = hip_source()
    body = src[src.index("__constant__ int QSIN[65] = {"):]
    body = body[body.index("{") + 1:body.index("}")]
    assert [int(x) for x in body.replace("\n", " ").split(",")] == list(dg.QSIN)
    for banned in ("sinf", "cosf"):
        assert banned not in src


# ------------------------------------------------------------------------------------------------ constants
def constexpr_ints(text):
    out = {}
    for line in re.findall(r"static constexpr int ([^;]*);", text):
        for k, v in re.findall(r"(\w+) = (-?\d+)(?=,|$)", line):
            out[k] = int(v)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_hip_constants_mirror_the_python_classes(name):
    """Every literal ``static constexpr int`` of DoomNav and of the game's struct in csrc/games.hip equals the module
    or class constant of the same name; LIVING / DEATH_PENALTY / TIMEOUT are the scenario table's values."""
    src = hip_source()
    nav = src[src.index("struct DoomNav : DoomView {"):]
    body = src[src.index("struct %s : DoomNav {" % name):]
    env = make(name)
    shared = constexpr_ints(nav[:nav.index("\n};")])
    assert set(shared) == {"U", "ZVIEW", "COL", "DXMAX"}
    for k, v in shared.items():
        assert getattr(dg, k) == v, k
    own = constexpr_ints(body[:body.index("\n};")])
    assert len(own) >= 20
    for k, v in own.items():
        assert getattr(env, k) == v, (name, k)
    spec = SCENARIOS[CFG[name]]
    assert env.TIMEOUT == own["TIMEOUT"] == spec["episode_timeout"] == 2100
    assert env.DEATH_PENALTY == own["DEATH_PENALTY"] == spec["death_penalty"]
    assert env.LIVING == own.get("LIVING", 0) == spec.get("living_reward", 0)
    # every class constant that is a plain int is mirrored (the scenario's own and the driver's aside)
    mine = {k for k, v in vars(type(env)).items() if k.isupper() and isinstance(v, int)} - {"SCALE"}
    assert mine <= set(own), mine - set(own)


def test_hip_lane_and_group_positions_mirror_the_python_tuples():
    src = hip_source()
    a, b = re.search(r"lane_x\(int k\) \{ return (-?\d+) \+ (\d+) \* k; \}", src).groups()
    assert tuple(int(a) + int(b) * k for k in range(6)) == GAMES["DoomDefendLine"].LANE_X
    z = re.search(r"enemy_z\(int i\) \{ return i < 2 \? (\d+) : i < 4 \? (\d+) : (\d+); \}", src).groups()
    assert tuple(int(v) for v in z) == GAMES["DoomCorridor"].GROUP_Z


# ------------------------------------------------------------------------------------------------ registration
def test_games_are_registered_with_the_scenario_tables_constants():
    envs = []
    for name in NAMES:
        assert registry.is_synthetic(name) and registry.is_synthetic("Synth" + name + "-v0")
        for env_id in (name, "Synth" + name + "-v0"):
            env = registry.make(env_id, num_envs=1)
            assert isinstance(env, GAMES[name]) and env.HIP_GAME == name
        assert env.BUTTONS == SCENARIOS[CFG[name]]["buttons"]
        assert env.max_steps == 10000 and [f for f, _ in env.HIP_FIELDS]
        envs.append(env)
    assert [e.num_actions for e in envs] == [4, 4, 7]
    assert envs[0].BUTTONS == ["ATTACK", "TURN_RIGHT", "TURN_LEFT"]
    assert envs[1].BUTTONS == ["MOVE_FORWARD", "TURN_RIGHT", "TURN_LEFT"]
    assert envs[2].BUTTONS == ["ATTACK", "MOVE_RIGHT", "MOVE_LEFT", "MOVE_FORWARD", "TURN_RIGHT", "TURN_LEFT"]
    from pathnet_gym_amd.ops.envs import GAME_IDS
    assert [GAME_IDS[n] for n in NAMES] == [8, 9, 10]
    with pytest.raises(Exception) as ei:
        registry.make("gym_doom/DoomCorridor-v0")
    assert type(ei.value).__name__ == "DependencyNotInstalled"
    env = registry.make("DoomCorridor", num_envs=4)
    env.reset()
    obs, r, d, info = env.step(torch.tensor([0, 4, 5, 6]))
    assert obs.shape == (4, 160, 120, 4) and r.tolist() == [0.0, float(env.SPEED * env.frameskip), 0.0, 0.0]


@pytest.mark.parametrize("name", NAMES)
def test_state_pack_roundtrip(name):
    """HIP_FIELDS round-trips every state tensor after 40 random steps: signed th / px / kx, vec and mask fields."""
    env = GAMES[name](8, device="cpu", seed=5)
    env.reset()
    g = torch.Generator().manual_seed(0)
    neg = False
    for _ in range(40):
        env.step(torch.randint(0, env.num_actions, (8,), generator=g))
        neg |= any(bool((getattr(env, k) < 0).any()) for k, _ in env.HIP_FIELDS if getattr(env, k).dtype != torch.bool)
    kinds = {kind for _, kind in env.HIP_FIELDS}
    assert {"i", "mask"} <= kinds and (name == "DoomCorridor" or "vec" in kinds)
    assert neg                                           # every one of the three has a signed field in use
    ref = {k: getattr(env, k).clone() for k, _ in env._fields()}
    packed = env._hip_pack()
    other = GAMES[name](8, device="cpu", seed=5)
    other._hip, other._st32 = True, packed               # unpack path without a GPU
    other.sync_from_device()
    for k, v in ref.items():
        assert torch.equal(getattr(other, k), v), k


# ------------------------------------------------------------------------------------------------ view transform
def test_view_transform_at_the_four_quarter_headings():
    env = make("DoomCorridor", n=4)
    env.th[:] = torch.tensor([0, 64, 128, 192])
    pts = {"ahead": (0, 50), "right": (50, 0), "behind": (0, -50), "left": (-50, 0)}
    want = {  # heading -> where each world point lands in the view (dx, dz)
        0: {"ahead": (0, 50), "right": (50, 0), "behind": (0, -50), "left": (-50, 0)},
        64: {"ahead": (-50, 0), "right": (0, 50), "behind": (50, 0), "left": (0, -50)},
        128: {"ahead": (0, -50), "right": (-50, 0), "behind": (0, 50), "left": (50, 0)},
        192: {"ahead": (50, 0), "right": (0, -50), "behind": (-50, 0), "left": (0, 50)},
    }
    for key, (x, z) in pts.items():
        dx, dz = env.view(torch.full((4,), x * U), torch.full((4,), z * U))
        for i, h in enumerate((0, 64, 128, 192)):
            assert (int(dx[i]), int(dz[i])) == want[h][key], (h, key)
    # a forward step moves along the heading: +z at 0, +x at 64 (positive turns right)
    env = make("DoomHealthGathering", n=2)
    env.th[:] = torch.tensor([0, 64])
    act(env, 1)
    step = env.SPEED * env.frameskip * U
    assert env.px.tolist() == [0, step] and env.pz.tolist() == [step, 0]


def test_a_point_behind_the_player_is_not_drawn_and_fog_starts_past_zview():
    env = make("DoomCorridor", n=3)
    dz = torch.tensor([-1, dg.ZVIEW, dg.ZVIEW + 1])
    y0, x0, h, w, drawn = env.nav_project(torch.zeros(3, dtype=torch.int64), dz, 12, 12)
    assert drawn.tolist() == [False, True, False]
    assert int(w[1]) == 12 * dg.K // (dg.ZVIEW + dg.Z0) >= 3
    # in the scene: the vest behind the player (heading 128) has zero height, ahead and near it is shown
    env.pz[:] = (env.LEN - 100) * U
    env.th[:] = torch.tensor([0, 128, 64])
    vest = env.scene().geometry()[:, dg_rect(env, "vest")]
    assert (vest[0, 2] > 0) and vest[1, 2] == 0 and vest[2, 2] > 0      # at 64 the vest is at dz = 0, still drawn
    env.pz[:] = (env.LEN - dg.ZVIEW - 1) * U
    env.th[:] = 0
    assert (env.scene().geometry()[:, dg_rect(env, "vest"), 2] == 0).all()


def dg_rect(env, what):
    """Rectangle indices of a kind in the game's scene (the order of ``scene()``)."""
    n = env.id
    if n == "DoomDefendLine":
        base = {"posts": (3, env.NP), "enemies": (3 + env.NP, env.NM), "fireballs": (3 + env.NP + env.NM, env.NF)}
    elif n == "DoomHealthGathering":
        base = {"posts": (3, env.NP), "kits": (3 + env.NP, env.NK)}
    else:
        base = {"posts": (3, 2 * env.NPOST), "vest": (3 + 2 * env.NPOST, 1), "enemies": (4 + 2 * env.NPOST, env.NE)}
    a, k = base[what]
    return a if k == 1 else slice(a, a + k)


def test_view_transform_fits_int32_over_the_rooms_corners_and_all_headings():
    worst = 0
    for name in NAMES:
        env = GAMES[name](256, device="cpu", seed=0)
        env.reset()
        env.th[:] = torch.arange(256)
        if name == "DoomDefendLine":
            env.th[:] = torch.arange(256) % (2 * env.TH_MAX + 1) - env.TH_MAX
            spans = [(x, z) for x in (-2 * env.POST_GAP, 2 * env.POST_GAP, min(env.LANE_X), max(env.LANE_X))
                     for z in (0, env.DMAX)]
        elif name == "DoomHealthGathering":
            spans = [(2 * sx * env.ROOM * U, 2 * sz * env.ROOM * U) for sx in (-1, 1) for sz in (-1, 1)]
        else:
            spans = [(sx * 2 * env.HALFW * U, sz * (env.LEN + env.NPOST * env.POST_GAP) * U)
                     for sx in (-1, 1) for sz in (-1, 1)]
        s, c = env.isin(env.th), env.icos(env.th)
        for rx, rz in spans:
            for term in (rx * c, rz * s, rx * s, rz * c, rx * c - rz * s, rx * s + rz * c):
                assert term.dtype == torch.int64
                worst = max(worst, int(term.abs().max()))
            assert abs(rx) <= 1 << 15 and abs(rz) <= 1 << 15
    print("largest view-transform intermediate", worst)
    assert worst < 1 << 24 < 1 << 31                       # the bound written next to DoomNavVec.view, with room


# ------------------------------------------------------------------------------------------------ DoomDefendLine
def _dl(n=2):
    env = make("DoomDefendLine", n=n)
    env.md[:] = env.DMAX                                  # everyone back on the far line, heading 0
    return env


def test_defend_line_hit_scan_takes_the_nearest_covering_monster():
    env = _dl()
    # heading 0 looks between lanes 2 (x = -20) and 3 (x = +20): at the far line neither covers column 80
    assert (env.aim() == env.BIG).all()
    r, _, _ = act(env, 1)
    assert r.tolist() == [0, 0] and env.alive.all() and (env.cool > 0).all()     # the shot went off and hit nothing
    # close to the player both lanes' monsters cover the column: the nearer one is taken, a tie goes to the lower
    env = _dl()
    env.md[:, 2], env.md[:, 3] = 20, 12
    key = env.aim()
    assert (key % 8 == 3).all() and (key // 8 == 12).all()
    env.md[:, 2] = 12
    assert (env.aim() % 8 == 2).all()
    r, _, _ = act(env, 1)
    assert r.tolist() == [1, 1] and not env.alive[:, 2].any() and env.alive[:, 3].all()


def test_defend_line_kill_respawn_and_growing_hit_points():
    env = _dl()
    env.md[:, 2] = 12
    r, d, _ = act(env, 1)
    assert r.tolist() == [1, 1] and not d.any() and not env.alive[:, 2].any() and (env.mk[:, 2] == 1).all()
    steps = env.RESPAWN // env.frameskip
    for i in range(1, steps):
        assert not env.alive[:, 2].any(), i
        act(env, NOOP)
    assert env.alive[:, 2].all() and (env.md[:, 2] == env.DMAX).all() and (env.mhp[:, 2] == 2).all()
    # a monster with 2 hit points needs two shots, and the cooldown blocks the one in between
    env.md[:, 2] = 12
    r, _, _ = act(env, 1)
    assert r.tolist() == [0, 0] and (env.mhp[:, 2] == 1).all() and env.alive[:, 2].all()
    r, _, _ = act(env, 1)                                                     # tics 5..8 of the cooldown
    assert env.COOLDOWN == 2 * env.frameskip and r.tolist() == [0, 0] and (env.mhp[:, 2] == 1).all()
    r, _, _ = act(env, 1)
    assert r.tolist() == [1, 1] and not env.alive[:, 2].any() and (env.mk[:, 2] == 2).all()
    # hit points stop at HP_MAX
    env.mk[:, 2] = 7
    for _ in range(steps - 1):
        act(env, NOOP)
    assert env.alive[:, 2].all() and (env.mhp[:, 2] == env.HP_MAX).all()


def test_defend_line_bite_fireball_and_death():
    env = _dl()
    env.md[:, 0] = 1                                      # melee: at the player after one tic
    for _ in range(env.BITE // env.frameskip):
        r, d, _ = act(env, NOOP)
    assert (env.health == env.HEALTH - env.DAMAGE).all() and r.tolist() == [0, 0]
    # a shooter at its stand-off throws at tic % FIRE == 0 (shooter 1 has phase 0); the ball lands STANDOFF / FSPEED
    # tics later, whatever the player does
    env = _dl()
    env.md[:, 1] = env.STANDOFF
    for _ in range(env.FIRE // env.frameskip):
        act(env, NOOP)
    assert env.fact[:, 0].all() and (env.fd[:, 0] == env.STANDOFF).all() and not env.fact[:, 1:].any()
    assert (env.md[:, 1] == env.STANDOFF).all()                               # it does not come closer
    a = torch.tensor([2, 3])                                                   # turning does not dodge it
    for _ in range(env.STANDOFF // env.FSPEED // env.frameskip):
        assert (env.health == env.HEALTH).all()
        env._advance(a)
    assert (env.health == env.HEALTH - env.FDAMAGE).all() and not env.fact.any()
    # death pays -1 and ends the episode
    env = _dl()
    env.md[:, 0] = 0
    env.health[:] = env.DAMAGE
    for _ in range(env.BITE // env.frameskip):
        r, d, ep = act(env, NOOP)
    assert r.tolist() == [-1, -1] and d.all() and ep.tolist() == [-1.0, -1.0]
    assert (env.health == env.HEALTH).all() and (env.tic == 0).all()


def test_defend_line_heading_clamps():
    env = _dl()
    for _ in range(env.TH_MAX // (env.TURN * env.frameskip) + 2):
        act(env, 2)
    assert (env.th == env.TH_MAX).all()
    for _ in range(2 * env.TH_MAX // (env.TURN * env.frameskip) + 2):
        act(env, 3)
    assert (env.th == -env.TH_MAX).all()
    # at the clamp the outermost lane's monster on the far line can still be brought into the sights
    env = _dl()
    hit = False
    for _ in range(12):
        act(env, 3)
        hit |= bool(((env.aim() % 8 == 0) & (env.aim() < env.BIG)).all())
    assert hit


# ------------------------------------------------------------------------------------------------ DoomHealthGathering
def _hg(n=2):
    env = make("DoomHealthGathering", n=n)
    env.kact[:] = False
    env.th[:] = 0
    return env


def test_health_gathering_acid_living_reward_and_timeout():
    env = _hg()
    fs = env.frameskip
    for i in range(1, 3 * env.ACID // fs + 1):
        r, d, _ = act(env, NOOP)
        assert r.tolist() == [fs * env.LIVING] * 2 == [fs] * 2 and not d.any()
        assert (env.health == env.HEALTH - env.ACID_DMG * (i * fs // env.ACID)).all(), i
    env.health[:] = 10 ** 6                                                   # outlive the acid: the timeout ends it
    env.tic[:] = env.TIMEOUT - 2
    r, d, ep = act(env, NOOP)
    assert r.tolist() == [2, 2] and d.all() and SCENARIOS["health_gathering.cfg"]["episode_timeout"] == env.TIMEOUT


def test_health_gathering_pickup_heals_up_to_hmax_and_spawn_refills_the_lowest_slot():
    env = _hg()
    env.health[:] = torch.tensor([50, 90])
    env.kx[:, 5], env.kz[:, 5], env.kact[:, 5] = env.PICK, -env.PICK, True    # just inside the reach on both axes
    env.kx[:, 6], env.kz[:, 6], env.kact[:, 6] = env.PICK + 1, 0, True        # just outside
    act(env, NOOP)
    assert env.health.tolist() == [50 + env.HEAL, env.HMAX] and not env.kact[:, 5].any() and env.kact[:, 6].all()
    env = _hg()
    env.kact[:, 0] = True
    env.kx[:, 0] = env.kz[:, 0] = 80
    for _ in range(env.SPAWN // env.frameskip):
        assert env.kact.sum(1).tolist() == [1, 1]
        act(env, NOOP)
    assert env.kact[:, :2].all() and env.kact.sum(1).tolist() == [2, 2]      # slot 1: the lowest empty one
    assert (env.kx[:, 1].abs() <= env.KROOM).all() and (env.kz[:, 1].abs() <= env.KROOM).all()
    assert not torch.equal(env.kx[0, 1], env.kx[1, 1]) or not torch.equal(env.kz[0, 1], env.kz[1, 1])


def test_health_gathering_position_is_clamped_to_the_room():
    env = _hg()
    env.th[:] = torch.tensor([64, 128])                                       # walk +x, walk -z
    env.health[:] = 10 ** 6
    for _ in range(env.ROOM // (env.SPEED * env.frameskip) + 2):
        act(env, 1)
    assert env.px.tolist() == [env.ROOM * U, 0] and env.pz.tolist() == [0, -env.ROOM * U]


def test_health_gathering_death_pays_the_penalty():
    env = _hg()
    env.health[:] = env.ACID_DMG
    env.tic[:] = env.ACID - 2
    r, d, ep = act(env, NOOP)
    assert r.tolist() == [2 - 100, 2 - 100] and d.all() and env.DEATH_PENALTY == 100
    assert (env.health == env.HEALTH).all() and env.kact.sum(1).tolist() == [env.KIT0] * 2


# ------------------------------------------------------------------------------------------------ DoomCorridor
FWD, RIGHT, LEFT, TR, TL = 4, 2, 3, 5, 6


def _co(n=2):
    return make("DoomCorridor", n=n)


def test_corridor_progress_reward_telescopes():
    env = _co()
    step = env.SPEED * env.frameskip
    r, _, _ = act(env, FWD)
    assert r.tolist() == [step, step] and (env.pz == step * U).all()
    for a in (RIGHT, LEFT):                                                   # strafing at heading 0 pays nothing
        r, _, _ = act(env, a)
        assert r.tolist() == [0, 0]
    assert (env.px == 0).all()
    for _ in range(128 // (env.TURN * env.frameskip)):                        # turn round
        r, _, _ = act(env, TR)
        assert r.tolist() == [0, 0]
    assert (env.th == 128).all()
    r, _, _ = act(env, FWD)
    assert r.tolist() == [-step, -step] and (env.pz == 0).all()
    # over an episode of mixed play the rewards sum to the net whole-unit progress
    env = _co(n=8)
    env.alive[:] = False
    g = torch.Generator().manual_seed(1)
    total = torch.zeros(8, dtype=torch.int64)
    for _ in range(60):
        r, d, _ = env._advance(torch.randint(0, 7, (8,), generator=g))
        total += r
        assert not d.any()
    assert torch.equal(total, env.pz // U) and (total != 0).any() and (env.pz % U != 0).any()


def test_corridor_enemies_in_range_damage_at_their_tics_and_dead_ones_do_not():
    env = _co()
    env.pz[:] = (env.GROUP_Z[0] - env.RANGE) * U                              # pair 0 just in range, pair 1 not
    env.alive[1, :2] = False                                                  # env 1: both of the pair are dead
    hurt = torch.zeros(2, dtype=torch.int64)
    for i in range(env.EFIRE // env.frameskip):
        before = env.health.clone()
        tics = range(i * env.frameskip + 1, (i + 1) * env.frameskip + 1)
        due = sum(1 for t in tics for k in (0, 1) if (t + env.EPHASE * k) % env.EFIRE == 0)
        act(env, NOOP)
        lost = before - env.health
        assert int(lost[1]) == 0 and int(lost[0]) in {env.EDMG * j for j in range(due + 1)}, i
        hurt += lost
    assert int(hurt[0]) <= 2 * env.EDMG and (env.health[1] == env.HEALTH)
    # out of range nobody shoots; over many volleys about one shot in EMISS misses
    env = _co(n=64)
    env.pz[:] = (env.GROUP_Z[0] - env.RANGE - 1) * U
    for _ in range(10):
        act(env, NOOP)
    assert (env.health == env.HEALTH).all()
    env.pz[:] = env.GROUP_Z[0] * U
    env.health[:] = 10 ** 6
    for _ in range(5 * env.EFIRE // env.frameskip):
        act(env, NOOP)
    hits = (10 ** 6 - env.health).sum().item() // env.EDMG
    assert 0.6 * 640 < hits < 0.9 * 640, hits                                 # 64 envs x 2 enemies x 5 volleys


def test_corridor_shot_kills_the_enemy_in_the_sights_and_ammo_is_finite():
    env = _co()
    env.pz[:] = (env.GROUP_Z[0] - 60) * U
    env.px[:] = -env.ENEMY_X * U                                              # facing enemy 0 down its lane
    assert (env.aim() % 8 == 0).all() and (env.aim() // 8 == 60).all()
    r, _, _ = act(env, 1)
    assert not env.alive[:, 0].any() and env.alive[:, 1:].all() and (env.ammo == env.AMMO - 1).all()
    assert (env.aim() == env.BIG).all()                                       # enemy 2 is past ZVIEW: not drawn
    env.ammo[:] = 0
    env.px[:] = env.ENEMY_X * U
    assert (env.aim() % 8 == 1).all()
    for _ in range(3):
        act(env, 1)
    assert env.alive[:, 1].all() and (env.ammo == 0).all()


def test_corridor_vest_death_seventh_action_and_out_of_range_actions():
    env = _co()
    env.alive[:] = False
    env.pz[:] = (env.LEN - env.TOUCH - env.SPEED * env.frameskip) * U
    r, d, ep = act(env, FWD)
    assert d.all() and r.tolist() == [env.SPEED * env.frameskip] * 2           # no penalty, no bonus
    assert (env.pz == 0).all() and env.alive.all() and not env.won.any()
    env.pz[:] = (env.LEN - env.TOUCH) * U
    env.px[:] = (env.TOUCH + 1) * U                                            # beside the vest: not touching
    r, d, _ = act(env, NOOP)
    assert not d.any()
    # death pays -100
    env = _co()
    env.pz[:] = env.GROUP_Z[0] * U
    env.health[:] = 1
    d = torch.zeros(2, dtype=torch.bool)
    total = torch.zeros(2, dtype=torch.int64)
    for _ in range(3 * env.EFIRE // env.frameskip):
        r, d, _ = act(env, NOOP)
        total += r
        if d.all():
            break
    assert d.all() and total.tolist() == [-100, -100] == [-SCENARIOS["deadly_corridor.cfg"]["death_penalty"]] * 2
    # the 7th action (TURN_LEFT) is accepted; an action past the last or below 0 is a NOOP, as in the other games
    env = _co(n=3)
    env._advance(torch.tensor([6, 7, -1]))
    assert env.th.tolist() == [256 - env.TURN * env.frameskip, 0, 0] and (env.pz == 0).all() and (env.px == 0).all()


# ------------------------------------------------------------------------------------------------ scene
def _luma(c):
    return (c[0] * 4899 + c[1] * 9617 + c[2] * 1868 + 8192) >> 14


# the kinds that can overlap on screen in each game, as the module docstring lists them
OVERLAPS = {
    "DoomDefendLine": [("PILLAR", "CEIL"), ("PILLAR", "FLOOR"), ("PILLAR", "WALL"), ("MONSTER", "PILLAR"),
                       ("MONSTER", "CEIL"), ("MONSTER", "FLOOR"), ("MONSTER", "WALL"), ("FIREBALL", "MONSTER"),
                       ("FIREBALL", "PILLAR"), ("FIREBALL", "WALL"), ("FIREBALL", "FLOOR"), ("FIREBALL", "CEIL"),
                       ("GUN", "FLOOR"), ("GUN", "MONSTER"), ("GUN", "FIREBALL"), ("HBAR", "HUD")],
    "DoomHealthGathering": [("PILLAR", "CEIL"), ("PILLAR", "FLOOR"), ("PILLAR", "WALL"), ("KIT", "PILLAR"),
                            ("KIT", "FLOOR"), ("KIT", "WALL"), ("HBAR", "HUD")],
    "DoomCorridor": [("PILLAR", "CEIL"), ("PILLAR", "FLOOR"), ("PILLAR", "WALL"), ("VEST", "PILLAR"),
                     ("VEST", "FLOOR"), ("VEST", "WALL"), ("MONSTER", "VEST"), ("MONSTER", "PILLAR"),
                     ("MONSTER", "CEIL"), ("MONSTER", "FLOOR"), ("MONSTER", "WALL"), ("GUN", "FLOOR"),
                     ("GUN", "MONSTER"), ("GUN", "VEST"), ("HBAR", "HUD"), ("ABAR", "HUD")],
}


@pytest.mark.parametrize("name", NAMES)
def test_overlapping_kinds_are_24_gray_levels_apart(name):
    doc = dg.__doc__
    section = doc[doc.index("``%s``:" % name):]
    section = section[:section.index("\n\n")]
    for a, b in OVERLAPS[name]:
        assert abs(_luma(getattr(dg, a)) - _luma(getattr(dg, b))) >= 24, (a, b)
        assert "%s/%s" % (a, b) in section.replace("\n", " "), (name, a, b)   # and the docstring lists the pair
    used = {c for c in make(name).scene().colors}
    named = {getattr(dg, k) for pair in OVERLAPS[name] for k in pair}
    assert used <= named                                                      # no colour of the scene is left out


@pytest.mark.parametrize("name", NAMES)
def test_scene_is_fixed_size_in_range_and_far_objects_are_3px_wide(name):
    env = GAMES[name](8, device="cpu", seed=9)
    env.max_episode_steps = 120
    env.reset()
    g = torch.Generator().manual_seed(4)
    nrect = len(env.scene().colors)
    assert nrect < 40
    bars = torch.tensor([c in (dg.HBAR, dg.ABAR) for c in env.scene().colors])
    lo, hi, wmin, shown_n = 0, 0, 1 << 20, 0
    for _ in range(300):
        env._advance(torch.randint(0, env.num_actions, (8,), generator=g))
        geo = env.scene().geometry()
        assert geo.shape == (8, nrect, 4)
        lo, hi = min(lo, int(geo.min())), max(hi, int(geo.max()))
        shown = (geo[..., 2] > 0) & ~bars[None]
        wmin = min(wmin, int(geo[..., 3][shown].min()))
        shown_n += int(shown[:, 3:].sum())
    assert -2048 < lo and hi < 2048
    assert wmin >= 3 and shown_n > 300
    widths = [v for k, v in vars(type(env)).items() if k.endswith("_W")]
    assert len(widths) >= 2
    for w in widths:                                        # every object kind is at least 3 px wide at ZVIEW
        assert w * dg.K // (dg.ZVIEW + dg.Z0) >= 3
    # the extreme poses: every corner of the room at every eighth of a turn
    if name != "DoomDefendLine":
        xs = (-env.ROOM, env.ROOM) if name == "DoomHealthGathering" else (-env.HALFW, env.HALFW)
        zs = (-env.ROOM, env.ROOM) if name == "DoomHealthGathering" else (0, env.LEN)
        for x in xs:
            for z in zs:
                env.px[:], env.pz[:], env.th[:] = x * U, z * U, torch.arange(8) * 32
                geo = env.scene().geometry()
                assert -2048 < int(geo.min()) and int(geo.max()) < 2048


def test_an_object_beyond_zview_has_zero_height():
    env = make("DoomHealthGathering")
    env.th[:] = 0
    env.kact[:] = False
    env.kact[:, 0] = env.kact[:, 1] = True
    env.kx[:, 0], env.kz[:, 0] = 0, dg.ZVIEW - env.ROOM                       # from z = -ROOM: exactly at ZVIEW
    env.kx[:, 1], env.kz[:, 1] = 0, dg.ZVIEW - env.ROOM + 1
    env.pz[:] = -env.ROOM * U
    kits = env.scene().geometry()[:, dg_rect(env, "kits")]
    assert (kits[:, 0, 2] > 0).all() and (kits[:, 0, 3] >= 3).all() and (kits[:, 1:, 2] == 0).all()
    env = _dl()
    assert (env.scene().geometry()[:, dg_rect(env, "enemies"), 2] > 0).all()  # the far line is inside the view


@pytest.mark.parametrize("name", NAMES)
def test_view_moves_with_heading_and_position(name):
    """Two envs that differ only in heading, or only in position, render differently, with nothing but the posts
    (and the vest) in view."""
    env = make(name, n=3)
    if name == "DoomDefendLine":
        env.alive[:] = False
        env.th[:] = torch.tensor([0, 8, 0])
    elif name == "DoomHealthGathering":
        env.kact[:] = False
        env.th[:] = torch.tensor([0, 8, 0])
        env.pz[2] = 24 * U
    else:
        env.alive[:] = False
        env.th[:] = torch.tensor([0, 8, 0])
        env.pz[2] = 12 * U
    img, gray = env.render(), env.frame()
    assert not torch.equal(img[0], img[1]) and not torch.equal(gray[0], gray[1])
    if name != "DoomDefendLine":                                               # DefendLine's player does not move
        assert not torch.equal(img[0], img[2]) and not torch.equal(gray[0], gray[2])
    pillar = torch.tensor(dg.PILLAR, dtype=torch.uint8)
    assert (img == pillar).all(-1).any()


# ------------------------------------------------------------------------------------------------ experts
def _mean_return(name, policy, steps=400, n=8, seed=3):
    """Mean return per episode over ``steps`` agent steps (the running episodes included)."""
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
#   DoomDefendLine      12.41 -   3.31 = 9.1
#   DoomHealthGathering  1600 -  138.6 = 1461 (the expert's episodes are still running after 400 steps)
#   DoomCorridor        807.2 -  106.9 = 700
# the test asserts half of each
@pytest.mark.parametrize("name,margin", [("DoomDefendLine", 9.1), ("DoomHealthGathering", 1461.0),
                                         ("DoomCorridor", 700.0)])
def test_expert_beats_random(name, margin):
    rand, expert = _mean_return(name, "random"), _mean_return(name, "expert")
    print(name, "random", rand, "expert", expert)
    assert margin > 0 and expert > rand + margin / 2, (rand, expert)


# ------------------------------------------------------------------------------------------------ presets
def _shape(cfg):
    return [(l.kind, l.out, l.kernel, l.stride) for l in cfg.net.layers], (cfg.net.L, cfg.net.M, cfg.net.N)


def test_doom6_and_the_single_task_presets():
    cfg, ref, pong = preset("doom6"), preset("doom3"), preset("pong")
    assert cfg.tasks == ["DoomBasic", "DoomCorridor", "DoomDefendCenter", "DoomDefendLine", "DoomHealthGathering",
                         "DoomTakeCover"]
    assert cfg.tasks == [n for n in dg.LEVEL_NAMES if n in dg.DOOM_GAMES]    # the curriculum's order
    assert cfg.net.num_actions == 7 and cfg.net.num_tasks == 6
    assert _shape(cfg) == _shape(pong) == _shape(ref)
    # otherwise identical to doom3
    a, b = vars(cfg).copy(), vars(ref).copy()
    for d in (a, b):
        for k in ("tasks", "net"):
            d.pop(k)
    assert a == b
    na, nb = vars(cfg.net).copy(), vars(ref.net).copy()
    for d in (na, nb):
        for k in ("num_actions", "num_tasks"):
            d.pop(k)
    assert na == nb
    for task in cfg.tasks:
        env = registry.make(task, num_envs=1, frameskip=cfg.frameskip, gray=cfg.gray)
        assert env.num_actions <= cfg.net.num_actions == 7 and env.obs_shape == tuple(cfg.net.input_shape)
        assert env.reward_threshold == registry.reward_threshold(task) < float("inf")
    for name, task, na in (("doom-corridor", "DoomCorridor", 7), ("doom-defend-line", "DoomDefendLine", 4),
                           ("doom-health", "DoomHealthGathering", 4)):
        one = preset(name)
        assert one.tasks == [task] and one.env == task and one.net.num_tasks == 1 and one.net.num_actions == na
        assert _shape(one) == _shape(pong)
        assert registry.make(one.env, num_envs=1).num_actions == na
    # doom3 and doom-basic are what they were
    assert ref.tasks == ["DoomBasic", "DoomDefendCenter", "DoomTakeCover"]
    assert ref.net.num_actions == 4 and ref.net.num_tasks == 3
    basic = preset("doom-basic")
    assert basic.tasks == ["DoomBasic"] and basic.net.num_actions == 4 and basic.net.num_tasks == 1


def test_continual_script_and_cli_accept_doom6():
    import continual
    args = argparse.Namespace(preset="doom6", paths=None, envs=None, tmax=None, N=4, trunk_scale=None, lr=None,
                              frozen_mode="or", frames=1000, seed=1, dtype=None, ring=False)
    cfg = continual.build_cfg(args, preset("doom6").tasks)
    assert len(cfg.tasks) == 6 and cfg.net.num_tasks == 6 and cfg.net.num_actions == 7
    from pathnet_gym_amd.cli import build_parser
    text = build_parser()._subparsers._group_actions[0].choices["train"].format_help()
    text = re.sub(r"-\s*\n\s*", "-", text)                 # argparse wraps the list at hyphens
    for name in ("doom6", "doom-corridor", "doom-defend-line", "doom-health"):
        assert name in text, name


def test_thresholds_are_the_calibration_scripts_records():
    import json
    with open(os.path.join(ROOT, "pathnet_gym_amd", "envs", "thresholds.json")) as f:
        games = json.load(f)["games"]
    for name in NAMES:
        rec = games[name]
        want = rec["random"]["mean_return"] + 0.75 * (rec["expert"]["mean_return"] - rec["random"]["mean_return"])
        assert rec["fraction"] == 0.75 and rec["threshold"] == round(want, 1)
        assert rec["random"]["mean_return"] < rec["threshold"] <= rec["expert"]["mean_return"]
        assert rec["random"]["episodes"] == rec["expert"]["episodes"] == 128      # 64 envs, 2 episodes each
    # HealthGathering: the random policy dies well before the timeout, the expert survives much longer
    hg = games["DoomHealthGathering"]
    assert hg["random"]["mean_return"] < 2100 / 4 and hg["expert"]["mean_return"] > 3 * hg["random"]["mean_return"]


# ------------------------------------------------------------------------------------------------ the oracle run
SEED, ACTION_SEED = 11, 3
# the play of the bit-exact comparison: N = 96 envs, 300 agent steps, episodes capped at 60 steps.  Env i follows the
# scripted expert of scripts/calibrate_thresholds.py (read from the oracle's state) when i % 4 == 0, and uniform
# random actions otherwise.  DoomCorridor alone also starts late in a quarter of the envs, once, after the first
# reset: no policy walks 1000 units in 60 steps.  Env i with i % 8 == 0 (an expert) starts at z = 600 with the first
# two pairs dead, so it fights the last pair and reaches the vest; env i with i % 8 == 1 (random) starts at z = 600
# between two living pairs, so it is shot dead.
EXPERT_EVERY = 4
LATE_Z = 600


def _state(env):
    return {name: getattr(env, name).clone() for name, _ in env._fields()}


def late_start(env):
    """DoomCorridor's late state, written into the torch state and, for a HIP env, into the kernel's rows."""
    env.sync_from_device()
    i = torch.arange(env.num_envs, device=env.device)
    late = (i % 8) <= 1
    env.pz.copy_(torch.where(late, torch.full_like(env.pz, LATE_Z * U), env.pz))
    env.alive[:, :4] &= ~(i % 8 == 0)[:, None]
    if env._hip:
        env._st32.copy_(env._hip_pack())


class Events:
    """Counts, from the torch oracle's state before and after a step, the events that make each game."""

    def __init__(self, env, cap):
        self.env, self.cap = env, cap
        self.count = {}
        self.snap()

    def snap(self):
        self.prev = _state(self.env)

    def add(self, key, n):
        self.count[key] = self.count.get(key, 0) + int(n)

    def step(self, reward, done):
        e, p = self.env, self.prev
        run = ~done                                            # a finished env shows the next episode's state
        ended = done & (p["steps"] + 1 < self.cap)             # by the game, not by the cap (the tic timeout is far)
        hurt = run & (e.health < p["health"])
        if e.id == "DoomDefendLine":
            kill = run[:, None] & (e.mk > p["mk"])
            self.add("kill", kill.sum())
            self.add("multi_hit_kill", (kill & (p["mk"] >= 1)).sum())      # it had come back with 2 or 3 hit points
            self.add("respawn_tougher", (run[:, None] & ~p["alive"] & e.alive & (e.mhp >= 2)).sum())
            self.add("bite", (hurt & (e.alive & ~e.is_sh & (e.md == 0)).any(1)).sum())
            self.add("fireball_hit", (run[:, None] & p["fact"] & ~e.fact).sum())
            self.add("death", ended.sum())
        elif e.id == "DoomHealthGathering":
            self.add("pickup", (run[:, None] & p["kact"] & ~e.kact).sum())
            self.add("kit_spawn", (run[:, None] & ~p["kact"] & e.kact).sum())
            self.add("acid", hurt.sum())
            self.add("death", ended.sum())
            lim = e.ROOM * U
            self.add("wall_clamp", (run & ((e.px.abs() == lim) | (e.pz.abs() == lim))).sum())
        else:
            self.add("enemy_kill", (run[:, None] & p["alive"] & ~e.alive).sum())
            self.add("damage", hurt.sum())
            self.add("death", (ended & (reward < 0)).sum())
            self.add("vest", (ended & (reward >= 0)).sum())
            self.add("retreat", (reward < 0).sum() - (ended & (reward < 0)).sum())
        self.snap()


def play(name, device, hip, N=96, steps=300, cap=60):
    """The oracle (and, with ``hip``, the HIP env next to it, compared at every step) under the play described
    above; returns both envs and the oracle's event counts."""
    from calibrate_thresholds import EXPERTS
    et = GAMES[name](N, device=device, seed=SEED, backend="torch")
    eh = GAMES[name](N, device=device, seed=SEED, backend="hip") if hip else None
    envs = [e for e in (et, eh) if e is not None]
    if hip:
        assert eh._hip and not et._hip
    for e in envs:
        e.max_episode_steps = cap                      # time-limit resets on top of the games' own endings
    obs = [e.reset() for e in envs]
    assert all(torch.equal(obs[0], o) for o in obs)
    if name == "DoomCorridor":
        for e in envs:
            late_start(e)
    ev = Events(et, cap)
    g = torch.Generator().manual_seed(ACTION_SEED)
    expert = (torch.arange(N) % EXPERT_EVERY == 0).to(device)
    ndone = 0
    for i in range(steps):
        a = torch.randint(0, et.num_actions, (N,), generator=g).to(device)
        a = torch.where(expert, EXPERTS[name](et), a)
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


# what the oracle alone shows on the CPU with these seeds
EXPECTED = {
    "DoomDefendLine": {"kill": 4136, "multi_hit_kill": 1322, "respawn_tougher": 3887, "bite": 2865,
                       "fireball_hit": 7882, "death": 585, "done": 661},
    "DoomHealthGathering": {"pickup": 1165, "kit_spawn": 2657, "acid": 6488, "death": 211, "wall_clamp": 7083,
                            "done": 480},
    "DoomCorridor": {"enemy_kill": 569, "damage": 1462, "death": 14, "vest": 12, "retreat": 2800, "done": 480},
}
NEEDED = {"DoomDefendLine": ("kill", "multi_hit_kill", "respawn_tougher", "bite", "fireball_hit", "death"),
          "DoomHealthGathering": ("pickup", "acid", "kit_spawn", "death", "wall_clamp"),
          "DoomCorridor": ("enemy_kill", "damage", "death", "retreat", "vest")}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_run_contains_the_games_events(name):
    """CPU: the seeds and the action mix of the bit-exact comparison give a run with every event of the game."""
    _, _, count = play(name, "cpu", hip=False)
    print(name, count)
    for k in NEEDED[name]:
        assert count[k] >= 1, (k, count)
    assert count == EXPECTED[name]
