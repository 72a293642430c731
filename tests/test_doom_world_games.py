"""The last three synthetic Doom levels (envs/doom_world_games.py: DoomMyWayHome, DoomPredictPosition,
DoomDeathmatch) on the CPU: the games' rules, the map and its regions, the view transform's bound, palette and scene,
scripted experts, thresholds, presets, and the oracle run that the HIP comparison (tests/test_doom_world_hip.py)
replays."""
import argparse
import json
import os
import re
import sys

import pytest
import torch

from pathnet_gym_amd.config import preset
from pathnet_gym_amd.envs import doom_games as dg
from pathnet_gym_amd.envs import doom_world_games as dw
from pathnet_gym_amd.envs import registry
from pathnet_gym_amd.envs.atari_games import GAMES
from pathnet_gym_amd.envs.doom.constants import ACTION_CONFIGS, BUTTONS, LEVEL_NAMES
from pathnet_gym_amd.envs.doom.scenarios import SCENARIOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
NAMES = ["DoomMyWayHome", "DoomPredictPosition", "DoomDeathmatch"]
CFG = {"DoomMyWayHome": "my_way_home.cfg", "DoomPredictPosition": "predict_position.cfg",
       "DoomDeathmatch": "deathmatch.cfg"}
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


def struct_body(name):
    src = hip_source()
    body = src[src.index("struct %s : DoomNav {" % name):]
    return body[:body.index("\n};")]


def constexpr_ints(text):
    out = {}
    for line in re.findall(r"static constexpr int ([^;]*);", text):
        for k, v in re.findall(r"(\w+) = (-?\d+)(?=,|$)", line):
            out[k] = int(v)
    return out


# ------------------------------------------------------------------------------------------------ constants
@pytest.mark.parametrize("name", NAMES)
def test_hip_constants_mirror_the_python_classes(name):
    body = struct_body(name)
    env = make(name)
    own = constexpr_ints(body)
    assert len(own) >= 15
    for k, v in own.items():
        assert getattr(env, k) == v, (name, k)
    mine = {k for k, v in vars(type(env)).items() if k.isupper() and isinstance(v, int)}
    assert mine <= set(own), mine - set(own)
    spec = SCENARIOS[CFG[name]]
    assert env.TIMEOUT == own["TIMEOUT"] == spec["episode_timeout"] == {"DoomMyWayHome": 2100,
                                                                        "DoomPredictPosition": 700,
                                                                        "DoomDeathmatch": 6300}[name]
    assert env.DEATH_PENALTY == 0 == spec.get("death_penalty", 0) and "DEATH_PENALTY" not in own
    assert env.LIVING == 0 and "LIVING" not in own
    # the declared number of rectangles is the scene's, at most 40
    expr = re.search(r"static constexpr int R = ([^;]*);", body).group(1)
    assert eval(expr, {}, dict(own, NBACK=3)) == len(env.scene().colors) <= 40


def test_hip_region_table_is_the_python_table():
    body = struct_body("DoomMyWayHome")
    env = GAMES["DoomMyWayHome"]
    for k in ("X0", "Z0R", "X1", "Z1R", "DOORS", "MARKS"):
        vals = re.search(r"constexpr int %s\[NR\] = \{([^}]*)\};" % k, body).group(1)
        assert tuple(int(v) for v in vals.split(",")) == getattr(env, k), k
        assert len(getattr(env, k)) == env.NR


def test_living_reward_rounds_to_zero_and_the_old_levels_are_untouched():
    for name in NAMES[:2]:
        assert SCENARIOS[CFG[name]]["living_reward"] == -0.0001
        assert dw.world_scenario(name)[0] == 0
        with pytest.raises(AssertionError):
            dg.scenario(name)                                # the six levels' reader still refuses a fraction
    want = {"DoomBasic": (-10, 0, 350), "DoomCorridor": (0, 100, 2100), "DoomDefendCenter": (0, 1, 2100),
            "DoomDefendLine": (0, 1, 2100), "DoomHealthGathering": (1, 100, 2100), "DoomTakeCover": (1, 0, 2100)}
    for name, v in want.items():
        assert dg.scenario(name)[:3] == v
    # DoomDeathmatch plays constant-7, a subset of the level's 42 buttons
    living, death, timeout, buttons = dw.world_scenario("DoomDeathmatch")
    assert (living, death, timeout) == (0, 0, 6300)
    assert buttons == [BUTTONS[i] for i in ACTION_CONFIGS["constant-7"]] == [
        "ATTACK", "MOVE_RIGHT", "MOVE_LEFT", "MOVE_FORWARD", "TURN_RIGHT", "TURN_LEFT", "SELECT_NEXT_WEAPON"]
    assert set(buttons) <= {b.replace("ALTATTACK", "ALT_ATTACK") for b in SCENARIOS["deathmatch.cfg"]["buttons"]}


def test_games_are_registered_in_their_own_dict():
    assert list(dw.DOOM_WORLD_GAMES) == NAMES and len(dg.DOOM_GAMES) == 6
    assert not set(NAMES) & set(dg.DOOM_GAMES)
    assert [n for n in LEVEL_NAMES if n in dg.DOOM_GAMES or n in dw.DOOM_WORLD_GAMES] == LEVEL_NAMES
    envs = []
    for name in NAMES:
        assert registry.is_synthetic(name) and registry.is_synthetic("Synth" + name + "-v0")
        for env_id in (name, "Synth" + name + "-v0"):
            env = registry.make(env_id, num_envs=1)
            assert isinstance(env, GAMES[name]) and env.HIP_GAME == name
        envs.append(env)
    assert [e.num_actions for e in envs] == [4, 4, 8]
    assert envs[0].BUTTONS == ["MOVE_FORWARD", "TURN_RIGHT", "TURN_LEFT"]
    assert envs[1].BUTTONS == ["ATTACK", "TURN_RIGHT", "TURN_LEFT"]
    from pathnet_gym_amd.ops.envs import GAME_IDS
    assert [GAME_IDS[n] for n in NAMES] == [12, 13, 14] and 11 not in GAME_IDS.values()
    from pathnet_gym_amd.runtime.evaluator import unsupported_reason
    for name in NAMES:
        for env_id in (name, "Synth" + name + "-v0"):
            assert unsupported_reason(preset("doom9").net, env_id, "fp32x", 16) is None


@pytest.mark.parametrize("name", NAMES)
def test_state_pack_roundtrip(name):
    env = GAMES[name](8, device="cpu", seed=5)
    env.reset()
    g = torch.Generator().manual_seed(0)
    for _ in range(40):
        env.step(torch.randint(0, env.num_actions, (8,), generator=g))
    ref = {k: getattr(env, k).clone() for k, _ in env._fields()}
    packed = env._hip_pack()
    other = GAMES[name](8, device="cpu", seed=5)
    other._hip, other._st32 = True, packed               # unpack path without a GPU
    other.sync_from_device()
    for k, v in ref.items():
        assert torch.equal(getattr(other, k), v), k


# ------------------------------------------------------------------------------------------------ DoomMyWayHome
FWD = 1


def _mw(n=2):
    return make("DoomMyWayHome", n=n)


def _place(env, x, z, th):
    env.px[:], env.pz[:], env.th[:] = x * U, z * U, th


def test_my_way_home_regions_tile_and_membership_at_the_thresholds():
    env = _mw(n=1)
    pt = lambda x, z: int(env.region_of(torch.tensor([x]), torch.tensor([z]))[0])      # noqa: E731  sub-units
    # the doorway between rooms A and B: x in [128, 144), z in [48, 80)
    assert pt(128 * U - 1, 64 * U) == 0 and pt(128 * U, 64 * U) == 6
    assert pt(144 * U - 1, 64 * U) == 6 and pt(144 * U, 64 * U) == 1
    assert pt(128 * U, 48 * U - 1) == -1 and pt(128 * U, 48 * U) == 6
    assert pt(128 * U, 80 * U - 1) == 6 and pt(128 * U, 80 * U) == -1
    # the doorway between A and D runs along z
    assert pt(64 * U, 128 * U - 1) == 0 and pt(64 * U, 128 * U) == 8 and pt(64 * U, 144 * U) == 3
    assert pt(48 * U - 1, 130 * U) == -1 and pt(80 * U, 130 * U) == -1
    # the corridor off room C ends dead
    assert pt(352 * U, 128 * U - 1) == 2 and pt(352 * U, 128 * U) == 5 and pt(352 * U, 272 * U - 1) == 5
    assert pt(352 * U, 272 * U) == -1 and pt(336 * U - 1, 200 * U) == -1 and pt(368 * U, 200 * U) == -1
    assert pt(-1, 0) == -1 and pt(0, 0) == 0 and pt(0, -1) == -1
    # no two regions overlap: every point of a 4-unit grid lies in at most one
    xs, zs = torch.meshgrid(torch.arange(-8, 432, 4), torch.arange(-8, 288, 4), indexing="ij")
    x, z = xs.reshape(-1) * U, zs.reshape(-1) * U
    holds = sum(((x >= env.X0[k] * U) & (x < env.X1[k] * U) & (z >= env.Z0R[k] * U) & (z < env.Z1R[k] * U)).long()
                for k in range(env.NR))
    assert int(holds.max()) == 1 and int((holds == 0).sum()) > 0
    # every door opening leads, through the middle of its wall, into a region that has the door facing back
    for k in range(env.NR):
        xm, zm = (env.X0[k] + env.X1[k]) // 2, (env.Z0R[k] + env.Z1R[k]) // 2
        beyond = ((xm, env.Z1R[k]), (env.X1[k], zm), (xm, env.Z0R[k] - 1), (env.X0[k] - 1, zm))
        for j, (bx, bz) in enumerate(beyond):
            other = pt(bx * U, bz * U)
            if (env.DOORS[k] >> j) & 1:
                assert other >= 0 and other != k and (env.DOORS[other] >> ((j + 2) % 4)) & 1, (k, j)
            else:
                assert other == -1, (k, j)
    # the rooms' marker patterns differ from each other
    assert len({env.MARKS[k] for k in range(env.NROOMS)}) == env.NROOMS and env.WALL_T == env.X0[6] + 16 - env.X1[0]


def test_my_way_home_walls_block_and_doors_pass():
    env = _mw()
    _place(env, 120, 20, 64)                              # room A, walking +x at the east wall, away from the door
    for _ in range(3):
        r, d, _ = act(env, FWD)
    assert (env.px == (128 - env.SPEED) * U).all() and (env.pz == 20 * U).all()      # the last whole step that fits
    assert (env.region_of(env.px, env.pz) == 0).all()
    # a diagonal walk slides along the wall: x stays, z goes on
    _place(env, 126, 20, 32)
    z0 = env.pz.clone()
    act(env, FWD)
    assert (env.px < 128 * U).all() and (env.pz > z0).all()
    # through the door in the middle of the wall: room A, the doorway, room B
    _place(env, 120, 64, 64)
    seen = []
    for _ in range(3):
        act(env, FWD)
        seen.append(int(env.region_of(env.px, env.pz)[0]))
    assert seen == [6, 1, 1] and (env.px == (120 + 3 * 4 * env.SPEED) * U).all()
    # the map's outer wall and the dead end
    _place(env, 352, 268, 0)
    for _ in range(3):
        act(env, FWD)
    assert (env.pz < 272 * U).all() and (env.region_of(env.px, env.pz) == 5).all()
    # turning moves nothing
    p = (env.px.clone(), env.pz.clone())
    act(env, 2)
    assert torch.equal(env.px, p[0]) and torch.equal(env.pz, p[1]) and (env.th == 4 * env.TURN).all()


def test_my_way_home_vest_pays_once_and_timeout_ends():
    env = _mw()
    _place(env, env.VEST_X, env.VEST_Z - env.TOUCH - 4 * env.SPEED, 0)
    assert (env.region_of(env.px, env.pz) == env.VEST_ROOM).all()
    r, d, ep = act(env, FWD)
    assert r.tolist() == [1, 1] and d.all() and ep.tolist() == [1.0, 1.0]       # +1 on the touching tic only
    room = env.region_of(env.px, env.pz)
    assert ((room >= 0) & (room < env.NSTART)).all() and (env.tic == 0).all() and not env.won.any()
    # just outside the reach nothing happens
    _place(env, env.VEST_X + env.TOUCH + 1, env.VEST_Z, 0)
    r, d, _ = act(env, NOOP)
    assert r.tolist() == [0, 0] and not d.any()
    env.tic[:] = env.TIMEOUT - 2
    r, d, ep = act(env, NOOP)
    assert r.tolist() == [0, 0] and d.all() and ep.tolist() == [0.0, 0.0]


def test_my_way_home_starts_are_spread_over_the_start_rooms():
    env = GAMES["DoomMyWayHome"](256, device="cpu", seed=1)
    env.reset()
    room = env.region_of(env.px, env.pz)
    assert sorted(set(room.tolist())) == [0, 1, 2, 3]
    wx, wz = env.px // U, env.pz // U
    assert ((wx - env.rx0[room] >= env.MARGIN) & (env.rx1[room] - wx > env.MARGIN)).all()
    assert ((wz - env.rz0[room] >= env.MARGIN) & (env.rz1[room] - wz > env.MARGIN)).all()
    assert len(set(env.th.tolist())) > 64 and (env.px % U == 0).all()


def test_view_transform_fits_int32_over_the_whole_map():
    env = GAMES["DoomMyWayHome"](256, device="cpu", seed=0)
    env.reset()
    env.th[:] = torch.arange(256)
    s, c = env.isin(env.th), env.icos(env.th)
    w, h = max(env.X1) - min(env.X0), max(env.Z1R) - min(env.Z0R)
    assert (w, h) == (416, 272)
    worst = 0
    for rx in (-w * U, w * U):
        for rz in (-h * U, h * U):
            assert abs(rx) <= 1 << 14 and abs(rz) <= 1 << 14          # the bound stated in DoomNav::view
            for term in (rx * c, rz * s, rx * s, rz * c, rx * c - rz * s, rx * s + rz * c):
                worst = max(worst, int(term.abs().max()))
    print("largest view-transform intermediate", worst)
    assert worst <= 1 << 23 < 1 << 31


def test_my_way_home_draws_only_the_players_region():
    env = GAMES["DoomMyWayHome"](16, device="cpu", seed=0)
    env.reset()
    head = torch.arange(16) * 16
    d0, p0, v = 3, 3 + env.ND, 3 + env.ND + env.NP
    n_in, seen_vest = 0, False
    for x in range(2, 416, 12):
        for z in range(2, 272, 12):
            r = int(env.region_of(torch.tensor([x * U]), torch.tensor([z * U]))[0])
            if r < 0:
                continue
            n_in += 1
            _place(env, x, z, head)
            geo = env.scene().geometry()
            doors, marks = geo[:, d0:d0 + env.ND, 2] > 0, geo[:, p0 + 4:p0 + 8, 2] > 0
            for j in range(4):
                assert not doors[:, j].any() or (env.DOORS[r] >> j) & 1, (x, z, j)
                assert not marks[:, j].any() or (env.MARKS[r] >> j) & 1, (x, z, j)
            vest = geo[:, v, 2] > 0
            assert r == env.VEST_ROOM or not vest.any(), (x, z)      # the vest's room is two doors away at least
            seen_vest |= bool(vest.any())
    assert n_in > 300 and seen_vest
    # from the middle of a region, all its doors, posts and markers come into view over a turn, and nothing else
    for r in range(env.NR):
        _place(env, (env.X0[r] + env.X1[r]) // 2, (env.Z0R[r] + env.Z1R[r]) // 2, head)
        geo = env.scene().geometry()
        doors = (geo[:, d0:d0 + env.ND, 2] > 0).any(0).tolist()
        posts = (geo[:, p0:p0 + env.NP, 2] > 0).any(0).tolist()
        assert doors == [bool((env.DOORS[r] >> j) & 1) for j in range(4)], r
        assert posts == [True] * 4 + [bool((env.MARKS[r] >> j) & 1) for j in range(4)], r
        # a door is a dark opening, as wide as a doorway
        assert (geo[:, d0:d0 + env.ND, 3].max() >= 3) and env.DOOR_W == env.X1[8] - env.X0[8]


# ------------------------------------------------------------------------------------------------ DoomPredictPosition
ATTACK, TR, TL = 1, 2, 3


def _pp(n=2):
    env = make("DoomPredictPosition", n=n)
    env.mx[:], env.mdir[:] = 0, 1
    return env


def test_predict_position_no_shot_before_the_loading_time_and_a_single_rocket():
    env = _pp()
    for _ in range(env.LOAD // env.frameskip):
        r, d, _ = act(env, ATTACK)
        assert (env.ammo == 1).all() and not env.ract.any() and not d.any()
    assert (env.tic == env.LOAD).all()
    act(env, ATTACK)                                       # tic LOAD + 1 fires
    assert (env.ammo == 0).all() and env.ract.all() and (env.rth == 0).all()
    assert (env.rz == env.frameskip * env.RSPEED * U).all() and (env.rx == 0).all()
    env.th[:] = 20
    act(env, ATTACK)                                       # there is no second rocket: the first flies on, unturned
    assert (env.ammo == 0).all() and (env.rth == 0).all() and (env.rz == 2 * env.frameskip * env.RSPEED * U).all()


def test_predict_position_a_shot_at_the_present_column_misses_a_walking_monster_and_a_led_one_kills():
    env = _pp(n=3)
    env.tic[:] = 2 * env.DIRT                              # loaded; no chance turn during the flight
    env.mdir[:] = torch.tensor([1, 0, 1])                  # env 1: the monster stands still (not a state of play)
    lead = env.MSPEED * (env.MZ // env.RSPEED)             # the walk during the flight
    env.mx[2] = -lead                                      # env 2: it will be in the sights' column on arrival
    assert lead > env.HIT_W
    total = torch.zeros(3, dtype=torch.int64)
    for i in range(env.MZ // env.RSPEED // env.frameskip + 1):
        mx = env.mx.clone()
        r, d, ep = act(env, ATTACK)
        total += r
        if d.any():
            break
    assert d.all() and total.tolist() == [0, 1, 1] and ep.tolist() == [0.0, 1.0, 1.0]
    assert i == (env.MZ // env.RSPEED) // env.frameskip    # the flight took MZ / RSPEED tics
    assert (env.tic == 0).all() and (env.ammo == 1).all() and not env.killed.any() and not env.ract.any()


def test_predict_position_monster_turns_at_the_ends_and_by_chance():
    env = GAMES["DoomPredictPosition"](64, device="cpu", seed=2)
    env.reset()
    env.mx[:], env.mdir[:] = env.XMAX - 2, 1
    act(env, NOOP)                # no chance turn in tics 1-4: to the end, a tic held there and turned round, two back
    assert (env.mdir == -1).all() and (env.mx == env.XMAX - 2 * env.MSPEED).all()
    env.mx[:], env.mdir[:], env.tic[:] = 0, 1, env.DIRT - 4
    act(env, NOOP)                                         # tic DIRT: one chance in two
    turned = int((env.mdir == -1).sum())
    assert 16 <= turned <= 48 and ((env.mx == 4 * env.MSPEED) | (env.mx == 2 * env.MSPEED)).all()


def test_predict_position_timeout_and_heading_clamp():
    env = _pp()
    env.tic[:] = env.TIMEOUT - 2
    r, d, ep = act(env, NOOP)
    assert d.all() and r.tolist() == [0, 0] and ep.tolist() == [0.0, 0.0]
    env.tic[:] = env.TIMEOUT - 2                           # with the rocket in flight the timeout ends it as well
    env.ammo[:], env.ract[:] = 0, True
    r, d, _ = act(env, NOOP)
    assert d.all() and r.tolist() == [0, 0]
    for _ in range(env.TH_MAX // (env.TURN * env.frameskip) + 2):
        act(env, TR)
    assert (env.th == env.TH_MAX).all()


# ------------------------------------------------------------------------------------------------ DoomDeathmatch
DM_FWD, DM_SEL = 4, 7


def _dm(n=2, monsters=False):
    env = make("DoomDeathmatch", n=n)
    env.th[:] = 0
    if not monsters:
        env.alive[:] = False
        env.mt[:] = 10 ** 6
    return env


def test_deathmatch_each_pickup_and_its_limit():
    env = _dm()
    env.health[:] = torch.tensor([50, 90])
    env.ammo[:] = torch.tensor([5, 45])
    env.kx[:], env.kz[:] = torch.tensor([env.PICK, -env.PICK, 0]), torch.tensor([-env.PICK, 0, env.PICK])
    env.kact[:] = True
    act(env, NOOP)
    assert env.health.tolist() == [75, env.HMAX] and env.ammo.tolist() == [15, env.AMMO_MAX] and env.has2.all()
    assert not env.kact.any()
    env = _dm()
    env.kx[:, 0], env.kact[:, 0], env.health[:] = env.PICK + 1, True, 50      # just outside the reach
    act(env, NOOP)
    assert env.kact[:, 0].all() and (env.health == 50).all()
    # the slots fill at their tics: ammunition at PPHASE, the shotgun at 2 PPHASE, the medkit at PSPAWN
    env = _dm()
    order = []
    for i in range(env.PSPAWN // env.frameskip):
        before = env.kact.clone()
        act(env, NOOP)
        for k in (env.kact[0] & ~before[0]).nonzero().flatten().tolist():
            order.append((k, int(env.tic[0])))
    assert order == [(1, env.PPHASE), (2, 2 * env.PPHASE), (0, env.PSPAWN)]
    assert (env.kx.abs() <= env.KROOM).all() and (env.kz.abs() <= env.KROOM).all()
    assert not torch.equal(env.kx[0], env.kx[1])
    # an owned shotgun does not come again
    env.kact[:, 2], env.has2[:] = False, True
    for _ in range(env.PSPAWN // env.frameskip):
        act(env, NOOP)
    assert not env.kact[:, 2].any()


def test_deathmatch_weapon_cycling_with_one_and_two_weapons():
    env = _dm()
    act(env, DM_SEL)
    assert (env.weapon == 0).all() and (env.swt == 0).all()                  # one weapon: nothing to cycle to
    env.has2[:] = True
    act(env, DM_SEL)
    assert (env.weapon == 1).all() and (env.swt == env.SWITCH - env.frameskip + 1).all()
    ammo = env.ammo.clone()
    act(env, ATTACK)                                                          # no shot while the weapon changes
    assert torch.equal(env.ammo, ammo) and (env.weapon == 1).all()
    act(env, DM_SEL)                                                          # the change is over on this step's tic 1
    assert (env.weapon == 0).all()
    for _ in range(2):
        act(env, NOOP)
    act(env, ATTACK)
    assert torch.equal(env.ammo, ammo - env.PISTOL_COST)


def test_deathmatch_pistol_shotgun_ammunition_and_the_kill():
    env = _dm()
    env.alive[:, 0], env.mx[:, 0], env.mz[:, 0] = True, 0, 60                 # a melee monster straight ahead
    assert (env.aim() % 8 == 0).all()
    total = torch.zeros(2, dtype=torch.int64)
    shots = 0
    while env.alive[:, 0].all():
        r, _, _ = act(env, ATTACK)
        total += r
        shots += 1
        assert shots < 20
    # three pistol shots, one every PISTOL_CD tics, three rounds
    assert shots == 1 + 2 * env.PISTOL_CD // env.frameskip and (env.ammo == env.AMMO - 3 * env.PISTOL_COST).all()
    assert total.tolist() == [1, 1] and (env.mt[:, 0] > 0).all()
    env = _dm()
    env.alive[:, 0], env.mx[:, 0], env.mz[:, 0] = True, 0, 60
    env.has2[:], env.weapon[:] = True, 1
    r, _, _ = act(env, ATTACK)                                                # one shotgun shot, two rounds
    assert r.tolist() == [1, 1] and (env.ammo == env.AMMO - env.SHOTGUN_COST).all() and not env.alive[:, 0].any()
    assert (env.cool == env.SHOTGUN_CD - env.frameskip + 1).all()
    # limits: the shotgun needs two rounds, the pistol one
    for weapon, ammo, fires in ((1, 1, False), (1, 2, True), (0, 0, False), (0, 1, True)):
        env = _dm()
        env.has2[:], env.weapon[:], env.ammo[:] = True, weapon, ammo
        act(env, ATTACK)
        assert (env.ammo == (0 if fires else ammo)).all(), (weapon, ammo)
    # a shot with nothing in the sights costs its rounds and pays nothing
    env = _dm()
    r, _, _ = act(env, ATTACK)
    assert r.tolist() == [0, 0] and (env.ammo == env.AMMO - 1).all()


def test_deathmatch_both_damage_sources_death_and_respawn():
    env = _dm()
    env.alive[:, 0], env.mx[:, 0], env.mz[:, 0] = True, 0, env.MELEE + 2     # melee: two tics away from its reach
    for _ in range(env.BITE // env.frameskip):
        r, d, _ = act(env, NOOP)
    assert (env.health == env.HEALTH - env.DAMAGE).all() and (env.mz[:, 0] == env.MELEE).all()
    # a thrower stops at its stand-off and throws at tic % FIRE == 0; the ball lands FT tics later where the player
    # stood at the launch: env 0 stays and burns, env 1 walks away
    env = _dm()
    env.alive[:, 1], env.mx[:, 1], env.mz[:, 1] = True, 0, env.STANDOFF + 3
    for _ in range(env.FIRE // env.frameskip):
        act(env, NOOP)
    assert env.fact[:, 0].all() and not env.fact[:, 1].any() and (env.mz[:, 1] == env.STANDOFF).all()
    assert (env.ft[:, 0] == env.FT).all()
    env.th[1] = 128
    for _ in range(env.FT // env.frameskip):
        assert (env.health == env.HEALTH).all()
        env._advance(torch.tensor([NOOP, DM_FWD]))
    assert env.health.tolist() == [env.HEALTH - env.FDAMAGE, env.HEALTH] and not env.fact.any()
    # a thrower out of range does not throw
    env = _dm()
    env.px[:], env.pz[:] = -env.ROOM * U, -env.ROOM * U
    env.alive[:, 1], env.mx[:, 1], env.mz[:, 1], env.mhp[:, 1] = True, env.ROOM, env.ROOM, 10 ** 6
    for _ in range(env.FIRE // env.frameskip):
        act(env, NOOP)
    assert not env.fact.any()
    # death ends the episode and costs nothing
    env = _dm()
    env.alive[:, 0], env.mx[:, 0], env.mz[:, 0] = True, 0, 0
    env.health[:] = env.DAMAGE
    for _ in range(env.BITE // env.frameskip):
        r, d, ep = act(env, NOOP)
    assert d.all() and r.tolist() == [0, 0] and ep.tolist() == [0.0, 0.0]
    assert (env.health == env.HEALTH).all() and env.alive.all() and (env.ammo == env.AMMO).all()
    # after a reset every monster stands on its wall; a dead one comes back there after RESPAWN tics
    R = env.ROOM
    assert (env.mz[:, 0] == R).all() and (env.mx[:, 1] == R).all() and (env.mz[:, 2] == -R).all()
    assert (env.mx[:, 3] == -R).all() and (env.mx.abs() <= R).all() and (env.mz.abs() <= R).all()
    env = _dm()
    env.mt[:, 2] = env.RESPAWN
    env.mhp[:, 2] = 0
    for i in range(env.RESPAWN // env.frameskip):
        assert not env.alive[:, 2].any(), i
        act(env, NOOP)
    assert env.alive[:, 2].all() and (env.mz[:, 2] == -R).all() and (env.mhp[:, 2] == env.HP).all()


def test_deathmatch_eighth_action_and_out_of_range_actions():
    env = _dm(n=3)
    env._advance(torch.tensor([6, 8, -1]))
    assert env.th.tolist() == [256 - env.TURN * env.frameskip, 0, 0] and (env.px == 0).all() and (env.pz == 0).all()
    env._advance(torch.tensor([2, 3, 4]))                 # heading 0: right is +x, left is -x, forward is +z
    step = env.SPEED * env.frameskip * U
    assert env.px[1:].tolist() == [-step, 0] and env.pz[1:].tolist() == [0, step]


# ------------------------------------------------------------------------------------------------ palette and scene
def _luma(c):
    return (c[0] * 4899 + c[1] * 9617 + c[2] * 1868 + 8192) >> 14


# the kinds that can overlap on screen in each game, as the module docstring lists them
OVERLAPS = {
    "DoomMyWayHome": [("DOOR", "CEIL"), ("DOOR", "FLOOR"), ("DOOR", "WALL"), ("PILLAR", "DOOR"), ("PILLAR", "CEIL"),
                      ("PILLAR", "FLOOR"), ("PILLAR", "WALL"), ("VEST", "DOOR"), ("VEST", "PILLAR"), ("VEST", "FLOOR"),
                      ("VEST", "WALL"), ("HBAR", "HUD")],
    "DoomPredictPosition": [("PILLAR", "CEIL"), ("PILLAR", "FLOOR"), ("PILLAR", "WALL"), ("MONSTER", "PILLAR"),
                            ("MONSTER", "CEIL"), ("MONSTER", "FLOOR"), ("MONSTER", "WALL"), ("FIREBALL", "MONSTER"),
                            ("FIREBALL", "PILLAR"), ("FIREBALL", "WALL"), ("FIREBALL", "FLOOR"), ("FIREBALL", "CEIL"),
                            ("GUN", "FLOOR"), ("GUN", "MONSTER"), ("GUN", "FIREBALL"), ("HBAR", "HUD"),
                            ("ABAR", "HUD")],
    "DoomDeathmatch": [("PILLAR", "CEIL"), ("PILLAR", "FLOOR"), ("PILLAR", "WALL"), ("PICKUP", "PILLAR"),
                       ("PICKUP", "FLOOR"), ("PICKUP", "WALL"), ("MONSTER", "PICKUP"), ("MONSTER", "PILLAR"),
                       ("MONSTER", "CEIL"), ("MONSTER", "FLOOR"), ("MONSTER", "WALL"), ("FIREBALL", "MONSTER"),
                       ("FIREBALL", "PICKUP"), ("FIREBALL", "PILLAR"), ("FIREBALL", "WALL"), ("FIREBALL", "FLOOR"),
                       ("FIREBALL", "CEIL"), ("GUN", "FLOOR"), ("GUN", "MONSTER"), ("GUN", "FIREBALL"),
                       ("GUN", "PICKUP"), ("HBAR", "HUD"), ("ABAR", "HUD")],
}


@pytest.mark.parametrize("name", NAMES)
def test_overlapping_kinds_are_24_gray_levels_apart(name):
    doc = dw.__doc__
    section = doc[doc.index("``%s``:" % name):]
    section = section[:section.index("\n\n")].replace("\n", " ")
    listed = set(section.split()[1:])
    assert listed == {"%s/%s" % p for p in OVERLAPS[name]}                    # the docstring lists exactly these
    for a, b in OVERLAPS[name]:
        assert abs(_luma(getattr(dw, a)) - _luma(getattr(dw, b))) >= 24, (a, b)
    used = {c for c in make(name).scene().colors}
    named = {getattr(dw, k) for pair in OVERLAPS[name] for k in pair}
    assert used <= named                                                      # no colour of the scene is left out


@pytest.mark.parametrize("name", NAMES)
def test_scene_is_fixed_size_and_in_range_under_random_play(name):
    env = GAMES[name](8, device="cpu", seed=9)
    env.max_episode_steps = 120
    env.reset()
    g = torch.Generator().manual_seed(4)
    nrect = len(env.scene().colors)
    assert nrect == {"DoomMyWayHome": 18, "DoomPredictPosition": 14, "DoomDeathmatch": 24}[name] <= 40
    bars = torch.tensor([c in (dg.HBAR, dg.ABAR) for c in env.scene().colors])
    lo, hi, wmin, shown_n = 0, 0, 1 << 20, 0
    for _ in range(200):
        env._advance(torch.randint(0, env.num_actions, (8,), generator=g))
        geo = env.scene().geometry()
        assert geo.shape == (8, nrect, 4)
        lo, hi = min(lo, int(geo.min())), max(hi, int(geo.max()))
        shown = (geo[..., 2] > 0) & ~bars[None]
        wmin = min(wmin, int(geo[..., 3][shown].min()))
        shown_n += int(shown[:, 3:].sum())
    assert -2048 < lo and hi < 2048
    assert wmin >= 2 and shown_n > 300
    frames = env.frame()
    assert frames.float().std() > 0
    # the gun's width shows the weapon in hand
    if name == "DoomDeathmatch":
        env.weapon[:] = torch.arange(8) % 2
        gun = env.scene().geometry()[:, nrect - 4]
        assert gun[:, 3].tolist() == [env.GUN_W, env.GUN2_W] * 4 and (gun[:, 1] + gun[:, 3] // 2 == 80).all()


# ------------------------------------------------------------------------------------------------ experts, thresholds
def _mean_return(name, policy, steps=150, n=8, seed=3):
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


# margins: the expert of the first two games scores 1 in nearly every episode and chance stays below a quarter
# (MyWayHome: few random walks find the vest's room in 2100 tics; PredictPosition: the 24-unit hit width is an eighth
# of the 192 the monster walks), so half a point separates them; in DoomDeathmatch chance seldom kills before it dies
# and the expert kills every few steps for as long as it plays, so ten kills an episode do
@pytest.mark.parametrize("name,margin", [("DoomMyWayHome", 0.5), ("DoomPredictPosition", 0.5),
                                         ("DoomDeathmatch", 10.0)])
def test_expert_beats_random(name, margin):
    rand, expert = _mean_return(name, "random"), _mean_return(name, "expert")
    print(name, "random", rand, "expert", expert)
    assert expert > rand + margin, (rand, expert)


def test_thresholds_are_the_calibration_scripts_records():
    with open(os.path.join(ROOT, "pathnet_gym_amd", "envs", "thresholds.json")) as f:
        games = json.load(f)["games"]
    assert len(games) == 15
    for name in NAMES:
        rec = games[name]
        want = rec["random"]["mean_return"] + 0.75 * (rec["expert"]["mean_return"] - rec["random"]["mean_return"])
        assert rec["fraction"] == 0.75 and rec["threshold"] == round(want, 1)
        assert rec["random"]["mean_return"] < rec["threshold"] <= rec["expert"]["mean_return"]
        assert rec["random"]["episodes"] == rec["expert"]["episodes"] == 128      # 64 envs, 2 episodes each
        assert registry.reward_threshold(name) == rec["threshold"]
        assert registry.make("Synth" + name + "-v0", num_envs=1).reward_threshold == rec["threshold"]


# ------------------------------------------------------------------------------------------------ presets
def _shape(cfg):
    return [(l.kind, l.out, l.kernel, l.stride) for l in cfg.net.layers], (cfg.net.L, cfg.net.M, cfg.net.N)


def _same_but(a, b, skip=("tasks", "net", "env"), net_skip=("num_actions", "num_tasks")):
    x, y = vars(a).copy(), vars(b).copy()
    for d in (x, y):
        for k in skip:
            d.pop(k)
    nx, ny = vars(a.net).copy(), vars(b.net).copy()
    for d in (nx, ny):
        for k in net_skip:
            d.pop(k)
    return x == y and nx == ny


def test_new_presets_and_the_old_ones_unchanged():
    pong, doom3, doom6 = preset("pong"), preset("doom3"), preset("doom6")
    doom9, transfer = preset("doom9"), preset("doom-transfer")
    assert doom9.tasks == LEVEL_NAMES and doom9.env == "DoomBasic"
    assert doom9.net.num_actions == 8 and doom9.net.num_tasks == 9
    assert transfer.tasks == ["DoomBasic", "DoomDeathmatch"]
    assert transfer.net.num_actions == 8 and transfer.net.num_tasks == 2
    for cfg in (doom9, transfer):
        assert _shape(cfg) == _shape(pong) and _same_but(cfg, doom3)
        for task in cfg.tasks:
            env = registry.make(task, num_envs=1, frameskip=cfg.frameskip, gray=cfg.gray)
            assert env.num_actions <= cfg.net.num_actions and env.obs_shape == tuple(cfg.net.input_shape)
            assert env.reward_threshold == registry.reward_threshold(task) < float("inf")
    for name, task, na in (("doom-my-way-home", "DoomMyWayHome", 4), ("doom-predict", "DoomPredictPosition", 4),
                           ("doom-deathmatch", "DoomDeathmatch", 8)):
        one = preset(name)
        assert one.tasks == [task] and one.env == task and one.net.num_tasks == 1 and one.net.num_actions == na
        assert _shape(one) == _shape(pong) and _same_but(one, doom3)
        assert registry.make(one.env, num_envs=1).num_actions == (8 if na == 8 else 4)
    # what was there is what it was
    assert doom3.tasks == ["DoomBasic", "DoomDefendCenter", "DoomTakeCover"]
    assert doom3.net.num_actions == 4 and doom3.net.num_tasks == 3
    assert doom6.tasks == [n for n in LEVEL_NAMES if n in dg.DOOM_GAMES]
    assert doom6.net.num_actions == 7 and doom6.net.num_tasks == 6 and _same_but(doom6, doom3)
    for name, task, na in (("doom-basic", "DoomBasic", 4), ("doom_basic", "DoomBasic", 4),
                           ("doom-corridor", "DoomCorridor", 7), ("doom-defend-line", "DoomDefendLine", 4),
                           ("doom-health", "DoomHealthGathering", 4)):
        one = preset(name)
        assert one.tasks == [task] and one.net.num_actions == na and one.net.num_tasks == 1 and _same_but(one, doom3)


def test_continual_script_and_cli_accept_the_new_presets():
    import continual
    for name, nt in (("doom9", 9), ("doom-transfer", 2)):
        args = argparse.Namespace(preset=name, paths=None, envs=None, tmax=None, N=4, trunk_scale=None, lr=None,
                                  frozen_mode="or", frames=1000, seed=1, dtype=None, ring=False)
        cfg = continual.build_cfg(args, preset(name).tasks)
        assert len(cfg.tasks) == nt and cfg.net.num_tasks == nt and cfg.net.num_actions == 8
    from pathnet_gym_amd.cli import build_parser
    text = build_parser()._subparsers._group_actions[0].choices["train"].format_help()
    text = re.sub(r"-\s*\n\s*", "-", text)                 # argparse wraps the list at hyphens
    for name in ("doom9", "doom-transfer", "doom-my-way-home", "doom-predict", "doom-deathmatch", "doom6",
                 "doom-corridor"):
        assert name in text, name


# ------------------------------------------------------------------------------------------------ the oracle run
SEED, ACTION_SEED = 11, 3
# the play of the bit-exact comparison: N = 96 envs, 300 agent steps, episodes capped at 60 steps.  Env i follows the
# scripted expert of scripts/calibrate_thresholds.py (read from the oracle's state) when i % 4 == 0, and uniform
# random actions otherwise.  No policy lives to a tic timeout in 60 steps, so env i with i % 8 == 1 (random) starts
# late, once, after the first reset: DoomMyWayHome LATE_TICS["DoomMyWayHome"] tics before the timeout, and
# DoomPredictPosition so close to it that even a rocket fired at once is still in flight when it comes.
# DoomDeathmatch needs no late start: death comes to the random players long before the cap.
EXPERT_EVERY = 4
LATE_TICS = {"DoomMyWayHome": 100, "DoomPredictPosition": 8}


def _state(env):
    return {name: getattr(env, name).clone() for name, _ in env._fields()}


def late_start(env):
    """The late state, written into the torch state and, for a HIP env, into the kernel's rows."""
    if env.id not in LATE_TICS:
        return
    env.sync_from_device()
    i = torch.arange(env.num_envs, device=env.device)
    env.tic.copy_(torch.where(i % 8 == 1, torch.full_like(env.tic, env.TIMEOUT - LATE_TICS[env.id]), env.tic))
    if env._hip:
        env._st32.copy_(env._hip_pack())


class Events:
    """Counts, from the torch oracle's state before and after a step, the events that make each game."""
    BITES, BURNS = {6, 12, 16, 22, 26, 32}, {10, 20, 16, 22, 26, 32}     # health lost by 0-2 bites and 0-2 fireballs

    def __init__(self, env, cap):
        self.env, self.cap = env, cap
        self.count = {}
        self.snap()

    def snap(self):
        self.prev = _state(self.env)

    def add(self, key, n):
        self.count[key] = self.count.get(key, 0) + int(n)

    def step(self, action, reward, done):
        e, p = self.env, self.prev
        run = ~done                                            # a finished env shows the next episode's state
        ended = done & (p["steps"] + 1 < self.cap)             # by the game, not by the cap
        timeout = ended & (p["tic"] + e.frameskip >= e.TIMEOUT)
        if e.id == "DoomMyWayHome":
            self.add("door_crossing", (run & (e.region_of(p["px"], p["pz"]) != e.region_of(e.px, e.pz))).sum())
            fwd = e.SPEED * U
            sx, sz = dg.fdiv(fwd * e.isin(p["th"]), 256), dg.fdiv(fwd * e.icos(p["th"]), 256)
            free = (e.px - p["px"] == e.frameskip * sx) & (e.pz - p["pz"] == e.frameskip * sz)
            self.add("blocked", (run & (action == 1) & ~free).sum())
            self.add("vest", (ended & (reward > 0)).sum())
            self.add("timeout", (timeout & (reward == 0)).sum())
        elif e.id == "DoomPredictPosition":
            self.add("hit", (ended & (reward > 0)).sum())
            self.add("miss", (ended & (reward == 0) & ~timeout).sum())
            self.add("timeout", timeout.sum())
            self.add("launch", (run & ~p["ract"] & e.ract).sum())
        else:
            kills = torch.where(reward > 0, reward.long(), torch.zeros_like(p["weapon"]))
            self.add("kill_pistol", (kills * (p["weapon"] == 0)).sum())
            self.add("kill_shotgun", (kills * (p["weapon"] == 1)).sum())
            took = run[:, None] & p["kact"] & ~e.kact
            for k, key in enumerate(("medkit", "ammunition", "shotgun")):
                self.add(key, took[:, k].sum())
            lost = torch.where(run & ~took[:, 0], p["health"] - e.health, torch.zeros_like(e.health)).tolist()
            self.add("bite", sum(1 for v in lost if v in self.BITES))
            self.add("fireball_hit", sum(1 for v in lost if v in self.BURNS))
            self.add("respawn", (run[:, None] & ~p["alive"] & e.alive).sum())
            self.add("weapon_change", (run & (p["weapon"] != e.weapon)).sum())
            self.add("death", ended.sum())
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
        ev.step(a, rt, dt)
        ndone += int(dt.sum())
    ev.add("done", ndone)
    return et, eh, ev.count


# what the oracle alone shows on the CPU with these seeds
EXPECTED = {
    "DoomMyWayHome": {"door_crossing": 1391, "blocked": 2949, "vest": 233, "timeout": 12, "done": 591},
    "DoomPredictPosition": {"hit": 405, "miss": 947, "timeout": 12, "launch": 1367, "done": 1369},
    "DoomDeathmatch": {"kill_pistol": 338, "kill_shotgun": 334, "medkit": 172, "ammunition": 243, "shotgun": 164,
                       "bite": 3797, "fireball_hit": 1547, "respawn": 560, "weapon_change": 305, "death": 316,
                       "done": 505},
}
NEEDED = {"DoomMyWayHome": ("door_crossing", "blocked", "vest", "timeout"),
          "DoomPredictPosition": ("hit", "miss", "timeout"),
          "DoomDeathmatch": ("kill_pistol", "kill_shotgun", "medkit", "ammunition", "shotgun", "death", "bite",
                             "fireball_hit")}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_run_contains_the_games_events(name):
    """CPU: the seeds and the action mix of the bit-exact comparison give a run with every event of the game."""
    _, _, count = play(name, "cpu", hip=False)
    print(name, count)
    for k in NEEDED[name]:
        assert count[k] >= 1, (k, count)
    assert count == EXPECTED[name]
