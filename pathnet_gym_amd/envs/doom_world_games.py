"""Synthetic first-person Doom scenarios, the last three levels: DoomMyWayHome, DoomPredictPosition, DoomDeathmatch.

They use the machinery of ``envs/doom_games.py`` (``DoomNavVec``: integer trig, the view transform, the projection, the
hit-scan rule) and run in ``csrc/games.hip`` as game ids 12 to 14, with this torch code as the bit-exact oracle
(``tests/test_doom_world_games.py``, ``tests/test_doom_world_hip.py``).

* ``DoomMyWayHome``      NOOP, MOVE_FORWARD, TURN_RIGHT, TURN_LEFT.  A fixed map of five rooms, four doorways and one
                         dead-end corridor; the player starts in a random room at a random place and heading and
                         walks to the vest, which always lies in the same room.  Reaching it pays +1 and ends the
                         episode.
* ``DoomPredictPosition`` NOOP, ATTACK, TURN_RIGHT, TURN_LEFT.  The player turns at the origin; one monster walks
                         along the far side and turns round by chance.  After the loading time the launcher fires its
                         one rocket, which flies at a finite speed along the heading it was fired at: a hit pays +1,
                         and the rocket's arrival ends the episode either way.
* ``DoomDeathmatch``     the ``constant-7`` action set of the reference's Doom experiment: NOOP, ATTACK, MOVE_RIGHT,
                         MOVE_LEFT, MOVE_FORWARD, TURN_RIGHT, TURN_LEFT, SELECT_NEXT_WEAPON.  A square arena; four
                         monsters spawn at the walls and approach (melee and fireball throwers by turns); medkits,
                         ammunition and a shotgun spawn as pickups.  A kill pays +1; death ends the episode and
                         costs nothing.

Living reward: ``my_way_home.cfg`` and ``predict_position.cfg`` carry -0.0001 per tic.  The games' rewards are
integers (the driver sums ``int``; ``reward_clip = 1`` would destroy a rescaling), so ``world_scenario`` rounds it to
0 for these two levels.  ``doom_games.scenario`` is unchanged and still refuses a fractional value.

RNG streams (next to the list in ``envs/doom_games.py``): 100-103 (DoomMyWayHome: start room, x, z, heading), 110-112
(DoomPredictPosition: the monster's turns, its start x and direction), 120-123, 130-135 and 140 (DoomDeathmatch: the
spawn place of monster k, the x and z of pickup k, the heading at reset).

Painter's order per rectangle slot.  In ``DoomMyWayHome`` it is backdrop, door openings, posts, vest, HUD.  Its world is not
convex, but only the region the player stands in is drawn (its door openings, its posts and, in the vest's room, the
vest), and every region is a convex rectangle, so the rule of ``DoomNavVec`` holds: a door opening is part of the
wall's surface, posts stand in front of the walls, and whatever lies inside the region is nearer than both.  Both
implementations find the region by the same integer rule, ``region_of``: region k holds the points with
``X0[k] * U <= px < X1[k] * U`` and ``Z0[k] * U <= pz < Z1[k] * U``.  Rooms are told apart by their marker posts (a
post at a quarter of a wall; ``MARKS``), a door is a dark opening in the middle of its wall.  In
``DoomPredictPosition`` it is backdrop, posts on the far wall, the monster (it walks in front of the wall), the rocket,
HUD.  In ``DoomDeathmatch`` it is backdrop, posts on the walls of the convex arena, pickups, monsters, fireballs, HUD.  The kinds that can overlap on
screen, each pair at least 24 gray levels apart:

``DoomMyWayHome``: DOOR/CEIL DOOR/FLOOR DOOR/WALL PILLAR/DOOR PILLAR/CEIL PILLAR/FLOOR PILLAR/WALL VEST/DOOR
VEST/PILLAR VEST/FLOOR VEST/WALL HBAR/HUD

``DoomPredictPosition``: PILLAR/CEIL PILLAR/FLOOR PILLAR/WALL MONSTER/PILLAR MONSTER/CEIL MONSTER/FLOOR MONSTER/WALL
FIREBALL/MONSTER FIREBALL/PILLAR FIREBALL/WALL FIREBALL/FLOOR FIREBALL/CEIL GUN/FLOOR GUN/MONSTER GUN/FIREBALL
HBAR/HUD ABAR/HUD

``DoomDeathmatch``: PILLAR/CEIL PILLAR/FLOOR PILLAR/WALL PICKUP/PILLAR PICKUP/FLOOR PICKUP/WALL MONSTER/PICKUP
MONSTER/PILLAR MONSTER/CEIL MONSTER/FLOOR MONSTER/WALL FIREBALL/MONSTER FIREBALL/PICKUP FIREBALL/PILLAR
FIREBALL/WALL FIREBALL/FLOOR FIREBALL/CEIL GUN/FLOOR GUN/MONSTER GUN/FIREBALL GUN/PICKUP HBAR/HUD ABAR/HUD

"""
from __future__ import annotations

import torch

from .atari_games import GAMES, Scene
from .doom.constants import ACTION_CONFIGS, ACTIONS, BUTTONS, CONFIG, DOOM_SETTINGS, LEVEL_NAMES
from .doom.scenarios import SCENARIOS
from .doom_games import (ABAR, CEIL, FH, FIREBALL, FLOOR, GUN, HBAR, HUD, HUD_Y0, K, MONSTER,  # noqa: F401
                         PILLAR, QSIN, SHOOTER, SIDE, U, VEST, WALL, Z0, ZVIEW, DoomNavVec, fdiv)

DOOR = SIDE                            # a door opening: over CEIL, FLOOR and WALL; under PILLAR and VEST
PICKUP = SHOOTER                       # medkit, ammunition, shotgun: over FLOOR, WALL and PILLAR; under MONSTER


def world_scenario(level: str):
    """(living_reward, death_penalty, episode_timeout, buttons) of a level, as ``doom_games.scenario`` gives them,
    with the two differences of these levels: a living reward below half a point rounds to 0, and DoomDeathmatch
    plays the ``constant-7`` buttons (its own 42 are beyond the heads kernels' 32 actions)."""
    row = DOOM_SETTINGS[LEVEL_NAMES.index(level)]
    spec = SCENARIOS[row[CONFIG]]
    if level == "DoomDeathmatch":
        picked = ACTION_CONFIGS["constant-7"]
        assert set(picked) <= set(row[ACTIONS]), level
        buttons = [BUTTONS[i] for i in picked]
    else:
        buttons = [BUTTONS[i] for i in row[ACTIONS]]
        assert buttons == spec["buttons"], level
    living, death = spec.get("living_reward", 0), spec.get("death_penalty", 0)
    assert abs(living) < 0.5 and death == int(death), level
    return int(round(living)), int(death), int(spec["episode_timeout"]), buttons


class DoomWorldVec(DoomNavVec):
    """``DoomNavVec`` with the scenario constants of ``world_scenario``."""

    def init_state(self):
        self.LIVING, self.DEATH_PENALTY, self.TIMEOUT, self.BUTTONS = world_scenario(self.LEVEL)
        assert self.n_actions == 1 + len(self.BUTTONS) and self.LIVING == 0
        self.qsin = torch.tensor(QSIN, dtype=torch.int64, device=self.device)

    def const(self, values):
        return torch.tensor(values, dtype=torch.int64, device=self.device)

    def flag(self, a, name: str):
        return self.button(a, name).long()



# ===========================================================================
class DoomMyWayHomeVec(DoomWorldVec):
    """Free space is the union of NR regions, rectangles in whole world units that tile without overlap: five rooms
    A to E (0-4), the dead-end corridor F (5) off room C, and four doorways (6-9), one per door, as thick as the
    walls (WALL_T).  MOVE_FORWARD walks SPEED per tic along the heading (TURN units per tic), one axis after the
    other; an axis' move is taken when its end point lies in a region and dropped otherwise, so walls stop the
    player, who slides along them, and a doorway is the only passage: a step (4 units) is shorter than a wall is
    thick.  The vest lies in the middle of room E; being within TOUCH of it on both axes pays +1 and ends the
    episode.  At reset the player gets one of the rooms A to D, a place at least MARGIN from its walls and a heading.

    Scene of the region the player stands in: a door opening (DOOR_W x DOOR_H) in the middle of every wall that has
    a door (``DOORS``, bit 0 north = z1, 1 east = x1, 2 south = z0, 3 west = x0), posts (POST_W) at the four
    corners and marker posts at a quarter of the walls named in ``MARKS`` (same bits), and the vest in room E.

    int32 bound of the view transform: the map spans 416 x 272 world units, 6656 x 4352 sub-units, so the offset of
    any two of its points is below 2^13 on each axis, inside the 2^14 of ``DoomNav::view``.
    """
    id = "DoomMyWayHome"
    LEVEL = "DoomMyWayHome"
    n_actions = 4
    reward_threshold = 0.5
    max_steps = 10000
    HIP_GAME = "DoomMyWayHome"
    HIP_FIELDS = (("px", "i"), ("pz", "i"), ("th", "i"), ("tic", "i"), ("won", "i"))
    NR, NROOMS, NSTART, ND, NP = 10, 5, 4, 4, 8
    #      A    B    C    D    E    F    AB   BC   AD   DE
    X0 = (0, 144, 288, 0, 144, 336, 128, 272, 48, 128)
    Z0R = (0, 0, 0, 144, 144, 128, 48, 48, 128, 192)
    X1 = (128, 272, 416, 128, 272, 368, 144, 288, 80, 144)
    Z1R = (128, 128, 128, 272, 272, 272, 80, 80, 144, 224)
    DOORS = (3, 10, 9, 6, 8, 4, 10, 10, 5, 10)
    MARKS = (4, 1, 6, 9, 7, 0, 0, 0, 0, 0)
    VEST_ROOM, VEST_X, VEST_Z = 4, 208, 208
    WALL_T, MARGIN, ROOM_SIZE = 16, 16, 128
    SPEED, TURN, TOUCH = 4, 4, 16
    DOOR_W, DOOR_H, POST_W = 32, 70, 12
    VEST_W, VEST_H = 16, 16

    def init_state(self):
        super().init_state()
        self.px, self.pz, self.th, self.tic = (self.zeros() for _ in range(4))
        self.won = self.zeros(dtype=torch.bool)
        self.rx0, self.rz0, self.rx1, self.rz1 = (self.const(v) for v in (self.X0, self.Z0R, self.X1, self.Z1R))
        self.doors, self.marks = self.const(self.DOORS), self.const(self.MARKS)
        self.bits = torch.arange(4, device=self.device)[None]

    def region_of(self, px, pz):
        """Index [N] of the region that holds the point (in sub-units), -1 for a point inside a wall."""
        r = torch.full_like(px, -1)
        for k in range(self.NR):
            inside = (px >= self.X0[k] * U) & (px < self.X1[k] * U) & (pz >= self.Z0R[k] * U) & (pz < self.Z1R[k] * U)
            r = torch.where(inside, torch.full_like(r, k), r)
        return r

    def reset_state(self, m):
        room = self.rand(100, self.NSTART)
        span = self.ROOM_SIZE - 2 * self.MARGIN
        x = (self.rx0[room] + self.MARGIN + self.rand(101, span)) * U
        z = (self.rz0[room] + self.MARGIN + self.rand(102, span)) * U
        self.px = torch.where(m, x, self.px)
        self.pz = torch.where(m, z, self.pz)
        self.th = torch.where(m, self.rand(103, 256), self.th)
        self.tic = self.where_set(self.tic, m, 0)
        self.won = self.won & ~m

    def physics(self, a):
        live = ~self.game_over()
        self.put("tic", live, self.tic + 1)
        self.put("th", live, (self.th + self.heading_step(a)) % 256)
        fwd = self.flag(a, "MOVE_FORWARD") * self.SPEED * U
        nx = self.px + fdiv(fwd * self.isin(self.th), 256)
        self.put("px", live & (self.region_of(nx, self.pz) >= 0), nx)
        nz = self.pz + fdiv(fwd * self.icos(self.th), 256)
        self.put("pz", live & (self.region_of(self.px, nz) >= 0), nz)
        wx, wz = fdiv(self.px, U), fdiv(self.pz, U)
        touch = live & ((wx - self.VEST_X).abs() <= self.TOUCH) & ((wz - self.VEST_Z).abs() <= self.TOUCH)
        self.won = self.won | touch
        return touch.long()

    def game_over(self):
        return self.won | (self.tic >= self.TIMEOUT)

    def scene(self) -> Scene:
        sc = Scene(self.num_envs, self.device)
        self.backdrop(sc)
        r = self.region_of(self.px, self.pz).clamp(min=0)
        x0, z0, x1, z1 = (t[r][:, None] for t in (self.rx0, self.rz0, self.rx1, self.rz1))
        px, pz = self.px[:, None], self.pz[:, None]
        xm, zm = fdiv(x0 + x1, 2), fdiv(z0 + z1, 2)
        dx, dz = self.view(torch.cat([xm, x1, xm, x0], 1) * U - px, torch.cat([z1, zm, z0, zm], 1) * U - pz)
        y0, xl, h, w, drawn = self.nav_project(dx, dz, self.DOOR_W, self.DOOR_H)
        sc.add_many(y0, xl, h, w, [DOOR] * self.ND, visible=drawn & (((self.doors[r][:, None] >> self.bits) & 1) == 1))
        xq, zq = x0 + fdiv(x1 - x0, 4), z0 + fdiv(z1 - z0, 4)
        dx, dz = self.view(torch.cat([x0, x1, x1, x0, xq, x1, xq, x0], 1) * U - px,
                           torch.cat([z0, z0, z1, z1, z1, zq, z0, zq], 1) * U - pz)
        y0, xl, h, w, drawn = self.nav_project(dx, dz, self.POST_W, 2 * FH)
        marked = ((self.marks[r][:, None] >> self.bits) & 1) == 1
        sc.add_many(y0, xl, h, w, [PILLAR] * self.NP, visible=drawn & torch.cat([torch.ones_like(marked), marked], 1))
        dx, dz = self.view(self.VEST_X * U - self.px, self.VEST_Z * U - self.pz)
        y0, xl, h, w, drawn = self.nav_project(dx, dz, self.VEST_W, self.VEST_H)
        sc.add(y0, xl, h, w, VEST, visible=drawn & (r == self.VEST_ROOM))
        self.hud(sc, torch.full_like(self.px, 100))
        return sc


# ===========================================================================
class DoomPredictPositionVec(DoomWorldVec):
    """The player stands at the origin and turns within +-TH_MAX (TURN units per tic).  The monster walks MSPEED per
    tic along the line z = MZ between x = +-XMAX, turns round at the ends and, every DIRT tics, with one chance in
    two (RNG stream 110).  ATTACK fires the one rocket once ``tic > LOAD``; it starts at the player and flies RSPEED
    per tic along the heading it was fired at (``rth``).  On the tic its depth reaches MZ the flight ends: within
    HIT_W of the monster it kills (+1), and either way the episode is over.  At z = MZ the flight takes MZ / RSPEED
    = 15 tics or more, in which the monster walks 30 units, more than HIT_W: a shot at its present column misses.
    Posts stand on the far wall z = WALLZ at multiples of POST_GAP.
    """
    id = "DoomPredictPosition"
    LEVEL = "DoomPredictPosition"
    n_actions = 4
    reward_threshold = 0.5
    max_steps = 10000
    HIP_GAME = "DoomPredictPosition"
    HIP_FIELDS = (("th", "i"), ("tic", "i"), ("mx", "i"), ("mdir", "i"), ("rx", "i"), ("rz", "i"), ("rth", "i"),
                  ("ract", "i"), ("ammo", "i"), ("killed", "i"))
    NP = 5
    TURN, TH_MAX = 1, 40
    MZ, WALLZ, XMAX, MSPEED, DIRT = 120, 128, 96, 2, 32
    LOAD, RSPEED, HIT_W = 48, 8, 12
    MON_W, MON_H, POST_W, POST_GAP = 24, 40, 12, 48
    RK_W, RK_H, RK_LIFT = 8, 8, 25

    def init_state(self):
        super().init_state()
        self.th, self.tic, self.mx, self.mdir, self.rx, self.rz, self.rth, self.ammo = (self.zeros() for _ in range(8))
        self.ract, self.killed = self.zeros(dtype=torch.bool), self.zeros(dtype=torch.bool)
        self.post_x = (torch.arange(self.NP, device=self.device)[None] - self.NP // 2) * self.POST_GAP

    def reset_state(self, m):
        for name, v in (("th", 0), ("tic", 0), ("rx", 0), ("rz", 0), ("rth", 0), ("ammo", 1)):
            setattr(self, name, self.where_set(getattr(self, name), m, v))
        self.mx = torch.where(m, self.rand(111, 2 * self.XMAX + 1) - self.XMAX, self.mx)
        self.mdir = torch.where(m, self.rand(112, 2) * 2 - 1, self.mdir)
        self.ract = self.ract & ~m
        self.killed = self.killed & ~m

    def physics(self, a):
        live = ~self.game_over()
        self.put("tic", live, self.tic + 1)
        self.put("th", live, (self.th + self.heading_step(a)).clamp(-self.TH_MAX, self.TH_MAX))
        turn = live & (self.tic % self.DIRT == 0) & (self.rand(110, 2) == 1)
        mdir = torch.where(turn, -self.mdir, self.mdir)
        nmx = self.mx + mdir * self.MSPEED
        mdir = torch.where(nmx.abs() > self.XMAX, -mdir, mdir)
        self.put("mdir", live, mdir)
        self.put("mx", live, nmx.clamp(-self.XMAX, self.XMAX))
        fire = live & self.button(a, "ATTACK") & (self.tic > self.LOAD) & (self.ammo > 0)
        self.ammo = self.ammo - fire.long()
        self.rx = torch.where(fire, torch.zeros_like(self.rx), self.rx)
        self.rz = torch.where(fire, torch.zeros_like(self.rz), self.rz)
        self.rth = torch.where(fire, self.th, self.rth)
        self.ract = self.ract | fire
        fly = live & self.ract
        step = self.RSPEED * U
        self.rx = torch.where(fly, self.rx + fdiv(step * self.isin(self.rth), 256), self.rx)
        self.rz = torch.where(fly, self.rz + fdiv(step * self.icos(self.rth), 256), self.rz)
        arrive = fly & (fdiv(self.rz, U) >= self.MZ)
        hit = arrive & ((fdiv(self.rx, U) - self.mx).abs() <= self.HIT_W)
        self.ract = self.ract & ~arrive
        self.killed = self.killed | hit
        return hit.long()

    def game_over(self):
        return self.killed | ((self.ammo <= 0) & ~self.ract) | (self.tic >= self.TIMEOUT)

    def scene(self) -> Scene:
        sc = Scene(self.num_envs, self.device)
        self.backdrop(sc)
        dx, dz = self.view(self.post_x.expand(self.num_envs, self.NP) * U,
                           torch.full_like(self.post_x, self.WALLZ * U).expand(self.num_envs, self.NP))
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.POST_W, 2 * FH)
        sc.add_many(y0, x0, h, w, [PILLAR] * self.NP, visible=drawn)
        dx, dz = self.view(self.mx * U, torch.full_like(self.mx, self.MZ * U))
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.MON_W, self.MON_H)
        sc.add(y0, x0, h, w, MONSTER, visible=drawn & ~self.killed)
        dx, dz = self.view(self.rx, self.rz)
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.RK_W, self.RK_H)
        sc.add(y0 - fdiv(self.RK_LIFT * K, dz.clamp(0, ZVIEW) + Z0), x0, h, w, FIREBALL, visible=drawn & self.ract)
        self.hud(sc, torch.full_like(self.th, 100), self.ammo, gun=True)
        return sc


# ===========================================================================
class DoomDeathmatchVec(DoomWorldVec):
    """A square arena |x|, |z| <= ROOM.  MOVE_FORWARD / MOVE_RIGHT / MOVE_LEFT walk SPEED per tic along or across the
    heading (TURN units per tic), clamped to the arena.

    Monsters: NM slots in whole world units, HP hit points each.  Slot k spawns on wall k % 4 (north, east, south,
    west) at a random place and walks MSPEED per tic and axis towards the player while it is farther than its stop
    distance on either axis: even slots are melee (MELEE) and, once that close, bite for DAMAGE every BITE tics; odd
    slots are throwers (STANDOFF) and, within FRANGE, every FIRE tics (phase FPHASE per thrower) throw a fireball at
    where the player stands; it flies FT tics and takes FDAMAGE when the player is then within HIT of that spot on
    both axes.  A dead slot comes back at its wall after RESPAWN tics.

    Weapons: the pistol (weapon 0: PISTOL_DMG a shot, PISTOL_COST rounds, every PISTOL_CD tics) and the shotgun
    (weapon 1, once picked up: SHOTGUN_DMG, SHOTGUN_COST, SHOTGUN_CD), so the shotgun kills with one shot and two
    rounds where the pistol needs three shots and three rounds.  ATTACK hits the monster in the sights
    (``DoomNavVec.sights``, width MON_W).  SELECT_NEXT_WEAPON cycles through the owned weapons; the change takes
    SWITCH tics, in which the player can neither shoot nor change again.  A kill pays +1.

    Pickups: slot 0 a medkit (HEAL up to HMAX), slot 1 ammunition (AMMO_BOX rounds up to AMMO_MAX), slot 2 the
    shotgun (only while it is not owned).  Slot k appears when ``tic % PSPAWN == PPHASE * k`` and it is empty, at a
    random place within KROOM of the centre; standing within PICK of it on both axes takes it.
    """
    id = "DoomDeathmatch"
    LEVEL = "DoomDeathmatch"
    n_actions = 8
    reward_threshold = 20.0
    max_steps = 10000
    HIP_GAME = "DoomDeathmatch"
    HIP_FIELDS = (("px", "i"), ("pz", "i"), ("th", "i"), ("health", "i"), ("ammo", "i"), ("cool", "i"), ("swt", "i"),
                  ("weapon", "i"), ("has2", "i"), ("tic", "i"), ("mx", "vec"), ("mz", "vec"), ("mhp", "vec"),
                  ("mt", "vec"), ("fx", "vec"), ("fz", "vec"), ("fvx", "vec"), ("fvz", "vec"), ("ft", "vec"),
                  ("kx", "vec"), ("kz", "vec"), ("alive", "mask"), ("fact", "mask"), ("kact", "mask"))
    NM, NF, NK, NP = 4, 2, 3, 8
    ROOM, KROOM, SPEED, TURN, MSPEED = 96, 88, 4, 4, 1
    HP, MELEE, STANDOFF, FRANGE, RESPAWN = 3, 10, 48, 120, 32
    BITE, DAMAGE, FIRE, FPHASE, FT, FDAMAGE, HIT = 8, 6, 32, 16, 24, 10, 12
    HEALTH, HMAX, HEAL, AMMO, AMMO_MAX, AMMO_BOX = 100, 100, 25, 20, 50, 10
    PISTOL_DMG, PISTOL_COST, PISTOL_CD, SHOTGUN_DMG, SHOTGUN_COST, SHOTGUN_CD, SWITCH = 1, 1, 8, 3, 2, 16, 8
    PSPAWN, PPHASE, PICK, KMULX, KMULZ, SMUL = 64, 16, 12, 37, 59, 41
    MON_W, MON_H, SH_W, SH_H, POST_W = 24, 40, 20, 48, 12
    KIT_W, KIT_H, BOX_W, BOX_H, SG_W, SG_H = 12, 12, 8, 16, 24, 8
    FB_W, FB_H, FB_LIFT = 12, 12, 25
    GUN_W, GUN2_W = 12, 20

    def init_state(self):
        super().init_state()
        (self.px, self.pz, self.th, self.health, self.ammo, self.cool, self.swt, self.weapon,
         self.tic) = (self.zeros() for _ in range(9))
        self.has2 = self.zeros(dtype=torch.bool)
        self.mx, self.mz, self.mhp, self.mt = (self.zeros(self.NM) for _ in range(4))
        self.fx, self.fz, self.fvx, self.fvz, self.ft = (self.zeros(self.NF) for _ in range(5))
        self.kx, self.kz = self.zeros(self.NK), self.zeros(self.NK)
        self.alive = self.zeros(self.NM, dtype=torch.bool)
        self.fact = self.zeros(self.NF, dtype=torch.bool)
        self.kact = self.zeros(self.NK, dtype=torch.bool)
        dev, R = self.device, self.ROOM
        self.kidx = torch.arange(self.NM, device=dev)[None]
        self.jidx = torch.arange(self.NF, device=dev)[None]
        self.pidx = torch.arange(self.NK, device=dev)[None]
        self.is_sh = (self.kidx % 2) == 1
        self.stop = torch.where(self.is_sh, self.STANDOFF, self.MELEE)
        self.mw = torch.where(self.is_sh, self.SH_W, self.MON_W)
        self.mh = torch.where(self.is_sh, self.SH_H, self.MON_H)
        posts = ((-R, -R), (0, -R), (R, -R), (R, 0), (R, R), (0, R), (-R, R), (-R, 0))
        self.post_x = self.const([p[0] for p in posts])[None]
        self.post_z = self.const([p[1] for p in posts])[None]
        self.kw, self.kh = self.const([self.KIT_W, self.BOX_W, self.SG_W])[None], \
            self.const([self.KIT_H, self.BOX_H, self.SG_H])[None]

    def spawn_place(self, tic):
        """([N, NM] x, z): slot k's place on wall k % 4.  The RNG counter moves once per agent step, the tic
        separates a step's tics."""
        span = 2 * self.ROOM + 1
        c = torch.stack([self.rand(120 + k, span) for k in range(self.NM)], 1)
        c = (c + tic[:, None] * self.SMUL) % span - self.ROOM
        wall = self.kidx % 4
        R = torch.full_like(c, self.ROOM)
        x = torch.where(wall == 0, c, torch.where(wall == 1, R, torch.where(wall == 2, c, -R)))
        z = torch.where(wall == 0, R, torch.where(wall == 1, c, torch.where(wall == 2, -R, c)))
        return x, z

    def reset_state(self, m):
        for name, v in (("px", 0), ("pz", 0), ("health", self.HEALTH), ("ammo", self.AMMO), ("cool", 0), ("swt", 0),
                        ("weapon", 0), ("tic", 0)):
            setattr(self, name, self.where_set(getattr(self, name), m, v))
        self.th = torch.where(m, self.rand(140, 256), self.th)
        self.has2 = self.has2 & ~m
        mm = m[:, None]
        x, z = self.spawn_place(torch.zeros_like(self.tic))
        self.mx = torch.where(mm, x, self.mx)
        self.mz = torch.where(mm, z, self.mz)
        self.mhp = torch.where(mm, torch.full_like(self.mhp, self.HP), self.mhp)
        self.mt = torch.where(mm, torch.zeros_like(self.mt), self.mt)
        for name in ("fx", "fz", "fvx", "fvz", "ft", "kx", "kz"):
            t = getattr(self, name)
            setattr(self, name, torch.where(mm, torch.zeros_like(t), t))
        self.alive = self.alive | mm
        self.fact = self.fact & ~mm
        self.kact = self.kact & ~mm

    def monsters_view(self):
        return self.view(self.mx * U - self.px[:, None], self.mz * U - self.pz[:, None])

    def aim(self):
        dx, dz = self.monsters_view()
        return self.sights(dx, dz, self.mw, self.alive)

    def cost(self):
        return torch.where(self.weapon == 1, self.SHOTGUN_COST, self.PISTOL_COST)

    def physics(self, a):
        live = ~self.game_over()
        self.put("tic", live, self.tic + 1)
        self.put("th", live, (self.th + self.heading_step(a)) % 256)
        fwd = self.flag(a, "MOVE_FORWARD")
        side = self.flag(a, "MOVE_RIGHT") - self.flag(a, "MOVE_LEFT")
        s, c = self.isin(self.th), self.icos(self.th)
        step, lim = self.SPEED * U, self.ROOM * U
        self.put("px", live, (self.px + fdiv(step * (fwd * s + side * c), 256)).clamp(-lim, lim))
        self.put("pz", live, (self.pz + fdiv(step * (fwd * c - side * s), 256)).clamp(-lim, lim))
        wx, wz = fdiv(self.px, U), fdiv(self.pz, U)
        # weapons
        swt = (self.swt - 1).clamp(min=0)
        change = live & self.button(a, "SELECT_NEXT_WEAPON") & (swt == 0) & self.has2
        self.put("swt", live, torch.where(change, torch.full_like(swt, self.SWITCH), swt))
        self.weapon = torch.where(change, 1 - self.weapon, self.weapon)
        cool = (self.cool - 1).clamp(min=0)
        shotgun = self.weapon == 1
        fire = live & self.button(a, "ATTACK") & (cool == 0) & (self.swt == 0) & (self.ammo >= self.cost())
        self.put("cool", live, torch.where(fire, torch.where(shotgun, self.SHOTGUN_CD, self.PISTOL_CD), cool))
        self.ammo = self.ammo - fire.long() * self.cost()
        key = self.aim()
        shot = (fire & (key < self.BIG))[:, None] & (self.kidx == (key % 8)[:, None])
        self.mhp = self.mhp - shot.long() * torch.where(shotgun, self.SHOTGUN_DMG, self.PISTOL_DMG)[:, None]
        dead = shot & (self.mhp <= 0)
        self.alive = self.alive & ~dead
        self.mt = torch.where(dead, torch.full_like(self.mt, self.RESPAWN), self.mt)
        reward = dead.long().sum(1)
        # monsters walk towards the player and stop at their distance; the melee ones bite there
        walk = live[:, None] & self.alive
        ox, oz = wx[:, None] - self.mx, wz[:, None] - self.mz
        far = torch.maximum(ox.abs(), oz.abs()) > self.stop
        self.mx = torch.where(walk & far, self.mx + self.MSPEED * ox.sign(), self.mx)
        self.mz = torch.where(walk & far, self.mz + self.MSPEED * oz.sign(), self.mz)
        biting = (walk & ~far & ~self.is_sh).long().sum(1)
        self.health = self.health - torch.where(self.tic % self.BITE == 0, biting * self.DAMAGE, 0 * biting)
        # fireballs: fly, arrive, and the throwers in range throw the next
        fly = live[:, None] & self.fact
        self.ft = torch.where(fly, self.ft - 1, self.ft)
        self.fx = torch.where(fly, self.fx + self.fvx, self.fx)
        self.fz = torch.where(fly, self.fz + self.fvz, self.fz)
        arrive = fly & (self.ft <= 0)
        burn = arrive & ((fdiv(self.fx, U) - wx[:, None]).abs() <= self.HIT) & \
            ((fdiv(self.fz, U) - wz[:, None]).abs() <= self.HIT)
        self.health = self.health - self.FDAMAGE * burn.long().sum(1)
        self.fact = self.fact & ~arrive
        tx, tz = self.mx[:, 1::2], self.mz[:, 1::2]
        near = torch.maximum((wx[:, None] - tx).abs(), (wz[:, None] - tz).abs()) <= self.FRANGE
        launch = walk[:, 1::2] & near & ~self.fact & ((self.tic[:, None] + self.FPHASE * self.jidx) % self.FIRE == 0)
        self.fx = torch.where(launch, tx * U, self.fx)
        self.fz = torch.where(launch, tz * U, self.fz)
        self.fvx = torch.where(launch, fdiv(self.px[:, None] - tx * U, self.FT), self.fvx)
        self.fvz = torch.where(launch, fdiv(self.pz[:, None] - tz * U, self.FT), self.fvz)
        self.ft = torch.where(launch, torch.full_like(self.ft, self.FT), self.ft)
        self.fact = self.fact | launch
        # pickups: take what is in reach, then the empty slots whose tic it is fill
        pick = live[:, None] & self.kact & ((self.kx - wx[:, None]).abs() <= self.PICK) & \
            ((self.kz - wz[:, None]).abs() <= self.PICK)
        self.health = torch.where(pick[:, 0], (self.health + self.HEAL).clamp(max=self.HMAX), self.health)
        self.ammo = torch.where(pick[:, 1], (self.ammo + self.AMMO_BOX).clamp(max=self.AMMO_MAX), self.ammo)
        self.has2 = self.has2 | pick[:, 2]
        self.kact = self.kact & ~pick
        span = 2 * self.KROOM + 1
        due = (self.tic[:, None] % self.PSPAWN) == self.PPHASE * self.pidx
        new = live[:, None] & due & ~self.kact & ((self.pidx != 2) | ~self.has2[:, None])
        nx = torch.stack([self.rand(130 + k, span) for k in range(self.NK)], 1)
        nz = torch.stack([self.rand(133 + k, span) for k in range(self.NK)], 1)
        self.kx = torch.where(new, (nx + self.tic[:, None] * self.KMULX) % span - self.KROOM, self.kx)
        self.kz = torch.where(new, (nz + self.tic[:, None] * self.KMULZ) % span - self.KROOM, self.kz)
        self.kact = self.kact | new
        # dead slots come back at their wall after RESPAWN tics
        wait = live[:, None] & ~self.alive
        self.mt = torch.where(wait, (self.mt - 1).clamp(min=0), self.mt)
        back = wait & (self.mt == 0)
        x, z = self.spawn_place(self.tic)
        self.alive = self.alive | back
        self.mx = torch.where(back, x, self.mx)
        self.mz = torch.where(back, z, self.mz)
        self.mhp = torch.where(back, torch.full_like(self.mhp, self.HP), self.mhp)
        return reward

    def game_over(self):
        return (self.health <= 0) | (self.tic >= self.TIMEOUT)

    def scene(self) -> Scene:
        sc = Scene(self.num_envs, self.device)
        self.backdrop(sc)
        px, pz = self.px[:, None], self.pz[:, None]
        dx, dz = self.view(self.post_x * U - px, self.post_z * U - pz)
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.POST_W, 2 * FH)
        sc.add_many(y0, x0, h, w, [PILLAR] * self.NP, visible=drawn)
        dx, dz = self.view(self.kx * U - px, self.kz * U - pz)
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.kw, self.kh)
        sc.add_many(y0, x0, h, w, [PICKUP] * self.NK, visible=drawn & self.kact)
        dx, dz = self.monsters_view()
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.mw, self.mh)
        sc.add_many(y0, x0, h, w, [MONSTER] * self.NM, visible=drawn & self.alive)
        dx, dz = self.view(self.fx - px, self.fz - pz)
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.FB_W, self.FB_H)
        sc.add_many(y0 - fdiv(self.FB_LIFT * K, dz.clamp(0, ZVIEW) + Z0), x0, h, w, [FIREBALL] * self.NF,
                    visible=drawn & self.fact)
        gw = torch.where(self.weapon == 1, self.GUN2_W, self.GUN_W)
        sc.add(HUD_Y0 - 20, 80 - fdiv(gw, 2), 20, gw, GUN)
        sc.add(HUD_Y0, 0, 210 - HUD_Y0, 160, HUD)
        sc.add(HUD_Y0 + 4, 8, 6, fdiv(self.health.clamp(min=0) * 3, 5), HBAR)
        sc.add(HUD_Y0 + 14, 8, 6, self.ammo.clamp(min=0) * 2, ABAR)
        return sc


DOOM_WORLD_GAMES = {"DoomMyWayHome": DoomMyWayHomeVec, "DoomPredictPosition": DoomPredictPositionVec,
                    "DoomDeathmatch": DoomDeathmatchVec}
GAMES.update(DOOM_WORLD_GAMES)
