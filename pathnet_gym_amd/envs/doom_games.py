"""Synthetic first-person Doom scenarios: DoomBasic, DoomDefendCenter, DoomTakeCover, DoomDefendLine,
DoomHealthGathering, DoomCorridor.

The reference's ``gym_doom`` levels need the ViZDoom engine (``envs/doom``, ids ``gym_doom/Doom*-v0``).  These
six are small on-device re-creations with the machinery of the synthetic Atari games (``envs/atari_games.py``):
integer dynamics, the counter-based RNG, a 210x160 RGB frame painted far to near from a fixed number of
rectangles, and the same logic in ``csrc/games.hip`` (game ids 5 to 10) with this torch code as the bit-exact
oracle (``tests/test_doom_games_hip.py``, ``tests/test_doom_nav_hip.py``).

* ``DoomBasic``        NOOP, ATTACK, MOVE_RIGHT, MOVE_LEFT.  The player strafes along the near wall; one monster
                       stands at the far wall.  A hit pays ``KILL`` and ends the episode, every shot costs ``SHOT``.
* ``DoomDefendCenter`` NOOP, ATTACK, TURN_RIGHT, TURN_LEFT.  The player turns in the centre of a round arena;
                       five monsters walk inward and bite at distance 0.  26 rounds; a kill pays +1.
* ``DoomTakeCover``    NOOP, MOVE_RIGHT, MOVE_LEFT.  Shooters at the far wall throw fireballs aimed at the
                       player's position at launch; the living reward counts the tics survived.
* ``DoomDefendLine``   NOOP, ATTACK, TURN_RIGHT, TURN_LEFT.  The player turns at the origin; six monsters walk down
                       their lanes from the far line, melee and fireball throwers by turns, and come back tougher.
                       Unlimited ammo; a kill pays +1, death -1.
* ``DoomHealthGathering`` NOOP, MOVE_FORWARD, TURN_RIGHT, TURN_LEFT.  The player walks a square room whose floor
                       hurts and picks up medkits; the living reward counts the tics survived, death costs 100.
* ``DoomCorridor``     NOOP, ATTACK, MOVE_RIGHT, MOVE_LEFT, MOVE_FORWARD, TURN_RIGHT, TURN_LEFT.  The player runs a
                       corridor past three pairs of shooting enemies to the vest at its end; the reward is the
                       progress along the corridor, death costs 100.

One ``physics()`` call is one Doom tic and an agent step is ``frameskip`` tics.  The scenario's
``episode_timeout`` counts tics, so every game keeps its own ``tic`` field; a finished episode (kill, death,
timeout) plays no further tic of its agent step, as ViZDoom's ``make_action`` stops at the episode's end.
``living_reward``, ``death_penalty``, ``episode_timeout`` and the button order come from the scenario table
(``envs/doom/scenarios.py``, ``envs/doom/constants.py``); what lives in the WADs (kill reward, shot cost,
damage, speeds, ammo) is set here and mirrored as ``static constexpr`` in ``csrc/games.hip``.

View: an object at lateral offset ``dx`` and depth ``z`` is drawn at x centre ``80 + dx * K // (z + Z0)`` with
width and height ``size * K // (z + Z0)``; its bottom edge stands on the floor, ``80 + FH * K // (z + Z0)``.
With K = 64, Z0 = 32 and depths in [0, 96] the scale runs from 1/2 (far wall) to 2 (at the player), so every
coordinate stays within a few hundred pixels of the screen.

Free view (``DoomNavVec``; the last three games): the player has a position ``(px, pz)`` in 1/U world units and a
heading ``th`` of 256 units a turn.  ``isin`` / ``icos`` read the quarter-wave table ``QSIN``; a world point at
offset ``(rx, rz)`` from the player is seen at ``dx = (rx icos - rz isin) // 256`` and depth
``dz = (rx isin + rz icos) // 256`` and drawn with the projection above when ``0 <= dz <= ZVIEW``; farther it is in
fog.  A shot hits the nearest living enemy whose drawn rectangle covers screen column ``COL``.  RNG streams: 50-57,
60-67, 70-72 (DoomHealthGathering), 80-85 (DoomDefendLine), 90 (DoomCorridor); 100-103 (DoomMyWayHome), 110-112
(DoomPredictPosition), 120-123, 130-135, 140 (DoomDeathmatch): ``envs/doom_world_games.py``.

Painter's order is fixed per rectangle slot: backdrop, posts, vest, enemies or kits, fireballs, HUD.  Posts stand
on the walls of a convex room, so whatever inside the room overlaps one on screen is nearer.  Objects of one layer
share one colour, so their order among themselves does not show.  The colours are the ten kinds above, reused: a
medkit is ``KIT`` = FIREBALL white, the vest ``VEST`` = SHOOTER green.  The kinds that can overlap on screen, each
pair at least 24 gray levels apart:

``DoomDefendLine``: PILLAR/CEIL PILLAR/FLOOR PILLAR/WALL MONSTER/PILLAR MONSTER/CEIL MONSTER/FLOOR MONSTER/WALL
FIREBALL/MONSTER FIREBALL/PILLAR FIREBALL/WALL FIREBALL/FLOOR FIREBALL/CEIL GUN/FLOOR GUN/MONSTER GUN/FIREBALL
HBAR/HUD (melee and throwers share MONSTER and differ in shape)

``DoomHealthGathering``: PILLAR/CEIL PILLAR/FLOOR PILLAR/WALL KIT/PILLAR KIT/FLOOR KIT/WALL HBAR/HUD

``DoomCorridor``: PILLAR/CEIL PILLAR/FLOOR PILLAR/WALL VEST/PILLAR VEST/FLOOR VEST/WALL MONSTER/VEST
MONSTER/PILLAR MONSTER/CEIL MONSTER/FLOOR MONSTER/WALL GUN/FLOOR GUN/MONSTER GUN/VEST HBAR/HUD ABAR/HUD

"""
from __future__ import annotations

import torch

from .atari_games import GAMES, PixelGameVec, Scene
from .doom.constants import ACTIONS, BUTTONS, CONFIG, DOOM_SETTINGS, LEVEL_NAMES
from .doom.scenarios import SCENARIOS

# projection
K, Z0, ZFAR = 64, 32, 96
HORIZON, FH = 80, 50                 # horizon row; half the room's height in world units
WALL_Y0, WALL_H = HORIZON - FH * K // (ZFAR + Z0), 2 * (FH * K // (ZFAR + Z0))     # far wall: rows 55..105
HUD_Y0 = 186

# colours by kind (cv2 luma in brackets): any two kinds that can overlap differ by at least 24
CEIL = (30, 30, 30)                  # 30
SIDE = (50, 55, 70)                  # 55
FLOOR = (84, 80, 70)                 # 80
HUD = (105, 105, 105)                # 105
WALL = (130, 130, 130)               # 130
GUN = (160, 155, 150)                # 156
PILLAR = (180, 180, 180)             # 180
SHOOTER = (200, 210, 190)            # 205
MONSTER = (255, 224, 200)            # 231
FIREBALL = (255, 255, 255)           # 255
HBAR = (230, 230, 230)               # 230 (over the HUD strip only)
ABAR = (180, 180, 180)               # 180 (over the HUD strip only)


def scenario(level: str):
    """(living_reward, death_penalty, episode_timeout, buttons) of a level from the scenario table."""
    row = DOOM_SETTINGS[LEVEL_NAMES.index(level)]
    spec = SCENARIOS[row[CONFIG]]
    buttons = [BUTTONS[i] for i in row[ACTIONS]]
    assert buttons == spec["buttons"], level
    living, death = spec.get("living_reward", 0), spec.get("death_penalty", 0)
    assert living == int(living) and death == int(death), level        # the driver sums integer rewards
    return int(living), int(death), int(spec["episode_timeout"]), buttons


def fdiv(a, b):
    return torch.div(a, b, rounding_mode="floor")


class DoomGameVec(PixelGameVec):
    """Shared parts of the scenarios: scenario constants, action lookup, backdrop and projection."""
    LEVEL = ""

    def init_state(self):
        self.LIVING, self.DEATH_PENALTY, self.TIMEOUT, self.BUTTONS = scenario(self.LEVEL)
        assert self.n_actions == 1 + len(self.BUTTONS)

    def button(self, a, name: str):
        """bool [N]: the action presses ``name`` (action 0 is NOOP, action 1 + i the level's i-th button)."""
        return a == 1 + self.BUTTONS.index(name)

    def zeros(self, *shape, dtype=torch.int64):
        return torch.zeros(self.num_envs, *shape, dtype=dtype, device=self.device)

    def put(self, name: str, live, new):
        """Commit ``new`` to a state tensor for the envs whose episode is still running."""
        old = getattr(self, name)
        m = live if old.dim() == 1 else live[:, None]
        setattr(self, name, torch.where(m, new.to(old.dtype), old))

    def backdrop(self, sc: Scene):
        sc.add(0, 0, HORIZON, 160, CEIL)
        sc.add(HORIZON, 0, HUD_Y0 - HORIZON, 160, FLOOR)
        sc.add(WALL_Y0, 0, WALL_H, 160, WALL)

    def hud(self, sc: Scene, health, ammo=None, gun: bool = False):
        if gun:
            sc.add(HUD_Y0 - 20, 74, 20, 12, GUN)
        sc.add(HUD_Y0, 0, 210 - HUD_Y0, 160, HUD)
        sc.add(HUD_Y0 + 4, 8, 6, fdiv(health.clamp(min=0) * 3, 5), HBAR)
        if ammo is not None:
            sc.add(HUD_Y0 + 14, 8, 6, ammo.clamp(min=0) * 2, ABAR)

    @staticmethod
    def project(dx, z, w: int, h: int):
        """(y0, x0, h, w) of an object of world size w x h standing on the floor at lateral offset dx, depth z."""
        den = z + Z0
        pw, ph = fdiv(torch.full_like(den, w * K), den), fdiv(torch.full_like(den, h * K), den)
        cx = 80 + fdiv(dx * K, den)
        yb = HORIZON + fdiv(torch.full_like(den, FH * K), den)
        return yb - ph, cx - fdiv(pw, 2), ph, pw

    def strafe_walls(self, sc: Scene, px):
        """Side-wall edges and two far-wall pillars at fixed world x, drawn at x - px: strafing is visible."""
        den = ZFAR + Z0
        el = 80 + fdiv((-self.ROOM - px) * K, den)
        er = 80 + fdiv((self.ROOM - px) * K, den)
        sc.add(WALL_Y0, el - 200, WALL_H, 200, SIDE)
        sc.add(WALL_Y0, er, WALL_H, 200, SIDE)
        for x in self.PILLARS:
            y0, x0, h, w = self.project(x - px, torch.full_like(px, ZFAR), 8, 2 * FH)
            sc.add(y0, x0, h, w, PILLAR)


# ===========================================================================
class DoomBasicVec(DoomGameVec):
    id = "DoomBasic"
    LEVEL = "DoomBasic"
    n_actions = 4
    reward_threshold = 10.0
    max_steps = 10000                      # the gym_doom registry's step limit; the tic timeout ends it long before
    HIP_GAME = "DoomBasic"
    HIP_FIELDS = (("px", "i"), ("mx", "i"), ("cool", "i"), ("tic", "i"), ("killed", "i"), ("ammo", "i"))
    XMAX, ROOM, SPEED = 100, 130, 4        # player / monster x in [-XMAX, XMAX]; side walls at +-ROOM
    PILLARS = (-50, 50)
    MON_W, MON_H, MON_HALF = 24, 40, 12    # monster size; a shot within MON_HALF of its centre hits
    KILL, SHOT, COOLDOWN, AMMO = 101, -5, 8, 50

    def init_state(self):
        super().init_state()
        self.px, self.mx, self.cool, self.tic, self.ammo = (self.zeros() for _ in range(5))
        self.killed = self.zeros(dtype=torch.bool)

    def reset_state(self, m):
        self.px = self.where_set(self.px, m, 0)
        self.mx = torch.where(m, self.rand(20, 2 * self.XMAX + 1) - self.XMAX, self.mx)
        self.cool = self.where_set(self.cool, m, 0)
        self.tic = self.where_set(self.tic, m, 0)
        self.ammo = self.where_set(self.ammo, m, self.AMMO)
        self.killed = self.killed & ~m

    def physics(self, a):
        live = ~self.game_over()
        right, left = self.button(a, "MOVE_RIGHT").long(), self.button(a, "MOVE_LEFT").long()
        self.put("tic", live, self.tic + 1)
        self.put("px", live, (self.px + self.SPEED * (right - left)).clamp(-self.XMAX, self.XMAX))
        cool = (self.cool - 1).clamp(min=0)
        fire = live & self.button(a, "ATTACK") & (cool == 0) & (self.ammo > 0)
        hit = fire & ((self.mx - self.px).abs() <= self.MON_HALF)
        self.put("cool", live, torch.where(fire, torch.full_like(cool, self.COOLDOWN), cool))
        self.ammo = self.ammo - fire.long()
        self.killed = self.killed | hit
        return live.long() * self.LIVING + fire.long() * self.SHOT + hit.long() * self.KILL

    def game_over(self):
        return self.killed | (self.tic >= self.TIMEOUT)

    def scene(self) -> Scene:
        sc = Scene(self.num_envs, self.device)
        self.backdrop(sc)
        self.strafe_walls(sc, self.px)
        y0, x0, h, w = self.project(self.mx - self.px, torch.full_like(self.px, ZFAR), self.MON_W, self.MON_H)
        sc.add(y0, x0, h, w, MONSTER, visible=~self.killed)
        self.hud(sc, torch.full_like(self.px, 100), self.ammo, gun=True)
        return sc


# ===========================================================================
class DoomDefendCenterVec(DoomGameVec):
    id = "DoomDefendCenter"
    LEVEL = "DoomDefendCenter"
    n_actions = 4
    reward_threshold = 10.0
    max_steps = 10000
    HIP_GAME = "DoomDefendCenter"
    HIP_FIELDS = (("th", "i"), ("cool", "i"), ("ammo", "i"), ("health", "i"), ("tic", "i"), ("ma", "vec"),
                  ("md", "vec"), ("mt", "vec"), ("alive", "mask"))
    NM, NP = 5, 8                          # monsters; wall pillars at world angles 32 k
    TURN, FOV = 3, 64                      # heading units (of 256 a turn) per tic; field of view
    DMAX, STAGGER = 96, 8                  # spawn distance; monster k starts STAGGER * k closer
    MON_W, MON_H = 16, 40
    TOL0, TOLDIV = 6, 8                    # aim tolerance TOL0 + (DMAX - md) // TOLDIV heading units
    COOLDOWN, AMMO, RESPAWN = 8, 26, 16
    BITE, DAMAGE, HEALTH = 8, 10, 100

    def init_state(self):
        super().init_state()
        self.th, self.cool, self.ammo, self.health, self.tic = (self.zeros() for _ in range(5))
        self.ma, self.md, self.mt = (self.zeros(self.NM) for _ in range(3))
        self.alive = self.zeros(self.NM, dtype=torch.bool)
        self.kidx = torch.arange(self.NM, device=self.device)[None]

    def spawn_angle(self, tic):
        """[N, NM] random angles: the RNG counter moves once per agent step, the tic separates a step's tics."""
        r = torch.stack([self.rand(30 + k, 256) for k in range(self.NM)], 1)
        return (r + tic[:, None] * 41) % 256

    def reset_state(self, m):
        for name, v in (("th", 0), ("cool", 0), ("ammo", self.AMMO), ("health", self.HEALTH), ("tic", 0)):
            setattr(self, name, self.where_set(getattr(self, name), m, v))
        mm = m[:, None]
        self.ma = torch.where(mm, self.spawn_angle(torch.zeros_like(self.tic)), self.ma)
        self.md = torch.where(mm, (self.DMAX - self.STAGGER * self.kidx).expand_as(self.md), self.md)
        self.mt = torch.where(mm, torch.zeros_like(self.mt), self.mt)
        self.alive = self.alive | mm

    def offsets(self, ang):
        """Wrapped angular offset of world angle(s) [N, k] from the heading, in [-128, 128)."""
        return (ang - self.th[:, None] + 128) % 256 - 128

    def tolerance(self):
        return self.TOL0 + fdiv(self.DMAX - self.md, self.TOLDIV)

    def physics(self, a):
        live = ~self.game_over()
        right, left = self.button(a, "TURN_RIGHT").long(), self.button(a, "TURN_LEFT").long()
        self.put("tic", live, self.tic + 1)
        self.put("th", live, (self.th + self.TURN * (right - left)) % 256)
        cool = (self.cool - 1).clamp(min=0)
        fire = live & self.button(a, "ATTACK") & (cool == 0) & (self.ammo > 0)
        self.put("cool", live, torch.where(fire, torch.full_like(cool, self.COOLDOWN), cool))
        self.ammo = self.ammo - fire.long()
        # the shot kills the nearest living monster inside its aim tolerance (ties: the lowest index)
        BIG = 1 << 20
        cand = self.alive & (self.offsets(self.ma).abs() <= self.tolerance())
        key = torch.where(cand, self.md * 8 + self.kidx, torch.full_like(self.md, BIG)).min(1).values
        kill = fire & (key < BIG)
        dead = kill[:, None] & (self.kidx == (key % 8)[:, None])
        self.alive = self.alive & ~dead
        self.mt = torch.where(dead, torch.full_like(self.mt, self.RESPAWN), self.mt)
        reward = kill.long()
        # walk inward, bite at distance 0
        walk = live[:, None] & self.alive
        self.md = torch.where(walk, (self.md - 1).clamp(min=0), self.md)
        biting = (walk & (self.md == 0)).long().sum(1)
        self.health = self.health - torch.where(self.tic % self.BITE == 0, biting * self.DAMAGE, 0 * biting)
        # dead slots come back at the rim after RESPAWN tics
        wait = live[:, None] & ~self.alive
        self.mt = torch.where(wait, (self.mt - 1).clamp(min=0), self.mt)
        back = wait & (self.mt == 0)
        self.alive = self.alive | back
        self.md = torch.where(back, torch.full_like(self.md, self.DMAX), self.md)
        self.ma = torch.where(back, self.spawn_angle(self.tic), self.ma)
        died = live & (self.health <= 0)
        return reward - died.long() * self.DEATH_PENALTY

    def game_over(self):
        return (self.health <= 0) | (self.tic >= self.TIMEOUT) | ((self.ammo <= 0) & (self.cool <= 0))

    def scene(self) -> Scene:
        sc = Scene(self.num_envs, self.device)
        self.backdrop(sc)
        pang = 32 * torch.arange(self.NP, device=self.device)[None].expand(self.num_envs, self.NP)
        far = torch.full_like(pang, ZFAR)
        y0, x0, h, w = self.project(0 * pang, far, 8, 2 * FH)
        sc.add_many(y0, 80 + fdiv(self.offsets(pang) * 5, 2) - w // 2, h, w, [PILLAR] * self.NP)
        y0, x0, h, w = self.project(0 * self.md, self.md, self.MON_W, self.MON_H)
        sc.add_many(y0, 80 + fdiv(self.offsets(self.ma) * 5, 2) - w // 2, h, w, [MONSTER] * self.NM,
                    visible=self.alive)
        self.hud(sc, self.health, self.ammo, gun=True)
        return sc


# ===========================================================================
class DoomTakeCoverVec(DoomGameVec):
    id = "DoomTakeCover"
    LEVEL = "DoomTakeCover"
    n_actions = 3
    reward_threshold = 750.0
    max_steps = 10000
    HIP_GAME = "DoomTakeCover"
    HIP_FIELDS = (("px", "i"), ("health", "i"), ("tic", "i"), ("fx", "vec"), ("fz", "vec"), ("fvx", "vec"),
                  ("fact", "mask"))
    XMAX, ROOM, SPEED = 100, 130, 4
    PILLARS = (-50, 50)
    NSH, NF = 6, 6                         # shooters (at most), fireball slots
    SHOOTER_X = (-18, 54, -90, 90, -54, 18)        # in the order the shooters appear
    SH_W, SH_H = 16, 40
    GROW, FIRE = 200, 8                    # one more shooter every GROW tics; a launch every FIRE tics
    U = 16                                 # fireball x is in 1/16 world units
    FSPEED = 8                             # depth units per tic: ZFAR / FSPEED tics of flight
    FB_W, FB_H, FB_LIFT = 12, 12, 25       # fireball size, height of its lower edge above the floor
    HIT_W, DAMAGE, HEALTH = 12, 20, 100

    def init_state(self):
        super().init_state()
        self.px, self.health, self.tic = (self.zeros() for _ in range(3))
        self.fx, self.fz, self.fvx = (self.zeros(self.NF) for _ in range(3))
        self.fact = self.zeros(self.NF, dtype=torch.bool)
        self.kidx = torch.arange(self.NF, device=self.device)[None]
        self.shx = torch.tensor(self.SHOOTER_X, dtype=torch.int64, device=self.device)

    def reset_state(self, m):
        for name, v in (("px", 0), ("health", self.HEALTH), ("tic", 0)):
            setattr(self, name, self.where_set(getattr(self, name), m, v))
        self.fact = self.fact & ~m[:, None]

    def shooters(self):
        return (1 + fdiv(self.tic, self.GROW)).clamp(max=self.NSH)

    def physics(self, a):
        live = ~self.game_over()
        right, left = self.button(a, "MOVE_RIGHT").long(), self.button(a, "MOVE_LEFT").long()
        self.put("tic", live, self.tic + 1)
        self.put("px", live, (self.px + self.SPEED * (right - left)).clamp(-self.XMAX, self.XMAX))
        # fireballs in flight
        fly = live[:, None] & self.fact
        self.fz = torch.where(fly, self.fz - self.FSPEED, self.fz)
        self.fx = torch.where(fly, self.fx + self.fvx, self.fx)
        arrive = fly & (self.fz <= 0)
        hit = arrive & ((fdiv(self.fx, self.U) - self.px[:, None]).abs() <= self.HIT_W)
        self.health = self.health - self.DAMAGE * hit.long().sum(1)
        self.fact = self.fact & ~arrive
        # a shooter throws the next one into the lowest idle slot, aimed at where the player stands now
        idle = torch.where(~self.fact, self.kidx, self.NF).min(1).values
        launch = live & (self.tic % self.FIRE == 0) & (idle < self.NF)
        sx = self.shx[(self.rand(40, self.NSH) + fdiv(self.tic, self.FIRE)) % self.shooters()]
        new = launch[:, None] & (self.kidx == idle[:, None])
        self.fx = torch.where(new, (sx * self.U)[:, None], self.fx)
        self.fz = torch.where(new, torch.full_like(self.fz, ZFAR), self.fz)
        self.fvx = torch.where(new, fdiv((self.px - sx) * self.U, ZFAR // self.FSPEED)[:, None], self.fvx)
        self.fact = self.fact | new
        return live.long() * self.LIVING

    def game_over(self):
        return (self.health <= 0) | (self.tic >= self.TIMEOUT)

    def scene(self) -> Scene:
        sc = Scene(self.num_envs, self.device)
        self.backdrop(sc)
        self.strafe_walls(sc, self.px)
        sdx = self.shx[None] - self.px[:, None]
        y0, x0, h, w = self.project(sdx, torch.full_like(sdx, ZFAR), self.SH_W, self.SH_H)
        sidx = torch.arange(self.NSH, device=self.device)[None]
        sc.add_many(y0, x0, h, w, [SHOOTER] * self.NSH, visible=sidx < self.shooters()[:, None])
        z = self.fz.clamp(min=0)
        y0, x0, h, w = self.project(fdiv(self.fx, self.U) - self.px[:, None], z, self.FB_W, self.FB_H)
        sc.add_many(y0 - fdiv(self.FB_LIFT * K, z + Z0), x0, h, w, [FIREBALL] * self.NF, visible=self.fact)
        self.hud(sc, self.health)
        return sc


# ===========================================================================
# free view: a player with a position and a heading in a room
U = 16                                 # positions are in 1/U world units
ZVIEW = 160                            # view depth: beyond it an object is in fog (12 * K // (ZVIEW + Z0) = 4 px)
COL = 80                               # the sights' screen column
DXMAX = 512                            # lateral offsets are clamped here: off screen at every depth
QSIN = (0, 6, 13, 19, 25, 31, 38, 44, 50, 56, 62, 68, 74, 80, 86, 92, 98, 104, 109, 115, 121, 126, 132, 137, 142,
        147, 152, 157, 162, 167, 172, 177, 181, 185, 190, 194, 198, 202, 206, 209, 213, 216, 220, 223, 226, 229,
        231, 234, 237, 239, 241, 243, 245, 247, 248, 250, 251, 252, 253, 254, 255, 255, 256, 256, 256)
KIT = FIREBALL                         # medkit: over FLOOR, WALL and PILLAR only
VEST = SHOOTER                         # armour: over FLOOR, WALL and PILLAR; under MONSTER


class DoomNavVec(DoomGameVec):
    """Shared parts of the free-view scenarios: integer trig, the view transform, the hit-scan rule.

    The heading ``th`` has 256 units a turn, 0 looks along +z and positive turns right, so the forward vector is
    ``(isin, icos) / 256`` and the right vector ``(icos, -isin) / 256``.
    """
    SCALE = U                              # sub-units per world unit of the positions given to ``view``
    BIG = 1 << 20                          # hit-scan key of an empty sights' column

    def init_state(self):
        super().init_state()
        self.qsin = torch.tensor(QSIN, dtype=torch.int64, device=self.device)

    def isin(self, h):
        h = h % 256
        k = h % 128
        q = self.qsin[torch.where(k <= 64, k, 128 - k)]
        return torch.where(h >= 128, -q, q)

    def icos(self, h):
        return self.isin(h + 64)

    def view(self, rx, rz):
        """(dx, dz) in whole world units of the offset (rx, rz) [N] or [N, k] from the player, in 1/SCALE units.

        int32 bound (the HIP row is int): |rx|, |rz| <= 2^14 (the longest room is DoomCorridor's, 1000 * 16
        sub-units) and |isin|, |icos| <= 2^8, so each product is at most 2^22 and their sum at most 2^23.
        """
        th = self.th if rx.dim() == 1 else self.th[:, None]
        s, c = self.isin(th), self.icos(th)
        return fdiv(rx * c - rz * s, 256 * self.SCALE), fdiv(rx * s + rz * c, 256 * self.SCALE)

    @staticmethod
    def nav_project(dx, dz, w, h):
        """(y0, x0, h, w, drawn): ``project`` for a view offset; drawn only with 0 <= dz <= ZVIEW."""
        drawn = (dz >= 0) & (dz <= ZVIEW)
        den = dz.clamp(0, ZVIEW) + Z0
        pw, ph = fdiv(0 * den + w * K, den), fdiv(0 * den + h * K, den)
        cx = 80 + fdiv(dx.clamp(-DXMAX, DXMAX) * K, den)
        yb = HORIZON + fdiv(0 * den + FH * K, den)
        return yb - ph, cx - fdiv(pw, 2), ph, pw, drawn

    def sights(self, dx, dz, w, alive):
        """Hit-scan key [N]: dz * 8 + index of the nearest living enemy that is drawn and whose rectangle covers
        column COL (ties: the lowest index), BIG when the column is free."""
        _, x0, _, pw, drawn = self.nav_project(dx, dz, w, 1)
        cover = alive & drawn & (x0 <= COL) & (COL < x0 + pw)
        return torch.where(cover, dz * 8 + self.kidx, torch.full_like(dz, self.BIG)).min(1).values

    def heading_step(self, a):
        return self.TURN * (self.button(a, "TURN_RIGHT").long() - self.button(a, "TURN_LEFT").long())


# ===========================================================================
class DoomDefendLineVec(DoomNavVec):
    """The player stands at the origin and turns within +-TH_MAX; NM monsters walk down their lanes from the far
    line z = DMAX (slot k at ``LANE_X[k] * md / DMAX``, depth ``md``; the start is staggered by up to STAGGER).

    Even slots are melee: at md = 0 each bites for DAMAGE every BITE tics.  Odd slots are shooters: they stop at
    md = STANDOFF and every FIRE tics (phase FPHASE per shooter) throw a fireball into their own slot; it flies
    FSPEED per tic down the lane and takes FDAMAGE on arrival, whatever the player does.  ATTACK (every COOLDOWN
    tics, unlimited ammo) takes one hit point from the monster in the sights (``DoomNavVec.sights``, widths MON_W /
    SH_W); at zero the kill pays +1 and the slot comes back at DMAX after RESPAWN tics with
    ``min(1 + kills of the slot, HP_MAX)`` hit points.  Posts stand on the far line at multiples of POST_GAP.
    """
    id = "DoomDefendLine"
    LEVEL = "DoomDefendLine"
    n_actions = 4
    reward_threshold = 15.0
    max_steps = 10000
    HIP_GAME = "DoomDefendLine"
    HIP_FIELDS = (("th", "i"), ("cool", "i"), ("health", "i"), ("tic", "i"), ("md", "vec"), ("mhp", "vec"),
                  ("mt", "vec"), ("mk", "vec"), ("fd", "vec"), ("alive", "mask"), ("fact", "mask"))
    SCALE = 1                              # monsters and posts are in whole world units
    NM, NF, NP = 6, 3, 5
    LANE_X = (-100, -60, -20, 20, 60, 100)
    TURN, TH_MAX = 2, 40
    DMAX, STAGGER, STANDOFF = 96, 32, 48
    MON_W, MON_H, SH_W, SH_H = 24, 40, 20, 48
    POST_W, POST_GAP = 12, 48
    COOLDOWN, RESPAWN, HP_MAX = 8, 16, 3
    BITE, DAMAGE, HEALTH = 8, 10, 100
    FIRE, FPHASE, FSPEED, FDAMAGE = 24, 8, 4, 6
    FB_W, FB_H, FB_LIFT = 12, 12, 25

    def init_state(self):
        super().init_state()
        self.th, self.cool, self.health, self.tic = (self.zeros() for _ in range(4))
        self.md, self.mhp, self.mt, self.mk = (self.zeros(self.NM) for _ in range(4))
        self.fd = self.zeros(self.NF)
        self.alive = self.zeros(self.NM, dtype=torch.bool)
        self.fact = self.zeros(self.NF, dtype=torch.bool)
        dev = self.device
        self.kidx = torch.arange(self.NM, device=dev)[None]
        self.jidx = torch.arange(self.NF, device=dev)[None]
        self.lane_x = torch.tensor(self.LANE_X, dtype=torch.int64, device=dev)[None]
        self.is_sh = (self.kidx % 2) == 1
        self.mw = torch.where(self.is_sh, self.SH_W, self.MON_W)
        self.mh = torch.where(self.is_sh, self.SH_H, self.MON_H)
        self.post_x = (torch.arange(self.NP, device=dev)[None] - self.NP // 2) * self.POST_GAP

    def reset_state(self, m):
        for name, v in (("th", 0), ("cool", 0), ("health", self.HEALTH), ("tic", 0)):
            setattr(self, name, self.where_set(getattr(self, name), m, v))
        mm = m[:, None]
        start = self.DMAX - torch.stack([self.rand(80 + k, self.STAGGER) for k in range(self.NM)], 1)
        self.md = torch.where(mm, start, self.md)
        self.mhp = torch.where(mm, torch.ones_like(self.mhp), self.mhp)
        self.mt = torch.where(mm, torch.zeros_like(self.mt), self.mt)
        self.mk = torch.where(mm, torch.zeros_like(self.mk), self.mk)
        self.fd = torch.where(mm, torch.zeros_like(self.fd), self.fd)
        self.alive = self.alive | mm
        self.fact = self.fact & ~mm

    def monsters_view(self):
        return self.view(fdiv(self.lane_x * self.md, self.DMAX), self.md)

    def aim(self):
        """The hit-scan key of the monsters as they stand (BIG: nothing in the sights)."""
        dx, dz = self.monsters_view()
        return self.sights(dx, dz, self.mw, self.alive)

    def physics(self, a):
        live = ~self.game_over()
        self.put("tic", live, self.tic + 1)
        self.put("th", live, (self.th + self.heading_step(a)).clamp(-self.TH_MAX, self.TH_MAX))
        cool = (self.cool - 1).clamp(min=0)
        fire = live & self.button(a, "ATTACK") & (cool == 0)
        self.put("cool", live, torch.where(fire, torch.full_like(cool, self.COOLDOWN), cool))
        key = self.aim()
        shot = (fire & (key < self.BIG))[:, None] & (self.kidx == (key % 8)[:, None])
        self.mhp = self.mhp - shot.long()
        dead = shot & (self.mhp <= 0)
        self.alive = self.alive & ~dead
        self.mt = torch.where(dead, torch.full_like(self.mt, self.RESPAWN), self.mt)
        self.mk = self.mk + dead.long()
        reward = dead.long().sum(1)
        # walk down the lane: melee to the player, shooters to their stand-off
        walk = live[:, None] & self.alive
        stop = self.is_sh.long() * self.STANDOFF
        self.md = torch.where(walk, torch.maximum(self.md - 1, stop), self.md)
        biting = (walk & ~self.is_sh & (self.md == 0)).long().sum(1)
        self.health = self.health - torch.where(self.tic % self.BITE == 0, biting * self.DAMAGE, 0 * biting)
        # fireballs: fly, arrive, and the shooters at their stand-off throw the next
        fly = live[:, None] & self.fact
        self.fd = torch.where(fly, self.fd - self.FSPEED, self.fd)
        arrive = fly & (self.fd <= 0)
        self.health = self.health - self.FDAMAGE * arrive.long().sum(1)
        self.fact = self.fact & ~arrive
        launch = walk[:, 1::2] & (self.md[:, 1::2] == self.STANDOFF) & ~self.fact & \
            ((self.tic[:, None] + self.FPHASE * self.jidx) % self.FIRE == 0)
        self.fd = torch.where(launch, torch.full_like(self.fd, self.STANDOFF), self.fd)
        self.fact = self.fact | launch
        # dead slots come back at the far line after RESPAWN tics, tougher
        wait = live[:, None] & ~self.alive
        self.mt = torch.where(wait, (self.mt - 1).clamp(min=0), self.mt)
        back = wait & (self.mt == 0)
        self.alive = self.alive | back
        self.md = torch.where(back, torch.full_like(self.md, self.DMAX), self.md)
        self.mhp = torch.where(back, (1 + self.mk).clamp(max=self.HP_MAX), self.mhp)
        died = live & (self.health <= 0)
        return reward - died.long() * self.DEATH_PENALTY

    def game_over(self):
        return (self.health <= 0) | (self.tic >= self.TIMEOUT)

    def scene(self) -> Scene:
        sc = Scene(self.num_envs, self.device)
        self.backdrop(sc)
        dx, dz = self.view(self.post_x.expand(self.num_envs, self.NP), torch.full_like(self.md[:, :self.NP], self.DMAX))
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.POST_W, 2 * FH)
        sc.add_many(y0, x0, h, w, [PILLAR] * self.NP, visible=drawn)
        dx, dz = self.monsters_view()
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.mw, self.mh)
        sc.add_many(y0, x0, h, w, [MONSTER] * self.NM, visible=drawn & self.alive)
        fd = self.fd.clamp(min=0)
        dx, dz = self.view(fdiv(self.lane_x[:, 1::2] * fd, self.DMAX), fd)
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.FB_W, self.FB_H)
        sc.add_many(y0 - fdiv(self.FB_LIFT * K, dz.clamp(0, ZVIEW) + Z0), x0, h, w, [FIREBALL] * self.NF,
                    visible=drawn & self.fact)
        self.hud(sc, self.health, None, gun=True)
        return sc


# ===========================================================================
class DoomHealthGatheringVec(DoomNavVec):
    """A square room |x|, |z| <= ROOM with an acid floor: ACID_DMG every ACID tics.  MOVE_FORWARD walks SPEED per
    tic along the heading (TURN units per tic), clamped to the room.  NK medkit slots: KIT0 kits at reset, and
    every SPAWN tics the lowest empty slot gets one at a random place within KROOM of the centre.  Standing within
    PICK of a kit on both axes takes it: ``health = min(health + HEAL, HMAX)``.  The living reward is the score; no
    weapon.  Eight posts (POST_W wide) stand at the corners and the middles of the walls.
    """
    id = "DoomHealthGathering"
    LEVEL = "DoomHealthGathering"
    n_actions = 4
    reward_threshold = 1000.0
    max_steps = 10000
    HIP_GAME = "DoomHealthGathering"
    HIP_FIELDS = (("px", "i"), ("pz", "i"), ("th", "i"), ("health", "i"), ("tic", "i"), ("kx", "vec"), ("kz", "vec"),
                  ("kact", "mask"))
    NK, KIT0, NP = 8, 4, 8
    ROOM, KROOM, SPEED, TURN = 96, 88, 4, 4
    ACID, ACID_DMG, SPAWN = 16, 8, 32
    PICK, HEAL, HMAX, HEALTH = 12, 25, 100, 100
    KIT_W, KIT_H, POST_W = 12, 12, 12
    KMULX, KMULZ = 37, 59                  # odd multipliers of the tic in the spawn position's key

    def init_state(self):
        super().init_state()
        self.px, self.pz, self.th, self.health, self.tic = (self.zeros() for _ in range(5))
        self.kx, self.kz = self.zeros(self.NK), self.zeros(self.NK)
        self.kact = self.zeros(self.NK, dtype=torch.bool)
        dev, R = self.device, self.ROOM
        self.kidx = torch.arange(self.NK, device=dev)[None]
        posts = ((-R, -R), (0, -R), (R, -R), (R, 0), (R, R), (0, R), (-R, R), (-R, 0))
        self.post_x = torch.tensor([p[0] for p in posts], dtype=torch.int64, device=dev)[None]
        self.post_z = torch.tensor([p[1] for p in posts], dtype=torch.int64, device=dev)[None]

    def reset_state(self, m):
        for name, v in (("px", 0), ("pz", 0), ("health", self.HEALTH), ("tic", 0)):
            setattr(self, name, self.where_set(getattr(self, name), m, v))
        self.th = torch.where(m, self.rand(72, 256), self.th)
        span = 2 * self.KROOM + 1
        first = m[:, None] & (self.kidx < self.KIT0)
        rx = torch.stack([self.rand(50 + k, span) for k in range(self.NK)], 1) - self.KROOM
        rz = torch.stack([self.rand(60 + k, span) for k in range(self.NK)], 1) - self.KROOM
        self.kx = torch.where(first, rx, torch.where(m[:, None], torch.zeros_like(self.kx), self.kx))
        self.kz = torch.where(first, rz, torch.where(m[:, None], torch.zeros_like(self.kz), self.kz))
        self.kact = torch.where(m[:, None], first, self.kact)

    def physics(self, a):
        live = ~self.game_over()
        self.put("tic", live, self.tic + 1)
        self.put("th", live, (self.th + self.heading_step(a)) % 256)
        fwd = self.button(a, "MOVE_FORWARD").long() * self.SPEED * U
        lim = self.ROOM * U
        self.put("px", live, (self.px + fdiv(fwd * self.isin(self.th), 256)).clamp(-lim, lim))
        self.put("pz", live, (self.pz + fdiv(fwd * self.icos(self.th), 256)).clamp(-lim, lim))
        wx, wz = fdiv(self.px, U)[:, None], fdiv(self.pz, U)[:, None]
        pick = live[:, None] & self.kact & ((self.kx - wx).abs() <= self.PICK) & ((self.kz - wz).abs() <= self.PICK)
        self.health = torch.where(pick.any(1), (self.health + self.HEAL * pick.long().sum(1)).clamp(max=self.HMAX),
                                  self.health)
        self.kact = self.kact & ~pick
        self.health = self.health - (live & (self.tic % self.ACID == 0)).long() * self.ACID_DMG
        # a new kit into the lowest empty slot
        empty = torch.where(~self.kact, self.kidx, self.NK).min(1).values
        new = (live & (self.tic % self.SPAWN == 0))[:, None] & (self.kidx == empty[:, None])
        span = 2 * self.KROOM + 1
        nx = (self.rand(70, span) + self.tic * self.KMULX) % span - self.KROOM
        nz = (self.rand(71, span) + self.tic * self.KMULZ) % span - self.KROOM
        self.kx = torch.where(new, nx[:, None], self.kx)
        self.kz = torch.where(new, nz[:, None], self.kz)
        self.kact = self.kact | new
        died = live & (self.health <= 0)
        return live.long() * self.LIVING - died.long() * self.DEATH_PENALTY

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
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.KIT_W, self.KIT_H)
        sc.add_many(y0, x0, h, w, [KIT] * self.NK, visible=drawn & self.kact)
        self.hud(sc, self.health)
        return sc


# ===========================================================================
class DoomCorridorVec(DoomNavVec):
    """A corridor |x| <= HALFW, 0 <= z <= LEN; the player starts at (0, 0) looking along it and the vest lies at
    (0, LEN).  The reward of a tic is the whole-unit progress ``pz_new // U - pz_old // U``; being within TOUCH of
    the vest on both axes ends the episode.  MOVE_FORWARD / MOVE_RIGHT / MOVE_LEFT walk SPEED per tic along or
    across the heading (TURN units per tic).  Six enemies stand in pairs at z = GROUP_Z[g], x = -+ENEMY_X; a living
    one within RANGE of the player along z shoots every EFIRE tics (phase EPHASE per index) and takes EDMG unless the
    shot is the one in EMISS that misses (RNG stream 90, keyed by the tic and the index).  ATTACK
    (AMMO rounds, every COOLDOWN tics) kills the enemy in the sights (``DoomNavVec.sights``, width EN_W).  NPOST
    posts a side at multiples of POST_GAP slide with the player.
    """
    id = "DoomCorridor"
    LEVEL = "DoomCorridor"
    n_actions = 7
    reward_threshold = 1000.0
    max_steps = 10000
    HIP_GAME = "DoomCorridor"
    HIP_FIELDS = (("px", "i"), ("pz", "i"), ("th", "i"), ("health", "i"), ("ammo", "i"), ("cool", "i"), ("tic", "i"),
                  ("won", "i"), ("alive", "mask"))
    NE, NPOST = 6, 5
    HALFW, LEN, SPEED, TURN = 56, 1000, 4, 2
    GROUP_Z = (250, 500, 750)
    ENEMY_X, EN_W, EN_H = 40, 24, 40
    RANGE, EFIRE, EPHASE, EDMG, EMISS = 160, 20, 3, 8, 4
    COOLDOWN, AMMO, HEALTH, TOUCH = 8, 26, 100, 24
    POST_W, POST_GAP = 12, 40
    VEST_W, VEST_H = 16, 16

    def init_state(self):
        super().init_state()
        self.px, self.pz, self.th, self.health, self.ammo, self.cool, self.tic = (self.zeros() for _ in range(7))
        self.won = self.zeros(dtype=torch.bool)
        self.alive = self.zeros(self.NE, dtype=torch.bool)
        dev = self.device
        self.kidx = torch.arange(self.NE, device=dev)[None]
        self.ex = ((self.kidx % 2) * 2 - 1) * self.ENEMY_X
        self.ez = torch.tensor([self.GROUP_Z[i // 2] for i in range(self.NE)], dtype=torch.int64, device=dev)[None]
        self.pidx = torch.arange(self.NPOST, device=dev)[None]

    def reset_state(self, m):
        for name, v in (("px", 0), ("pz", 0), ("th", 0), ("health", self.HEALTH), ("ammo", self.AMMO), ("cool", 0),
                        ("tic", 0)):
            setattr(self, name, self.where_set(getattr(self, name), m, v))
        self.won = self.won & ~m
        self.alive = self.alive | m[:, None]

    def enemies_view(self):
        return self.view(self.ex * U - self.px[:, None], self.ez * U - self.pz[:, None])

    def aim(self):
        dx, dz = self.enemies_view()
        return self.sights(dx, dz, self.EN_W, self.alive)

    def physics(self, a):
        live = ~self.game_over()
        self.put("tic", live, self.tic + 1)
        self.put("th", live, (self.th + self.heading_step(a)) % 256)
        fwd = self.button(a, "MOVE_FORWARD").long()
        side = self.button(a, "MOVE_RIGHT").long() - self.button(a, "MOVE_LEFT").long()
        s, c = self.isin(self.th), self.icos(self.th)
        step = self.SPEED * U
        old = fdiv(self.pz, U)
        self.put("px", live, (self.px + fdiv(step * (fwd * s + side * c), 256)).clamp(-self.HALFW * U, self.HALFW * U))
        self.put("pz", live, (self.pz + fdiv(step * (fwd * c - side * s), 256)).clamp(0, self.LEN * U))
        wx, wz = fdiv(self.px, U), fdiv(self.pz, U)
        reward = wz - old
        cool = (self.cool - 1).clamp(min=0)
        fire = live & self.button(a, "ATTACK") & (cool == 0) & (self.ammo > 0)
        self.put("cool", live, torch.where(fire, torch.full_like(cool, self.COOLDOWN), cool))
        self.ammo = self.ammo - fire.long()
        key = self.aim()
        dead = (fire & (key < self.BIG))[:, None] & (self.kidx == (key % 8)[:, None])
        self.alive = self.alive & ~dead
        shoot = live[:, None] & self.alive & ((self.ez - wz[:, None]).abs() <= self.RANGE) & \
            ((self.tic[:, None] + self.EPHASE * self.kidx) % self.EFIRE == 0) & \
            ((self.rand(90, self.EMISS)[:, None] + self.tic[:, None] * 41 + self.kidx * 3) % self.EMISS != 0)
        self.health = self.health - self.EDMG * shoot.long().sum(1)
        self.won = self.won | (live & (wx.abs() <= self.TOUCH) & (self.LEN - wz <= self.TOUCH))
        died = live & (self.health <= 0)
        return reward - died.long() * self.DEATH_PENALTY

    def game_over(self):
        return self.won | (self.health <= 0) | (self.tic >= self.TIMEOUT)

    def scene(self) -> Scene:
        sc = Scene(self.num_envs, self.device)
        self.backdrop(sc)
        px, pz = self.px[:, None], self.pz[:, None]
        zj = (fdiv(fdiv(self.pz, U), self.POST_GAP)[:, None] - 1 + self.pidx) * self.POST_GAP
        inside = (zj >= 0) & (zj <= self.LEN)
        for x in (-self.HALFW, self.HALFW):
            dx, dz = self.view(x * U - px + 0 * zj, zj * U - pz)
            y0, x0, h, w, drawn = self.nav_project(dx, dz, self.POST_W, 2 * FH)
            sc.add_many(y0, x0, h, w, [PILLAR] * self.NPOST, visible=drawn & inside)
        dx, dz = self.view(-self.px, self.LEN * U - self.pz)
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.VEST_W, self.VEST_H)
        sc.add(y0, x0, h, w, VEST, visible=drawn)
        dx, dz = self.enemies_view()
        y0, x0, h, w, drawn = self.nav_project(dx, dz, self.EN_W, self.EN_H)
        sc.add_many(y0, x0, h, w, [MONSTER] * self.NE, visible=drawn & self.alive)
        self.hud(sc, self.health, self.ammo, gun=True)
        return sc


DOOM_GAMES = {"DoomBasic": DoomBasicVec, "DoomDefendCenter": DoomDefendCenterVec, "DoomTakeCover": DoomTakeCoverVec,
              "DoomDefendLine": DoomDefendLineVec, "DoomHealthGathering": DoomHealthGatheringVec,
              "DoomCorridor": DoomCorridorVec}
GAMES.update(DOOM_GAMES)

from . import doom_world_games  # noqa: E402,F401  (adds DoomMyWayHome, DoomPredictPosition, DoomDeathmatch to GAMES)
