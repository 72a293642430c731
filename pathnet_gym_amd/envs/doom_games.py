"""Synthetic first-person Doom scenarios: DoomBasic, DoomDefendCenter, DoomTakeCover.

The reference's ``gym_doom`` levels need the ViZDoom engine (``envs/doom``, ids ``gym_doom/Doom*-v0``).  These
three are small on-device re-creations with the machinery of the synthetic Atari games (``envs/atari_games.py``):
integer dynamics, the counter-based RNG, a 210x160 RGB frame painted far to near from a fixed number of
rectangles, and the same logic in ``csrc/games.hip`` (game ids 5, 6, 7) with this torch code as the bit-exact
oracle (``tests/test_doom_games_hip.py``).

* ``DoomBasic``        NOOP, ATTACK, MOVE_RIGHT, MOVE_LEFT.  The player strafes along the near wall; one monster
                       stands at the far wall.  A hit pays ``KILL`` and ends the episode, every shot costs ``SHOT``.
* ``DoomDefendCenter`` NOOP, ATTACK, TURN_RIGHT, TURN_LEFT.  The player turns in the centre of a round arena;
                       five monsters walk inward and bite at distance 0.  26 rounds; a kill pays +1.
* ``DoomTakeCover``    NOOP, MOVE_RIGHT, MOVE_LEFT.  Shooters at the far wall throw fireballs aimed at the
                       player's position at launch; the living reward counts the tics survived.

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
    """Shared parts of the three scenarios: scenario constants, action lookup, backdrop and projection."""
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


DOOM_GAMES = {"DoomBasic": DoomBasicVec, "DoomDefendCenter": DoomDefendCenterVec, "DoomTakeCover": DoomTakeCoverVec}
GAMES.update(DOOM_GAMES)
