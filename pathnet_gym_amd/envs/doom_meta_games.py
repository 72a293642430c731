"""Synthetic meta-Doom: the nine synthetic Doom levels as one task (the reference's ``meta-Doom-v0``).

``DoomMetaVec`` (id ``DoomMeta``) composes the nine ``*Vec`` classes of ``envs/doom_games.py`` and
``envs/doom_world_games.py``.  Every env plays one level at a time; a finished episode is scored 0..1000, a level whose
last five scores sum to 3000 (an average of 600) unlocks the next one, and after every episode the env moves to the
unlocked level with the lowest score.  The goal is 9000 points.  This torch code is the bit-exact oracle of
``csrc/games.hip`` ``meta_step_kernel``, which steps a batch whose envs sit on different levels in one launch
(``tests/test_doom_meta_games.py``, ``tests/test_doom_meta_hip.py``).

The rule, in integers (``envs/doom/scoring.py:MetaDoomScorer`` is the reference's float rule; floats cannot be
bit-exact on a device).

Levels 0..8 are ``LEVEL_NAMES`` (the ``doom9`` preset's order); ``n_actions = 8``; an action ``a >= n_actions(level)``
or ``a < 0`` plays as 0.  ``level_table()`` holds per level ``(lo, target, n_actions, max_steps)`` with
``lo = floor(random mean return)`` and ``target = ceil(threshold)`` of ``envs/thresholds.json``; the episode cap of level
``l`` is ``min(max_steps[l], env.max_episode_steps)``.

Score of a finished episode with level return ``ret``: ``ret`` is clamped to +-10^6, then
``score = clamp(990 * (ret - lo) // (target - lo), 0, 1000)`` (``//`` floors), so the calibrated threshold scores 990,
the reference's pass mark.

Ledger per env: ``hist[9][5]`` (the last five scores of every level, newest first, 0 at the start), ``unlocked`` (9-bit
mask, bit 0 set at the start), ``level``, ``req`` (-1 or a level asked for through ``change_level``), ``total5`` (the
total in fifths of a point).  At an episode end, in this order:

1. shift the level's history and insert ``score``;
2. for ``i = 7 .. 0``: ``sum(hist[i]) >= 3000`` unlocks level ``i + 1``;
3. ``total5 = sum of all history sums``, plus 2250 if every level's sum is >= 4950;
4. the next level is ``req`` if ``req`` is unlocked (``req`` is then cleared), otherwise the unlocked level with the
   lowest history sum, ties to the lowest index (level 0 if the mask is empty);
5. that level's game is reset, with the RNG counter order of every other game (reset at the counter after the
   step's increment, then one more increment).  A level the env was not on starts from zeroed state words.

A step's ``reward`` is the level's own step reward and ``done`` its episode end.  (The reference's reward is the change
of the total; at the five-try scale that is worthless under ``reward_clip = 1`` and not integer-exact.)  The episode
return reported at ``done`` is the float32 ``float(total5) * 0.2f``, one fp32 multiply, so GA fitness and the
evaluator's ledger see the meta total.  ``reset_where`` restarts the level's game and leaves the ledger alone.

An env that sits on level ``l`` steps exactly as the single-level game ``l`` with the same seed, global env index and
counter: state, reward, done and scene.

Kernel state row (``HIP_FIELDS``): the level state in ``NSU`` words (the largest level row; a level uses its own row
without counter / steps / epret, the words past it are 0), then ``level, unlocked, req, total5, hist[45]``, then
``counter, steps, epret``.
"""
from __future__ import annotations

import json
import math
import os

import torch

from .atari_games import BG, GAMES, PixelGameVec
from .doom.constants import LEVEL_NAMES

NL, NH = 9, 5
PASS5, FULL5, BONUS5, RET_MAX = 3000, 4950, 2250, 10 ** 6
HIP_LEVEL_GAMES = (5, 10, 6, 8, 9, 12, 13, 7, 14)        # csrc/games.hip ids of levels 0..8
GOAL = 9000.0


def level_table():
    """[(lo, target, n_actions, max_steps)] of levels 0..8."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "thresholds.json")
    with open(path) as f:
        games = json.load(f)["games"]
    rows = []
    for name in LEVEL_NAMES:
        lo, target = math.floor(games[name]["random"]["mean_return"]), math.ceil(games[name]["threshold"])
        assert -RET_MAX < lo < target < RET_MAX, name
        rows.append((lo, target, GAMES[name].n_actions, GAMES[name].max_steps))
    return rows


LEVEL_TABLE = level_table()


def standard_score(ret, lo, target):
    """Score tensors (int64) of episode returns; ``lo`` / ``target`` ints or tensors."""
    ret = ret.clamp(-RET_MAX, RET_MAX)
    den = torch.as_tensor(target - lo, device=ret.device).clamp(min=1)
    return torch.div(990 * (ret - lo), den, rounding_mode="floor").clamp(0, 1000)


class DoomMetaVec(PixelGameVec):
    id = "DoomMeta"
    n_actions = 8
    max_steps = 10000
    reward_threshold = GOAL
    HIP_GAME = "DoomMeta"                  # entry points of its own (ops/envs.py meta_step), no id of GAME_IDS
    HIP_FIELDS = (("lstate", "vec"), ("level", "i"), ("unlocked", "i"), ("req", "i"), ("total5", "i"),
                  ("hist", "vec"))

    def init_state(self):
        N, dev = self.num_envs, self.device
        self.subs = [GAMES[name](N, device=dev, seed=0, frameskip=self.frameskip, gray=self.gray, backend="torch")
                     for name in LEVEL_NAMES]
        for sub in self.subs:
            sub.obs = sub.obs[:0]                                   # frames are kept by the meta env alone
        self._ns = [len(sub._hip_pack()[0]) - 3 for sub in self.subs]      # level state words per level
        self.NSU = max(self._ns) + 3
        cols = [sub.scene().colors for sub in self.subs]
        self._nr = [len(c) for c in cols]
        self.RU = max(self._nr)
        self._color_tab = torch.tensor([list(c) + [BG] * (self.RU - len(c)) for c in cols], dtype=torch.uint8,
                                       device=dev)                  # [9, RU, 3]
        self.table = torch.tensor(LEVEL_TABLE, dtype=torch.int64, device=dev)
        self.level = torch.zeros(N, dtype=torch.int64, device=dev)
        self.unlocked = torch.ones(N, dtype=torch.int64, device=dev)
        self.req = torch.full((N,), -1, dtype=torch.int64, device=dev)
        self.total5 = torch.zeros(N, dtype=torch.int64, device=dev)
        self.hist = torch.zeros(N, NL, NH, dtype=torch.int64, device=dev)
        self._lv = torch.arange(NL, device=dev)

    # -- plumbing shared by every sub-game --------------------------------------------------------------------
    def seed(self, seed: int):
        super().seed(seed)
        for sub in self.subs:
            sub.seed(seed)

    def set_id_base(self, base: int):
        super().set_id_base(base)
        for sub in self.subs:
            sub.set_id_base(base)

    def _on(self, l):
        return self.level == l

    def _skip(self, m) -> bool:
        """On the CPU a level nobody is on is skipped; on a device that would cost a host sync."""
        return self.device.type == "cpu" and not bool(m.any())

    @staticmethod
    def _keep(sub, m, saved):
        """Envs outside ``m`` get their saved state back."""
        for k, p in sub._persist.items():
            p.copy_(torch.where(m.view(-1, *([1] * (p.dim() - 1))), p, saved[k]))

    def _clock(self, sub):
        sub.counter.copy_(self.counter)
        sub.steps.copy_(self.steps)
        sub.epret.copy_(self.epret)

    # -- packed state -----------------------------------------------------------------------------------------
    @property
    def lstate(self):
        """int64 [N, NSU]: the level state words of the level each env is on."""
        out = torch.zeros(self.num_envs, self.NSU, dtype=torch.int64, device=self.device)
        for l, sub in enumerate(self.subs):
            on = self._on(l)
            if self._skip(on):
                continue
            w = sub._hip_pack()[:, :self._ns[l]].long()
            out[:, :self._ns[l]] = torch.where(on[:, None], w, out[:, :self._ns[l]])
        return out

    def unpack(self, rows: torch.Tensor):
        """Set the torch state (ledger, clock and the level each env is on) from packed rows [N, NS]."""
        v = rows.long().to(self.device)
        j = self.NSU
        self.level.copy_(v[:, j].clamp(0, NL - 1))
        self.unlocked.copy_(v[:, j + 1])
        self.req.copy_(v[:, j + 2])
        self.total5.copy_(v[:, j + 3])
        self.hist.copy_(v[:, j + 4:j + 4 + NL * NH].reshape(-1, NL, NH))
        self.counter.copy_(v[:, -3] & 0xFFFFFFFF)
        self.steps.copy_(v[:, -2])
        self.epret.copy_(v[:, -1])
        for l, sub in enumerate(self.subs):
            on = self._on(l)
            if self._skip(on):
                continue
            own = sub._hip_pack()
            own[:, :self._ns[l]] = torch.where(on[:, None], rows[:, :self._ns[l]].to(own), own[:, :self._ns[l]])
            sub._st32, sub._hip = own, True
            try:
                PixelGameVec.sync_from_device(sub)
            finally:
                sub._hip = False
                del sub._st32

    def load_packed(self, rows: torch.Tensor):
        """Adopt packed rows as the state, on the device too when the HIP game runs."""
        if self._hip:
            self._st32.copy_(rows.to(self._st32))
        self.unpack(rows)

    def sync_from_device(self):
        if self._hip:
            self.unpack(self._st32)

    # -- torch physics ----------------------------------------------------------------------------------------
    def reset_state(self, mask):
        for l, sub in enumerate(self.subs):
            m = mask & self._on(l)
            if self._skip(m):
                continue
            self._clock(sub)
            sub.reset_state(m)
            sub._commit()

    def _advance(self, actions):
        N = self.num_envs
        a = actions.long().to(self.device)
        reward = torch.zeros(N, dtype=torch.int64, device=self.device)
        done = torch.zeros(N, dtype=torch.bool, device=self.device)
        counter, steps, epret = self.counter.clone(), self.steps.clone(), self.epret.clone()
        for l, sub in enumerate(self.subs):
            on = self._on(l)
            if self._skip(on):
                continue
            saved = {k: p.clone() for k, p in sub._persist.items()}
            self._clock(sub)
            al = torch.where((a >= sub.num_actions) | (a < 0), torch.zeros_like(a), a)
            r = torch.zeros_like(reward)
            for _ in range(self.frameskip):
                r += sub.physics(al)
            sub.counter += 1
            sub.steps += 1
            sub.epret += r
            d = sub.game_over() | (sub.steps >= min(sub.max_steps, int(self.max_episode_steps)))
            sub._commit()
            reward = torch.where(on, r, reward)
            done = torch.where(on, d, done)
            counter = torch.where(on, sub.counter, counter)
            steps = torch.where(on, sub.steps, steps)
            epret = torch.where(on, sub.epret, epret)
            self._keep(sub, on, saved)
        old = self.level.clone()
        new, total5 = self._ledger(done, epret)
        ep_return = torch.where(done, total5.float() * torch.tensor(0.2, dtype=torch.float32, device=self.device),
                                torch.zeros(N, device=self.device))
        self.counter.copy_(counter)
        self.steps.copy_(torch.where(done, torch.zeros_like(steps), steps))
        self.epret.copy_(torch.where(done, torch.zeros_like(epret), epret))
        self.level.copy_(new)
        for l, sub in enumerate(self.subs):
            m = done & (new == l)
            if self._skip(m):
                continue
            fresh = m & (old != l)
            for name, _ in sub.HIP_FIELDS:
                t = getattr(sub, name)
                t.copy_(torch.where(fresh.view(-1, *([1] * (t.dim() - 1))), torch.zeros_like(t), t))
            sub.counter.copy_(counter)
            sub.reset_state(m)
            sub._commit()
        self.counter += done.long()
        return reward, done, ep_return

    def _ledger(self, done, ret):
        """Steps 1-4 of the rule for the envs in ``done``; returns (level after the step, total5)."""
        lv = self.level
        row = self.table[lv]
        score = standard_score(ret, row[:, 0], row[:, 1])
        sel = done[:, None] & (lv[:, None] == self._lv[None])                    # [N, 9]: the history that shifts
        shifted = torch.cat([score[:, None, None].expand(-1, NL, 1), self.hist[:, :, :NH - 1]], 2)
        hist = torch.where(sel[:, :, None], shifted, self.hist)
        sums = hist.sum(2)
        unlocked = self.unlocked | (((sums[:, :NL - 1] >= PASS5).long() << (self._lv[1:])[None]).sum(1))
        total5 = sums.sum(1) + BONUS5 * (sums >= FULL5).all(1).long()
        open_ = ((unlocked[:, None] >> self._lv[None]) & 1) != 0
        key = torch.where(open_, sums, torch.full_like(sums, 2 ** 31 - 1))
        nxt = key.argmin(1)                                                      # first of equal minima
        nxt = torch.where(open_.any(1), nxt, torch.zeros_like(nxt))
        reqc = self.req.clamp(0, NL - 1)
        asked = (self.req >= 0) & (self.req < NL) & (((unlocked >> reqc) & 1) != 0)
        nxt = torch.where(asked, reqc, nxt)
        self.hist.copy_(hist)
        self.unlocked.copy_(torch.where(done, unlocked, self.unlocked))
        self.total5.copy_(torch.where(done, total5, self.total5))
        self.req.copy_(torch.where(done & asked, torch.full_like(self.req, -1), self.req))
        return torch.where(done, nxt, lv), total5

    # -- scene and renderer -----------------------------------------------------------------------------------
    def scene_rects(self) -> torch.Tensor:
        """int64 [N, RU, 4]: every env's scene of its level, slots past the level's own hidden (zeros)."""
        out = torch.zeros(self.num_envs, self.RU, 4, dtype=torch.int64, device=self.device)
        for l, sub in enumerate(self.subs):
            on = self._on(l)
            if self._skip(on):
                continue
            g = sub.scene().geometry()
            out[:, :self._nr[l]] = torch.where(on[:, None, None], g, out[:, :self._nr[l]])
        return out

    def draw(self, img):
        """Paint the slot index of the topmost rectangle per pixel, then look the colours up per env: one pass over
        RU slots whatever the levels in the batch."""
        N = self.num_envs
        geo = self.scene_rects()
        col = torch.cat([self._color_tab[self.level], self.color(BG).expand(N, 1, 3)], 1)     # [N, RU + 1, 3]
        top = torch.full((N, self.rows.shape[1], self.cols.shape[2]), self.RU, dtype=torch.int64, device=self.device)
        for r in range(self.RU):
            y0, x0, h, w = (t[:, None, None] for t in geo[:, r].unbind(-1))
            top.masked_fill_(((self.rows >= y0) & (self.rows < y0 + h)) & ((self.cols >= x0) & (self.cols < x0 + w)), r)
        img.copy_(col.gather(1, top.view(N, -1, 1).expand(-1, -1, 3)).view(img.shape))

    # -- HIP --------------------------------------------------------------------------------------------------
    def _hip_setup(self):
        from ..ops import envs as henv
        from .pong import gray_weights
        ns, nr, nl = henv.meta_layout()
        self._st32 = self._hip_pack()
        if (self._st32.shape[1], self.RU, NL) != (ns, nr, nl):
            raise RuntimeError(f"DoomMeta: row of {self._st32.shape[1]} ints, {self.RU} rectangles, {NL} levels; "
                               f"the kernel expects {ns}, {nr}, {nl}")
        assert self.RU <= henv.RECT_MAX, self.RU
        for l, name in enumerate(LEVEL_NAMES):
            if henv.GAME_IDS[name] != HIP_LEVEL_GAMES[l] or henv.game_layout(name) != (self._ns[l] + 3, self._nr[l]):
                raise RuntimeError(f"DoomMeta: level {l} ({name}) does not match the kernel's game")
        wr, wg, wb = gray_weights(self.gray)
        lum = lambda c: (c[..., 0] * wr + c[..., 1] * wg + c[..., 2] * wb + 8192) >> 14   # noqa: E731  cv2 luma
        self._gray_tab = lum(self._color_tab.long()).to(torch.uint8).contiguous()          # [9, RU]
        self._bg_gray = int((BG[0] * wr + BG[1] * wg + BG[2] * wb + 8192) >> 14)
        self._level_tab = self.table.to(torch.int32).contiguous()
        N = self.num_envs
        self._rects = torch.zeros(N, nr, 4, dtype=torch.int16, device=self.device)
        self._lv8 = torch.zeros(N, dtype=torch.uint8, device=self.device)
        self._tab32 = self.tables.to(torch.int32).contiguous()
        self._rw = torch.zeros(N, dtype=torch.float32, device=self.device)
        self._dn = torch.zeros(N, dtype=torch.uint8, device=self.device)
        self._ep = torch.zeros(N, dtype=torch.float32, device=self.device)
        self._hip = True

    def _hip_run(self, actions, mask, reward, done, epret):
        from ..ops import envs as henv
        henv.meta_step(self._st32, self._level_tab, actions, mask, self.seed_int, self.frameskip,
                       int(self.max_episode_steps), reward, done, epret, self._rects, self._lv8, id_base=self.id_base)

    def _hip_push(self, obs_in, obs_out, reset_u8):
        from ..ops import envs as henv
        henv.rects16_stack_push_lv(self._rects, self._gray_tab, self._lv8, self._bg_gray, obs_in, obs_out, reset_u8,
                                   self._tab32)

    def _hip_ring_push(self, frames, slot, fc_in, fc_out, reset_u8):
        from ..ops import envs as henv
        henv.rects16_ring_push_lv(self._rects, self._gray_tab, self._lv8, self._bg_gray, frames, slot, fc_in, fc_out,
                                  reset_u8, self._tab32)

    # -- host interface, as the reference's ``info`` ------------------------------------------------------------
    def meta_info(self):
        """``level`` [N], ``scores`` [N, 9] (history sum / 5), ``locked_levels`` [N, 9] bool, ``total_reward`` [N]."""
        self.sync_from_device()
        return {"level": self.level.clone(),
                "scores": self.hist.sum(2).float() / 5,
                "locked_levels": ((self.unlocked[:, None] >> self._lv[None]) & 1) == 0,
                "total_reward": self.total5.float() * torch.tensor(0.2, dtype=torch.float32, device=self.device)}

    def change_level(self, levels, mask=None):
        """Ask for ``levels`` (an int or [N]) at the next episode end of the envs in ``mask`` (default all).  The
        request is honoured once the level is unlocked and cleared when it is used."""
        lv = torch.as_tensor(levels, device=self.device).long().expand(self.num_envs)
        if bool(((lv < 0) | (lv >= NL)).any()):
            raise ValueError(f"change_level: levels outside [0, {NL})")
        m = torch.ones(self.num_envs, dtype=torch.bool, device=self.device) if mask is None else \
            torch.as_tensor(mask, device=self.device).bool()
        if self._hip:                                               # the kernel's word is the authority
            self.req.copy_(self._st32[:, self.NSU + 2])
        self.req.copy_(torch.where(m, lv, self.req))
        if self._hip:
            self._st32[:, self.NSU + 2] = self.req.to(torch.int32)

