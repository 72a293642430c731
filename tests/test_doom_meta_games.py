"""Synthetic meta-Doom (envs/doom_meta_games.py): the integer curriculum rule against an independent implementation
and against the reference's float rule (envs/doom/scoring.py), the levels inside the meta env against the single-level
games, the score / action / return conventions, the host interface and the registration.

``seed_ledgers`` / ``mixed_env`` / ``play_mixed`` build the mixed-level run that tests/test_doom_meta_hip.py replays
on the device; ``test_mixed_run_reaches_every_branch`` checks here, on the oracle, that the run is worth replaying."""
import numpy as np
import pytest
import torch

from pathnet_gym_amd.envs import registry
from pathnet_gym_amd.envs.doom.constants import LEVEL_NAMES
from pathnet_gym_amd.envs.doom.scoring import MetaDoomScorer
from pathnet_gym_amd.envs.doom_meta_games import (BONUS5, HIP_LEVEL_GAMES, LEVEL_TABLE, NH, NL, DoomMetaVec,
                                                  standard_score)

N_MIX, T_MIX, ID_BASE, SEED, ACTION_SEED, CAP = 36, 72, 7, 11, 5, 12
ENV_SHORT, ENV_FULL, ENV_FULL_DROP = 0, 27, 35        # one score short of an unlock; every level at 5000 (two of them)


# ------------------------------------------------------------------------------------------- an independent ledger
def fdiv(a, b):
    q = abs(a) // abs(b)
    if (a < 0) != (b < 0):
        q = -q - (1 if abs(a) % abs(b) else 0)
    return q


def ref_score(ret, lo, target):
    ret = max(-10 ** 6, min(10 ** 6, ret))
    return max(0, min(1000, fdiv(990 * (ret - lo), target - lo)))


class RefLedger:
    """The rule of the issue, written for one env with Python ints and lists."""

    def __init__(self, table):
        self.table = table
        self.hist = [[0] * 5 for _ in range(9)]
        self.unlocked = [True] + [False] * 8
        self.level, self.req, self.total5 = 0, -1, 0

    def end(self, ret):
        lo, target = self.table[self.level][:2]
        self.hist[self.level] = [ref_score(ret, lo, target)] + self.hist[self.level][:4]
        for i in range(7, -1, -1):
            if sum(self.hist[i]) >= 3000:
                self.unlocked[i + 1] = True
        self.total5 = sum(sum(h) for h in self.hist)
        if all(sum(h) >= 4950 for h in self.hist):
            self.total5 += 2250
        if self.req >= 0 and self.unlocked[self.req]:
            self.level, self.req = self.req, -1
        else:
            best = None
            for i in range(9):
                if self.unlocked[i] and (best is None or sum(self.hist[i]) < sum(self.hist[best])):
                    best = i
            self.level = 0 if best is None else best
        return self.level


def _mask_of(flags):
    return sum(1 << i for i, f in enumerate(flags) if f)


def _end(env, done, ret):
    """What ``_advance`` does with the ledger at the episode ends in ``done``."""
    new, total5 = env._ledger(done, ret)
    env.level.copy_(new)
    return total5


def test_ledger_matches_an_independent_integer_implementation():
    N = 20
    env = DoomMetaVec(N, seed=1)
    refs = [RefLedger(LEVEL_TABLE) for _ in range(N)]
    g = torch.Generator().manual_seed(3)
    ends = 0
    while ends < 2000:
        done = torch.rand(N, generator=g) < 0.7
        # returns from below lo to well beyond the target of the level each env is on (most pass), some far outside
        row = env.table[env.level]
        span = row[:, 1] - row[:, 0]
        ret = row[:, 0] + ((torch.rand(N, generator=g) * 1.6 - 0.1) * span.float()).long()
        wild = torch.rand(N, generator=g) < 0.05
        ret = torch.where(wild, torch.randint(-10 ** 7, 10 ** 7, (N,), generator=g), ret)
        asks = torch.rand(N, generator=g) < 0.15
        want = torch.randint(0, NL, (N,), generator=g)
        env.change_level(want, asks)
        for e in range(N):
            if asks[e]:
                refs[e].req = int(want[e])
        _end(env, done, ret)
        for e in range(N):
            if done[e]:
                refs[e].end(int(ret[e]))
                ends += 1
            r = refs[e]
            assert env.hist[e].tolist() == r.hist, (ends, e)
            assert int(env.unlocked[e]) == _mask_of(r.unlocked), (ends, e)
            assert (int(env.level[e]), int(env.req[e]), int(env.total5[e])) == (r.level, r.req, r.total5), (ends, e)
    assert max(_mask_of(r.unlocked) for r in refs) == 511       # the sequences did unlock every level somewhere
    assert any(r.total5 > 0 for r in refs)


def test_ledger_matches_the_reference_float_scorer_on_multiples_of_five():
    """``MetaDoomScorer`` with five tries averaged over five and a pass mark of 600: with scores that are multiples
    of 5 every average is an exact integer, so the float rule and the integer rule must agree exactly."""
    N = 10
    env = DoomMetaVec(N, seed=1)
    env.table[:, 0], env.table[:, 1] = 0, 990                  # score == clamp(ret, 0, 1000): feed scores directly
    scorers = [MetaDoomScorer(average_over=5, min_tries_for_avg=5, passing_grade=600) for _ in range(N)]
    g = torch.Generator().manual_seed(4)
    ends = 0
    while ends < 2800:
        done = torch.rand(N, generator=g) < 0.8
        score = torch.randint(0, 201, (N,), generator=g) * 5
        good = torch.rand(N, generator=g) < 0.5                # half of the episodes pass: levels do unlock
        score = torch.where(good, score.clamp(min=700), score)
        if ends >= 2000:                                       # then 990 and better only, up to the bonus
            score = torch.randint(198, 201, (N,), generator=g) * 5
        total5 = _end(env, done, score)
        for e in range(N):
            if not done[e]:
                continue
            ends += 1
            sc = scorers[e]
            sc.start_episode()
            sc.scores[sc.level][0] = float(score[e])
            total = sc.get_total_reward()
            sc.unlock_levels()
            nxt = sc.change_level()
            assert int(env.unlocked[e]) == _mask_of(not k for k in sc.locked_levels), (ends, e)
            assert int(env.level[e]) == nxt, (ends, e)
            assert int(total5[e]) == total * 5 and int(env.total5[e]) == total * 5, (ends, e, total)
    assert int(env.unlocked.max()) == 511
    assert int(env.total5.max()) >= 9 * 4950 + BONUS5          # the 50-points-per-level bonus was reached


# ------------------------------------------------------------------------------------------- levels inside the meta env
def _pair(level, n=5, seed=3):
    m = registry.make("DoomMeta", num_envs=n, seed=seed)
    s = registry.make(LEVEL_NAMES[level], num_envs=n, seed=seed)
    for e in (m, s):
        e.set_id_base(ID_BASE)
        e.max_episode_steps = CAP
    m.level[:] = level
    m.unlocked[:] = 1 << level
    return m, s


@pytest.mark.parametrize("level", range(NL))
def test_pinned_level_is_the_single_level_game(level):
    """Only ``level`` unlocked through the state, and asked for again before every step (Basic's short episodes
    score 1000, so the ledger alone would unlock the next level and move on)."""
    m, s = _pair(level)
    assert torch.equal(m.reset(), s.reset())
    g = torch.Generator().manual_seed(1)
    ndone = 0
    for t in range(40):
        a = torch.randint(0, 8, (5,), generator=g)
        m.change_level(level)
        om, rm, dm, _ = m.step(a)
        os_, rs, ds, _ = s.step(a)
        assert torch.equal(om, os_) and torch.equal(rm, rs) and torch.equal(dm, ds), t
        pm, ps = m._hip_pack(), s._hip_pack()
        k = ps.shape[1] - 3
        assert torch.equal(pm[:, :k], ps[:, :k]) and torch.equal(pm[:, -3:], ps[:, -3:]), t
        assert not pm[:, k:m.NSU].any()
        assert (m.level == level).all()
        ndone += int(dm.sum())
    assert ndone >= 3 * 5


def test_mixed_batch_env_by_env_against_the_single_level_games():
    """One env per level, held on its level: env e equals env e of the single-level game of its level (same seed
    and global index), so what the other levels do in the same batch leaks nowhere."""
    N = 9
    lv = torch.arange(N) % NL
    m = registry.make("DoomMeta", num_envs=N, seed=9)
    singles = [registry.make(n, num_envs=N, seed=9) for n in LEVEL_NAMES]
    for e in [m] + singles:
        e.set_id_base(ID_BASE)
        e.max_episode_steps = CAP
    m.level.copy_(lv)
    m.unlocked[:] = 511
    om = m.reset()
    for l, s in enumerate(singles):
        assert torch.equal(om[lv == l], s.reset()[lv == l])
    g = torch.Generator().manual_seed(2)
    for t in range(15):                                        # across the episode cap
        a = torch.randint(0, 8, (N,), generator=g)
        m.change_level(lv)
        om, rm, dm, _ = m.step(a)
        rows = m._hip_pack()
        for l, s in enumerate(singles):
            on = lv == l
            os_, rs, ds, _ = s.step(a)
            assert torch.equal(om[on], os_[on]) and torch.equal(rm[on], rs[on]) and torch.equal(dm[on], ds[on]), (t, l)
            ps = s._hip_pack()
            assert torch.equal(rows[on][:, :ps.shape[1] - 3], ps[on][:, :-3]), (t, l)
            assert torch.equal(rows[on][:, -3:], ps[on][:, -3:]), (t, l)


# ------------------------------------------------------------------------------------------- score, actions, epret
def test_standard_score_points():
    for lo, target, _, _ in LEVEL_TABLE:
        t = lambda v: torch.tensor(v)                                              # noqa: E731
        assert int(standard_score(t(lo), lo, target)) == 0
        assert int(standard_score(t(target), lo, target)) == 990                  # the reference's pass mark
        assert int(standard_score(t(lo - 1000), lo, target)) == 0
        assert int(standard_score(t(target + 10 * (target - lo)), lo, target)) == 1000
        assert int(standard_score(t(10 ** 7), lo, target)) == 1000
        assert int(standard_score(t(-10 ** 7), lo, target)) == 0
        for ret in (lo + 1, (lo + target) // 2, target - 1, target + 1):
            assert int(standard_score(t(ret), lo, target)) == ref_score(ret, lo, target)
    # the clamp of the return to +-10^6 comes before the division: on a row this wide it decides the score
    lo, target = -999_999, 999_999
    assert int(standard_score(torch.tensor(10 ** 7), lo, target)) == ref_score(10 ** 6, lo, target) == 990
    assert int(standard_score(torch.tensor(-10 ** 7), lo, target)) == 0
    assert 990 * (10 ** 6 - lo) < 2 ** 31                     # and keeps the kernel's product far inside its type


@pytest.mark.parametrize("level", range(NL))
def test_actions_beyond_the_levels_own_play_as_noop(level):
    n_act = LEVEL_TABLE[level][2]
    envs = []
    for bad in (None, n_act, 7 if n_act < 8 else 8, -1):
        m, _ = _pair(level, n=4, seed=5)
        m.reset()
        g = torch.Generator().manual_seed(6)
        for t in range(10):
            a = torch.randint(0, n_act, (4,), generator=g)
            if bad is not None:
                a = torch.where(a == 0, torch.full_like(a, bad), a)
            m.change_level(level)
            m.step(a)
        envs.append(m._hip_pack())
    for rows in envs[1:]:
        assert torch.equal(rows, envs[0])
    assert DoomMetaVec.n_actions == 8 == max(r[2] for r in LEVEL_TABLE)


def test_episode_return_is_the_total_as_one_float32_multiply():
    m = mixed_env()
    g = torch.Generator().manual_seed(ACTION_SEED)
    seen = 0
    for t in range(CAP + 1):
        _, r, d, info = m.step(torch.randint(0, 8, (N_MIX,), generator=g))
        want = np.float32(m.total5.numpy().astype(np.float32)) * np.float32(0.2)
        ep = info["episode_return"]
        assert ep.dtype == torch.float32
        assert np.array_equal(ep.numpy()[d.numpy()], want[d.numpy()]) and not ep[~d].any()
        seen += int(d.sum())
    assert seen >= N_MIX                                       # the cap ends every env's episode once
    assert float(info["episode_return"].max()) <= 9450.0


# ------------------------------------------------------------------------------------------- bonus, requests, info
def test_bonus_of_fifty_points_per_level_when_every_level_passes():
    env = DoomMetaVec(2, seed=1)
    env.hist[:] = 1000
    env.unlocked[:] = 511
    done = torch.ones(2, dtype=torch.bool)
    ret = torch.tensor([LEVEL_TABLE[0][1], LEVEL_TABLE[0][0]])               # at the target: 990; at lo: 0
    _end(env, done, ret)
    assert env.hist[:, 0].tolist() == [[990, 1000, 1000, 1000, 1000], [0, 1000, 1000, 1000, 1000]]
    assert env.total5.tolist() == [8 * 5000 + 4990 + 2250, 8 * 5000 + 4000]
    assert env.meta_info()["total_reward"].tolist() == [np.float32(47240) * np.float32(0.2), 8800.0]
    # 4950 is the edge: one level at 4945 loses the bonus
    env.hist[0, 3] = torch.tensor([1000, 1000, 1000, 1000, 945])
    _end(env, torch.tensor([True, False]), torch.tensor([LEVEL_TABLE[int(env.level[0])][1]] * 2))
    assert int(env.total5[0]) == int(env.hist[0].sum())


def test_change_level_needs_an_unlocked_level_and_is_used_once():
    m = registry.make("DoomMeta", num_envs=3, seed=2)
    m.max_episode_steps = 3
    m.unlocked[:] = 0b101
    m.reset()
    m.change_level(torch.tensor([1, 2, 2]), torch.tensor([True, True, False]))
    assert m.req.tolist() == [1, 2, -1]
    for t in range(3):
        _, _, d, _ = m.step(torch.zeros(3, dtype=torch.long))
    assert d.all()
    # env 0 asked for a locked level: not honoured, still pending; env 1 got level 2; env 2 follows the scores
    assert m.req.tolist() == [1, -1, -1]
    assert m.level[1] == 2 and m.level[0] != 1
    for t in range(3):
        m.step(torch.zeros(3, dtype=torch.long))
    assert m.req.tolist() == [1, -1, -1]
    with pytest.raises(ValueError):
        m.change_level(9)


def test_meta_info_is_the_references_info():
    m = mixed_env()
    info = m.meta_info()
    assert set(info) == {"level", "scores", "locked_levels", "total_reward"}
    assert info["level"].shape == (N_MIX,) and info["scores"].shape == (N_MIX, NL)
    assert info["locked_levels"].shape == (N_MIX, NL) and info["locked_levels"].dtype == torch.bool
    assert info["total_reward"].shape == (N_MIX,) and info["total_reward"].dtype == torch.float32
    assert torch.equal(info["scores"], m.hist.sum(2).float() / 5)
    assert info["locked_levels"][ENV_SHORT].tolist() == [False] + [True] * 8
    assert not info["locked_levels"][ENV_FULL].any() and info["scores"][ENV_FULL].tolist() == [1000.0] * NL


# ------------------------------------------------------------------------------------------- registration
def test_registration_and_preset():
    from pathnet_gym_amd.config import preset
    from pathnet_gym_amd.ops import envs as henv
    for env_id in ("SynthDoomMeta-v0", "DoomMeta"):
        assert registry.is_synthetic(env_id) and registry.reward_threshold(env_id) == 9000.0
        env = registry.make(env_id, num_envs=2, seed=1)
        assert isinstance(env, DoomMetaVec) and env.id == env_id and env.reward_threshold == 9000.0
        assert env.num_actions == 8 and env.obs_shape == (160, 120, 4)
    assert "DoomMeta" not in registry.synthetic_thresholds()           # fixed by rule, not calibrated
    cfg = preset("doom-meta")
    assert cfg.tasks == ["DoomMeta"] and cfg.env == "DoomMeta"
    assert cfg.net.num_actions == 8 and cfg.net.num_tasks == 1
    assert cfg.net.layers == preset("doom9").net.layers
    assert henv.GAME_IDS == {"Breakout": 0, "SpaceInvaders": 1, "Alien": 2, "MsPacman": 3, "Centipede": 4,
                             "DoomBasic": 5, "DoomDefendCenter": 6, "DoomTakeCover": 7, "DoomDefendLine": 8,
                             "DoomHealthGathering": 9, "DoomCorridor": 10, "DoomMyWayHome": 12,
                             "DoomPredictPosition": 13, "DoomDeathmatch": 14}
    assert [henv.GAME_IDS[n] for n in LEVEL_NAMES] == list(HIP_LEVEL_GAMES) == [5, 10, 6, 8, 9, 12, 13, 7, 14]
    assert preset("doom9").tasks == LEVEL_NAMES
    # the level table: lo below target, read from the calibration file
    import json
    import math
    import os
    with open(os.path.join(os.path.dirname(registry.__file__), "thresholds.json")) as f:
        games = json.load(f)["games"]
    for name, (lo, target, n_act, steps) in zip(LEVEL_NAMES, LEVEL_TABLE):
        assert lo == math.floor(games[name]["random"]["mean_return"]) and target == math.ceil(games[name]["threshold"])
        assert lo < target and (n_act, steps) == (registry.make(name).num_actions, registry.make(name).max_steps)


def test_hip_fields_mirror_the_row():
    m = DoomMetaVec(3, seed=1)
    rows = m._hip_pack()
    assert rows.shape == (3, m.NSU + 4 + NL * NH + 3) and rows.dtype == torch.int32
    assert m.NSU == max(registry.make(n)._hip_pack().shape[1] for n in LEVEL_NAMES)
    j = m.NSU
    assert rows[:, j:j + 4].tolist() == [[0, 1, -1, 0]] * 3
    m.reset()
    g = torch.Generator().manual_seed(1)
    for t in range(5):
        m.step(torch.randint(0, 8, (3,), generator=g))
    rows = m._hip_pack()
    other = DoomMetaVec(3, seed=1)
    other.load_packed(rows)                                    # unpack is the inverse of pack
    assert torch.equal(other._hip_pack(), rows)
    a = torch.randint(0, 8, (3,), generator=g)
    other.obs = m.obs.clone()
    o1, r1, d1, _ = m.step(a)
    o2, r2, d2, _ = other.step(a)
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    assert torch.equal(other._hip_pack(), m._hip_pack())


# ------------------------------------------------------------------------------------------- the mixed-level run
def seed_ledgers(env):
    """Ledgers for N_MIX envs, written into the torch state before the first reset: four envs on each level.

    Group 0 (envs 0-8): the levels up to the env's own are unlocked.  Group 1 (9-17): everything unlocked and the
    NEXT level's history empty, so the first episode end moves the env there: every level is entered.  Group 2
    (18-26): everything unlocked, a request for level + 3 pending.  Group 3 (27-35): level 0 and the env's own.
    Histories are 0..495, no sum reaches 3000, except: ENV_SHORT sits on Basic with [1000, 1000, 0, 0, 0], one
    score of 1000 short of unlocking level 1 (a 12-step Basic episode scores 1000); ENV_FULL (on Basic) and
    ENV_FULL_DROP (on Deathmatch, where random play scores 0) have every level at 5000."""
    N = env.num_envs
    g = torch.Generator().manual_seed(23)
    e = torch.arange(N)
    level, grp = e % NL, e // NL
    hist = torch.randint(0, 100, (N, NL, NH), generator=g) * 5
    nxt = (level + 1) % NL
    hist[e[grp == 1], nxt[grp == 1]] = 0
    unlocked = torch.full((N,), 511)
    unlocked = torch.where(grp == 0, (2 << level) - 1, unlocked)
    unlocked = torch.where(grp == 3, (1 << level) | 1, unlocked)
    req = torch.where(grp == 2, (level + 3) % NL, torch.full((N,), -1))
    hist[ENV_SHORT, 0] = torch.tensor([1000, 1000, 0, 0, 0])
    for k in (ENV_FULL, ENV_FULL_DROP):
        hist[k] = 1000
        unlocked[k] = 511
    env.level.copy_(level)
    env.unlocked.copy_(unlocked)
    env.req.copy_(req)
    env.hist.copy_(hist)
    env.total5.copy_(hist.sum((1, 2)))


def mixed_env(n=N_MIX, id_base=ID_BASE, device="cpu", backend="torch", reset=True):
    env = registry.make("DoomMeta", num_envs=n, device=device, seed=SEED, backend=backend)
    env.set_id_base(id_base)
    env.max_episode_steps = CAP
    if device == "cpu":
        seed_ledgers(env)
        if reset:
            env.reset()
    return env


def mixed_actions():
    g = torch.Generator().manual_seed(ACTION_SEED)
    acts = torch.randint(-1, 10, (T_MIX, N_MIX), generator=g)       # -1, 8 and 9 are outside every level's set
    return acts


def play_mixed(env, on_step=None):
    """Play the mixed run on the oracle; returns (entries into each level by a level change, unlock events)."""
    into, unlocks = [0] * NL, 0
    for t, a in enumerate(mixed_actions()):
        lv0, un0 = env.level.clone(), env.unlocked.clone()
        out = env.step(a)
        moved = env.level != lv0
        for l in env.level[moved].tolist():
            into[l] += 1
        unlocks += int((env.unlocked != un0).sum())
        if on_step is not None:
            on_step(t, a, out)
    return into, unlocks


def test_mixed_run_reaches_every_branch():
    env = mixed_env()
    assert sorted(env.level.tolist()) == sorted(list(range(NL)) * 4)
    seen = {"req": 0}
    env._push = lambda obs_in, reset, obs_out=None: obs_in     # the ledger and the games only: no frames needed here

    def on_step(t, a, out):
        if t == CAP - 1:
            # the first episode ends: ENV_SHORT's 1000 made Basic's sum exactly 3000 and it moved on to level 1
            assert env.hist[ENV_SHORT, 0].tolist() == [1000, 1000, 1000, 0, 0]
            assert int(env.unlocked[ENV_SHORT]) == 0b11 and int(env.level[ENV_SHORT]) == 1
            assert int(env.total5[ENV_FULL]) == 45000 + BONUS5 and int(env.level[ENV_FULL]) == 0
            assert int(env.total5[ENV_FULL_DROP]) == 44000 and int(env.level[ENV_FULL_DROP]) == 8
            seen["req"] = int((env.req[18:27] == -1).sum())

    into, unlocks = play_mixed(env, on_step)
    assert min(into) >= 1, into                                # a level change into each of the nine levels
    assert unlocks >= 1
    assert seen["req"] == 9                                    # the nine pending requests were used
