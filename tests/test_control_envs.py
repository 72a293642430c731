"""Acrobot-v1 and MountainCar-v0 (envs/control.py, torch backend) and the vector suite's plumbing, on the CPU.

One step against a float64 numpy implementation of the equations (carried here, independent of the env's code),
scripted policies with the returns these tasks are known to give, the env rules (resets, id_base, step limit,
auto-reset, actions >= 3, padding) and the registry / presets / trainer / checkpoint / evaluator plumbing.

Deviations are fractions of each component's range (Acrobot: pi, pi, 4 pi, 9 pi; MountainCar: 1.2, 0.07); angles
are compared modulo 2 pi.  Bounds: Acrobot 99.9th percentile <= 2e-5 (measured with this env: angles 1.6e-6,
velocities 6.1e-6), maximum <= 1e-3 (measured 2.9e-4; ill-conditioned high-speed states dominate the tail);
MountainCar maximum <= 4 ulp of the range (measured 0.53 and 0.54 ulp).  Discrete outcomes are compared outside
near-ties (measured: 0.006 % of the Acrobot states within 1e-4 of the height threshold, 0.006 % within 1e-4 of a
wrap edge, 0.0005 % of the MountainCar states within 4 ulp of a threshold; at most 0.1 % may be left out).
"""
import math

import numpy as np
import pytest
import torch

from pathnet_gym_amd.config import preset
from pathnet_gym_amd.envs.base import env_rand_u32
from pathnet_gym_amd.envs.cartpole import CartPoleVec
from pathnet_gym_amd.envs.control import AcrobotVec, MountainCarVec
from pathnet_gym_amd.envs.registry import make, reward_threshold

PI = math.pi
ACRO_RANGE = np.array([PI, PI, 4 * PI, 9 * PI])
MC_RANGE = np.array([1.2, 0.07])
P999_BOUND = 2e-5
MAX_BOUND = 1e-3
TIE = 1e-4                      # near-tie: the float64 value lies within this of a threshold
MC_ULPS = 4.0
N_STATES = 200_000


# ---------------------------------------------------------------------------------------------------------------
# float64 references (the issue's equations; g and dt are arguments for the negative controls)
# ---------------------------------------------------------------------------------------------------------------
def acrobot_dsdt64(s, tau, g):
    m1 = m2 = 1.0
    l1 = 1.0
    lc1 = lc2 = 0.5
    I1 = I2 = 1.0
    th1, th2, w1, w2 = s.T
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * np.cos(th2)) + I1 + I2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * np.cos(th2)) + I2
    phi2 = m2 * lc2 * g * np.cos(th1 + th2 - PI / 2)
    phi1 = (-m2 * l1 * lc2 * w2 ** 2 * np.sin(th2) - 2 * m2 * l1 * lc2 * w2 * w1 * np.sin(th2)
            + (m1 * lc1 + m2 * l1) * g * np.cos(th1 - PI / 2) + phi2)
    a2 = (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 ** 2 * np.sin(th2) - phi2) / (m2 * lc2 ** 2 + I2 - d2 ** 2 / d1)
    a1 = -(d2 * a2 + phi1) / d1
    return np.stack([w1, w2, a1, a2], 1)


def acrobot_step64(s, a, g=9.8, dt=0.2):
    """-> dict(pre = state after RK4 before wrap / clamp, new = the new state, height, term, reward)."""
    s = np.asarray(s, np.float64)
    a = np.where(np.asarray(a) >= 3, 0, np.asarray(a))
    tau = (a - 1).astype(np.float64)
    k1 = acrobot_dsdt64(s, tau, g)
    k2 = acrobot_dsdt64(s + dt / 2 * k1, tau, g)
    k3 = acrobot_dsdt64(s + dt / 2 * k2, tau, g)
    k4 = acrobot_dsdt64(s + dt * k3, tau, g)
    pre = s + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    new = pre.copy()
    for c in (0, 1):
        x = new[:, c]
        for _ in range(3):
            x = np.where(x > PI, x - 2 * PI, x)
        for _ in range(3):
            x = np.where(x < -PI, x + 2 * PI, x)
        new[:, c] = x
    new[:, 2] = np.clip(new[:, 2], -4 * PI, 4 * PI)
    new[:, 3] = np.clip(new[:, 3], -9 * PI, 9 * PI)
    height = -np.cos(new[:, 0]) - np.cos(new[:, 0] + new[:, 1])
    term = height > 1.0
    return dict(pre=pre, new=new, height=height, term=term, reward=np.where(term, 0.0, -1.0))


def mountaincar_step64(s, a):
    s = np.asarray(s, np.float64)
    a = np.where(np.asarray(a) >= 3, 0, np.asarray(a))
    p, v = s.T
    v = v + (a - 1) * 0.001 + np.cos(3 * p) * (-0.0025)
    v = np.clip(v, -0.07, 0.07)
    pre_p, pre_v = p + v, v
    p = np.clip(pre_p, -1.2, 0.6)
    v = np.where((p == -1.2) & (v < 0), 0.0, v)
    return dict(pre_p=pre_p, pre_v=pre_v, new=np.stack([p, v], 1), term=(p >= 0.5) & (v >= 0))


def acrobot_dev(new32, ref64):
    """[N, 4] deviations in fractions of the range, angles modulo 2 pi."""
    d = np.asarray(new32, np.float64) - ref64
    d[:, :2] = (d[:, :2] + PI) % (2 * PI) - PI
    return np.abs(d) / ACRO_RANGE


def acrobot_states(n, seed):
    rng = np.random.default_rng(seed)
    s = (rng.uniform(-1, 1, (n, 4)) * ACRO_RANGE).astype(np.float32)
    return s, rng.integers(0, 3, n)


def mountaincar_states(n, seed):
    rng = np.random.default_rng(seed)
    s = np.stack([rng.uniform(-1.2, 0.6, n), rng.uniform(-0.07, 0.07, n)], 1).astype(np.float32)
    return s, rng.integers(0, 3, n)


def acrobot_near_tie(ref):
    """States whose float64 outcome lies within TIE of a discrete threshold: the height test, or a wrap edge."""
    tie_h = np.abs(ref["height"] - 1.0) < TIE
    ang = ref["pre"][:, :2]
    edge = np.abs((ang - PI) % (2 * PI))          # distance above an odd multiple of pi ...
    edge = np.minimum(edge, 2 * PI - edge)        # ... or below it
    return tie_h, (edge < TIE).any(1)


def one_step(env, states, actions):
    """Load ``states`` into a torch env, play ``actions``, return (state before any reset, terminal, reward)."""
    st = torch.from_numpy(np.ascontiguousarray(states))
    a = torch.from_numpy(np.asarray(actions)).long()
    new, term, reward = env._dynamics(st, a)
    return new.numpy(), term.numpy(), reward.numpy()


@pytest.fixture(scope="module")
def acrobot_case():
    s, a = acrobot_states(N_STATES, 11)
    env = AcrobotVec(N_STATES)
    new, term, reward = one_step(env, s, a)
    return dict(s=s, a=a, new=new, term=term, reward=reward, ref=acrobot_step64(s, a))


def test_acrobot_step_matches_float64(acrobot_case):
    c = acrobot_case
    dev = acrobot_dev(c["new"], c["ref"]["new"])
    p_ang = np.percentile(dev[:, :2], 99.9)
    p_vel = np.percentile(dev[:, 2:], 99.9)
    print(f"acrobot p99.9 angles {p_ang:.3e} velocities {p_vel:.3e} max {dev.max():.3e}")
    assert p_ang <= P999_BOUND and p_vel <= P999_BOUND
    assert dev.max() <= MAX_BOUND


@pytest.mark.parametrize("kw", [dict(g=9.81), dict(dt=0.21)])
def test_acrobot_negative_controls_fail_the_percentile_bound(acrobot_case, kw):
    c = acrobot_case
    dev = acrobot_dev(c["new"], acrobot_step64(c["s"], c["a"], **kw)["new"])
    assert max(np.percentile(dev[:, :2], 99.9), np.percentile(dev[:, 2:], 99.9)) > P999_BOUND


def test_acrobot_discrete_outcomes(acrobot_case):
    c = acrobot_case
    ref = c["ref"]
    tie_h, tie_w = acrobot_near_tie(ref)
    print(f"acrobot near-ties: height {tie_h.mean():.5%} wrap {tie_w.mean():.5%}")
    assert tie_h.mean() <= 1e-3 and tie_w.mean() <= 1e-3
    ok = ~tie_h
    assert np.array_equal(c["term"][ok], ref["term"][ok])
    assert np.array_equal(c["reward"][ok], ref["reward"][ok].astype(np.float32))
    # wrap: away from an edge the env took the same number of turns off (no 2 pi between the two)
    w = ~tie_w
    assert np.abs(c["new"][w, :2] - ref["new"][w, :2]).max() < 1.0
    # three passes bring anything within 7 pi home (a state at top speed can leave further than that in one step:
    # the rule is three passes, and env and reference then agree on where it is left)
    home = (np.abs(ref["pre"][:, :2]) < 7 * PI - TIE) & w[:, None]
    assert np.abs(c["new"][:, :2][home]).max() <= np.float32(PI) + 1e-6 and not home.all()
    # clamp: never outside the box, and at the bound wherever the reference is
    assert np.abs(c["new"][:, 2]).max() <= np.float32(4 * PI) and np.abs(c["new"][:, 3]).max() <= np.float32(9 * PI)
    for col, lim in ((2, 4 * PI), (3, 9 * PI)):
        hit = np.abs(ref["pre"][:, col]) > lim + TIE
        assert hit.any()
        assert np.array_equal(np.abs(c["new"][hit, col]), np.full(hit.sum(), np.float32(lim)))


def test_mountaincar_step_matches_float64():
    s, a = mountaincar_states(N_STATES, 12)
    new, term, _ = one_step(MountainCarVec(N_STATES), s, a)
    ref = mountaincar_step64(s, a)
    ulp = np.array([np.spacing(np.float32(1.2)), np.spacing(np.float32(0.07))], np.float64)
    tol = MC_ULPS * ulp
    # near-ties: the position within the bound of the left wall (the v = 0 rule) or of the goal, or the velocity
    # (before the wall rule zeroes it) within the bound of 0, the sign both rules test
    tie = (np.abs(ref["pre_p"] + 1.2) < tol[0]) | (np.abs(ref["new"][:, 0] - 0.5) < tol[0]) \
        | (np.abs(ref["pre_v"]) < tol[1])
    print(f"mountaincar near-ties {tie.mean():.5%}")
    assert tie.mean() <= 1e-3
    ok = ~tie
    dev = np.abs(new.astype(np.float64) - ref["new"])[ok] / ulp
    print(f"mountaincar max deviation {dev[:, 0].max():.2f} / {dev[:, 1].max():.2f} ulp of the range")
    assert dev.max() <= MC_ULPS
    assert np.array_equal(term[ok], ref["term"][ok])
    assert ref["term"].any() and (ref["new"][:, 0] == -1.2).any() and (ref["new"][:, 0] == 0.6).any()


# ---------------------------------------------------------------------------------------------------------------
# scripted policies
# ---------------------------------------------------------------------------------------------------------------
def play(env, policy, steps):
    env.reset()
    rets = []
    for _ in range(steps):
        _, _, d, info = env.step(policy(env))
        rets.append(info["episode_return"][d])
    return torch.cat(rets).numpy()


def test_mountaincar_scripted_policies():
    push = play(MountainCarVec(512, seed=1), lambda e: torch.where(e.state[:, 1] >= 0, 2, 0), 400)
    assert len(push) >= 3 * 512
    assert push.min() >= -130 and push.max() <= -105, (push.min(), push.max())
    gen = torch.Generator().manual_seed(0)
    rnd = play(MountainCarVec(512, seed=2), lambda e: torch.randint(0, 3, (512,), generator=gen), 400)
    assert len(rnd) == 2 * 512 and (rnd == -200).all()


def test_acrobot_scripted_policies():
    swing = play(AcrobotVec(512, seed=1), lambda e: torch.where(e.state[:, 2] >= 0, 0, 2), 700)
    assert len(swing) >= 512
    assert swing.mean() >= -100, swing.mean()
    gen = torch.Generator().manual_seed(0)
    rnd = play(AcrobotVec(512, seed=2), lambda e: torch.randint(0, 3, (512,), generator=gen), 1000)
    assert len(rnd) >= 512 and rnd.mean() <= -450, rnd.mean()


# ---------------------------------------------------------------------------------------------------------------
# rules
# ---------------------------------------------------------------------------------------------------------------
def wang64(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x = (x ^ np.uint64(61)) ^ (x >> np.uint64(16))
    x = (x * np.uint64(9)) & m
    x = x ^ (x >> np.uint64(4))
    x = (x * np.uint64(0x27D4EB2D)) & m
    return x ^ (x >> np.uint64(15))


def reset_formula(seed, env_ids, counter, stream, scale, off):
    h = wang64(np.uint64(counter * 4 + stream))
    h = wang64(h ^ np.asarray(env_ids, np.uint64))
    h = wang64(h ^ np.uint64(seed))
    u = (h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u * np.float32(scale) - np.float32(off)


ENVS = [(AcrobotVec, 4, 0.2, 0.1, 6), (MountainCarVec, 1, 0.2, 0.6, 2)]


@pytest.mark.parametrize("cls,streams,scale,off,native", ENVS)
def test_reset_values_are_bit_equal_to_the_formula(cls, streams, scale, off, native):
    env = cls(37, seed=5)
    env.set_id_base(1000)
    env.reset()
    ids = np.arange(37) + 1000
    for s in range(env.state_dim):
        want = reset_formula(5, ids, 0, s, scale, off) if s < streams else np.zeros(37, np.float32)
        assert np.array_equal(env.state[:, s].numpy(), want)
    assert (env.counter == 1).all() and (env.steps == 0).all()
    # the shared hash agrees with the independent one above
    h = env_rand_u32(torch.tensor(5), torch.from_numpy(ids), torch.zeros(37, dtype=torch.int64), 0)
    assert np.array_equal(h.numpy().astype(np.uint64), wang64(wang64(wang64(np.uint64(0)) ^ ids.astype(np.uint64))
                                                              ^ np.uint64(5)))


@pytest.mark.parametrize("cls,streams,scale,off,native", ENVS)
def test_id_base_selects_the_envs_of_a_larger_batch(cls, streams, scale, off, native):
    big, part = cls(24, seed=3), cls(8, seed=3)
    part.set_id_base(10)
    ob, op = big.reset(), part.reset()
    assert torch.equal(ob[10:18], op)
    limit = 7
    big.max_episode_steps = part.max_episode_steps = limit          # several resets inside the run
    gen = torch.Generator().manual_seed(1)
    for _ in range(3 * limit):
        a = torch.randint(0, 3, (24,), generator=gen)
        ob, rb, db, ib = big.step(a)
        op, rp, dp, ip = part.step(a[10:18])
        assert torch.equal(ob[10:18], op) and torch.equal(db[10:18], dp) and torch.equal(rb[10:18], rp)
        assert torch.equal(ib["episode_return"][10:18], ip["episode_return"])
    assert (part.counter == 4).all()


@pytest.mark.parametrize("cls,streams,scale,off,native", ENVS)
def test_step_limit_auto_reset_and_episode_return(cls, streams, scale, off, native):
    env = cls(5, seed=9)
    env.reset()
    limit = env.max_episode_steps
    assert limit == (500 if cls is AcrobotVec else 200)
    idle = torch.ones(5, dtype=torch.long)          # no torque / no push: never reaches the goal from a reset
    for t in range(limit - 1):
        _, r, d, info = env.step(idle)
        assert not d.any() and (r == -1).all() and (info["episode_return"] == 0).all()
    obs, r, d, info = env.step(idle)
    assert d.all() and (info["episode_return"] == -float(limit)).all()
    # auto-reset: the second draw of every env's stream, fresh counters, and the observation is the new episode's
    assert (env.steps == 0).all() and (env.ep_ret == 0).all() and (env.counter == 2).all()
    for s in range(streams):
        assert np.array_equal(env.state[:, s].numpy(), reset_formula(9, np.arange(5), 1, s, scale, off))
    assert torch.equal(obs, env.observe())
    _, _, d, info = env.step(idle)
    assert not d.any() and (env.steps == 1).all() and (env.ep_ret == -1).all()


@pytest.mark.parametrize("cls,streams,scale,off,native", ENVS)
def test_action_of_three_or_more_plays_zero(cls, streams, scale, off, native):
    a, b = cls(16, seed=4), cls(16, seed=4)
    a.reset(), b.reset()
    for t in range(30):
        oa, ra, da, _ = a.step(torch.zeros(16, dtype=torch.long))
        ob, rb, db, _ = b.step(torch.full((16,), 3 + t % 5, dtype=torch.long))
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
    c = cls(16, seed=4)
    c.reset()
    for t in range(30):
        oc, _, _, _ = c.step(torch.full((16,), 2, dtype=torch.long))
    assert not torch.equal(oa, oc)


@pytest.mark.parametrize("cls,streams,scale,off,native", ENVS)
def test_obs_dim_pads_with_exact_zeros(cls, streams, scale, off, native):
    base, wide = cls(9, seed=2), cls(9, seed=2, obs_dim=8)
    assert base.obs_shape == (native,) and wide.obs_shape == (8,)
    ob, ow = base.reset(), wide.reset()
    for t in range(12):
        assert ow.shape == (9, 8) and ow.dtype == torch.float32
        assert torch.equal(ow[:, :native], ob) and (ow[:, native:] == 0).all()
        a = torch.full((9,), t % 3, dtype=torch.long)
        ob, ow = base.step(a)[0], wide.step(a)[0]
    for bad in (native - 1, 9, 0):
        with pytest.raises(ValueError, match=cls.id):
            cls(2, obs_dim=bad)
    if cls is AcrobotVec:
        s = base.state
        want = torch.stack([s[:, 0].cos(), s[:, 0].sin(), s[:, 1].cos(), s[:, 1].sin(), s[:, 2], s[:, 3]], 1)
        assert torch.equal(base.observe(), want)
    else:
        assert torch.equal(base.observe(), base.state)


def test_cartpole_obs_dim():
    base, wide = CartPoleVec(9, seed=2), CartPoleVec(9, seed=2, obs_dim=8)
    assert base.obs_shape == (4,) and wide.obs_shape == (8,)
    ob, ow = base.reset(), wide.reset()
    assert ob.shape == (9, 4)
    for t in range(40):
        assert torch.equal(ow[:, :4], ob) and (ow[:, 4:] == 0).all()
        assert torch.equal(ob, base.state)
        a = (torch.arange(9) + t) % 2
        (ob, rb, db, _), (ow, rw, dw, _) = base.step(a), wide.step(a)
        assert torch.equal(rb, rw) and torch.equal(db, dw)
    for bad in (3, 9):
        with pytest.raises(ValueError, match="CartPole-v1"):
            CartPoleVec(2, obs_dim=bad)


# ---------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------
def test_registry_ids_thresholds_and_presets():
    for env_id, thr, n_obs, limit in (("Acrobot-v1", -100.0, 6, 500), ("MountainCar-v0", -110.0, 2, 200)):
        env = make(env_id, num_envs=3, seed=1, frameskip=4, gray="rgb", no_op_max=7)
        assert env.id == env_id and env.num_actions == 3 and env.obs_shape == (n_obs,)
        assert env.reward_threshold == thr and reward_threshold(env_id) == thr and env.max_episode_steps == limit
        assert make(env_id, num_envs=3, obs_dim=8).reset().shape == (3, 8)
    assert make("CartPole-v1", num_envs=2, obs_dim=8).reset().shape == (2, 8)
    assert make("CartPole-v1", num_envs=2).reset().shape == (2, 4)
    single = {"acrobot": "Acrobot-v1", "mountaincar": "MountainCar-v0"}
    cart = preset("cartpole")
    for name, env_id in single.items():
        cfg = preset(name)
        assert cfg.tasks == [env_id] and cfg.env == env_id
        assert cfg.net.input_shape == (8,) and cfg.net.num_actions == 3 and cfg.net.trunk_scale == "none"
        assert (cfg.net.L, cfg.net.M, cfg.net.N) == (cart.net.L, cart.net.M, cart.net.N)
        assert [(l.kind, l.out) for l in cfg.net.layers] == [(l.kind, l.out) for l in cart.net.layers]
        assert (cfg.paths, cfg.envs_per_path, cfg.a2c) == (cart.paths, cart.envs_per_path, cart.a2c)
    cpu = preset("cartpole-cpu")
    for name in ("control3", "control3-cpu"):
        cfg = preset(name)
        assert cfg.tasks == ["CartPole-v1", "Acrobot-v1", "MountainCar-v0"] and cfg.env == "CartPole-v1"
        assert cfg.net.input_shape == (8,) and cfg.net.num_actions == 3 and cfg.net.trunk_scale == "none"
        assert (cfg.net.L, cfg.net.M, cfg.net.N, cfg.net.num_tasks) == (3, 8, 2, 3)
        assert [(l.kind, l.out) for l in cfg.net.layers] == [("fc", 32)] * 3
        assert 3 * cfg.net.N < cfg.net.M          # three frozen paths leave free modules in every layer
    cfg = preset("control3-cpu")
    assert (cfg.backend, cfg.compute_dtype, cfg.use_graph, cfg.paths, cfg.envs_per_path) == \
        (cpu.backend, cpu.compute_dtype, cpu.use_graph, cpu.paths, cpu.envs_per_path)
    assert preset("control3").backend == cart.backend


def test_cli_help_names_the_presets():
    import contextlib
    import io
    from pathnet_gym_amd import cli
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        cli.main(["train", "--help"])
    for name in ("acrobot", "mountaincar", "control3", "control3-cpu"):
        assert name in buf.getvalue()


def test_hip_evaluator_admits_the_three_ids():
    from pathnet_gym_amd.runtime.evaluator import unsupported_reason
    for name in ("acrobot", "mountaincar", "control3"):
        cfg = preset(name)
        for env_id in cfg.tasks:
            for dt in (None, "bf16", "fp32"):
                assert unsupported_reason(cfg.net, env_id, dt, 16) is None, (name, env_id, dt)
    assert unsupported_reason(preset("cartpole").net, "CartPole-v1", None, 1) is None
    why = unsupported_reason(preset("cartpole").net, "Acrobot-v1", None, 1)          # 4 inputs cannot hold 6 values
    assert why is not None and "Acrobot-v1" in why


def test_width_mismatch_is_refused_by_name():
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset("cartpole-cpu")
    cfg.env, cfg.tasks = "Acrobot-v1", ["Acrobot-v1"]
    cfg.net.num_actions = 3
    with pytest.raises(ValueError, match="Acrobot-v1"):
        PathNetTrainer(cfg)


def small3():
    cfg = preset("control3-cpu")
    cfg.paths, cfg.envs_per_path = 4, 4
    cfg.gc_freeze = False
    return cfg


def test_control3_cpu_runs_all_three_tasks_and_resumes(tmp_path):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.utils import checkpoint as ckpt
    torch.manual_seed(0)
    tr = PathNetTrainer(small3())
    lay = tr.model.store.layout
    frozen_seen = np.zeros((3, 8), bool)
    path = str(tmp_path / "ck.safetensors")
    for task, env_id in enumerate(["CartPole-v1", "Acrobot-v1", "MountainCar-v0"]):
        if task:
            tr._start_task(task)
        assert tr.env.id == env_id and tr.env.obs_shape == (8,) and tr.obs.shape == (16, 8)
        kept = tr.model.store.flat.detach().clone()
        for _ in range(4):
            st = tr.update()
            assert np.isfinite(st.loss_pi) and np.isfinite(st.loss_v)
        now = tr.model.store.flat.detach()
        for s in lay.segments:          # the paths frozen by the earlier tasks did not train
            if s.layer >= 0 and frozen_seen[s.layer, s.module]:
                assert torch.equal(now[s.offset:s.offset + s.numel], kept[s.offset:s.offset + s.numel]), s.name
        if task == 1:
            ckpt.save(tr, path)
            torch.manual_seed(77)
            for _ in range(3):
                tr.update()
            b = PathNetTrainer(small3())
            ckpt.load(b, path)
            assert b.task_idx == 1 and b.env.id == "Acrobot-v1"
            torch.manual_seed(77)
            for _ in range(3):
                b.update()
            assert torch.equal(tr.model.store.flat, b.model.store.flat)
            assert torch.equal(tr.env.state, b.env.state) and torch.equal(tr.obs, b.obs)
            assert np.array_equal(tr.pop.genotypes, b.pop.genotypes) and tr.global_step == b.global_step
        before = tr.model.store.flat.detach().clone()
        winner, frozen = tr.end_task()
        after = tr.model.store.flat.detach()
        assert (frozen[frozen_seen] > 0.5).all() and (frozen > 0.5).sum() > frozen_seen.sum()
        changed = 0
        for s in lay.segments:
            sl = slice(s.offset, s.offset + s.numel)
            if s.layer >= 0 and frozen[s.layer, s.module] > 0.5:
                assert torch.equal(after[sl], before[sl]), s.name              # frozen: bit-identical over the switch
            else:
                assert torch.equal(after[sl], tr.init_flat[sl]), s.name       # everything else re-initialised
                changed += int(not torch.equal(before[sl], after[sl]))
        assert changed > 0
        frozen_seen = frozen > 0.5
    assert (~frozen_seen).any(1).all()          # free modules left in every layer after three tasks


def test_train_crosses_both_task_boundaries():
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    tr = PathNetTrainer(small3())
    solved = tr.train(steps_per_task=160)
    assert set(solved) == {0, 1, 2} and tr.task_idx == 2 and tr.env.id == "MountainCar-v0"
    assert tr.global_step == 3 * 160


@pytest.mark.parametrize("env_id", ["CartPole-v1", "Acrobot-v1", "MountainCar-v0"])
def test_evaluate_path_torch_backend(env_id):
    from pathnet_gym_amd.algo.evaluate import evaluate_path
    from pathnet_gym_amd.models.pathnet import ParamStore
    net = preset("control3").net
    store = ParamStore(net, "cpu", seed=0)
    expr = np.zeros((net.L, net.M), np.float32)
    expr[:, :2] = 1
    limit = {"CartPole-v1": 500, "Acrobot-v1": 500, "MountainCar-v0": 200}[env_id]
    r = evaluate_path(net, store.flat.detach(), expr, env_id, episodes=4, seed=7, max_steps=limit, backend="torch")
    assert r["backend"] == "torch" and r["finished"] == 4
    lo, hi = (1, 500) if env_id == "CartPole-v1" else (-limit, -1)
    assert all(lo <= x <= hi for x in r["returns"])
    assert r == evaluate_path(net, store.flat.detach(), expr, env_id, episodes=4, seed=7, max_steps=limit,
                              backend="torch")


def test_game_state_steps_acrobot():
    from pathnet_gym_amd.envs.game_state import GameState
    gs = GameState(0, "Acrobot-v1")
    gs.process(1)
    assert gs.reward == -1.0 and not gs.terminal
    assert np.asarray(gs.s_t).size >= 6
    gs.update()
