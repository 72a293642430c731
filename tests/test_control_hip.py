"""The classic-control step kernels (csrc/control.hip) and the engine's vector path on them, on an MI355X.

Step parity.  The HIP env and the torch env (envs/control.py) are loaded with the same state before every compared
step (Acrobot is chaotic: two trajectories would drift apart), the states coming from the torch env's trajectory
under a shared random action stream, and from a uniform draw over the state box (the CPU test's states).  The float
state is held to the CPU test's criteria (tests/test_control_envs.py: deviation from the float64 reference in
fractions of the component's range, 99.9th percentile of angles / of velocities and the maximum), each bound being
4 x the torch env's own deviation measured on the same states: the device sinf / cosf and its FMA contraction differ
from the host's libm and separate roundings by a few ulp per call, and those differences are amplified by the
dynamics exactly as torch's own rounding is.  Observation rows (cos / sin of the angles) of the two backends are
compared to 1e-6, a few ulp of values of magnitude <= 1; the states of fresh episodes, and every other output, bit
for bit.  Steps, counter, reward, done, episode return and the states of fresh episodes are bit-equal outside
near-ties (float64 value within 1e-4 of the Acrobot height threshold or of a wrap edge, within 4 ulp of a MountainCar
threshold; <= 0.1 % left out).

Measured on an MI355X, in fractions of the range (torch env / HIP env on the same states):
  state box, N = 100003
    Acrobot      p99.9 angles 1.64e-6 / 1.54e-6   p99.9 velocities 5.69e-6 / 4.92e-6   maximum 3.36e-4 / 1.65e-4
    MountainCar  maximum position 5.30e-8 / 5.30e-8 (0.53 ulp of 1.2)   velocity 5.93e-8 / 5.93e-8 (0.56 ulp of 0.07)
  trajectories from a reset (64 steps, B = 1 ... 1000): states stay near rest, every figure is a few 1e-8
    Acrobot      maximum 1.0e-8 ... 3.0e-8 / 1.0e-8 ... 2.2e-8, the percentiles 0.9e-8 ... 1.6e-8 on both sides
    MountainCar  maximum 2.6e-8 and 1.8e-8, bit-equal on both sides at every B
"""
import numpy as np
import pytest
import torch

from pathnet_gym_amd.config import preset

import test_control_envs as tce

pytestmark = pytest.mark.gpu
DEV = "cuda"


def classes():
    from pathnet_gym_amd.envs.control import AcrobotVec, MountainCarVec
    return {"acrobot": AcrobotVec, "mountaincar": MountainCarVec}


def load_state(dst, state, steps, ep_ret, counter):
    """Install a state (device tensors) in a HIP or torch env."""
    from pathnet_gym_amd.ops import envs as henv
    dst.state = state.clone().float().contiguous()
    dst.steps = steps.clone().to(torch.int32)
    dst.ep_ret = ep_ret.clone().float()
    dst.counter = counter.clone().long()
    if dst.backend == "hip":
        henv.control_sync_to_device(dst)


def ref_step(name, s, a):
    """float64 outcome of one step from fp32 states ``s`` (numpy) -> (new state, terminal, near-tie mask)."""
    if name == "acrobot":
        r = tce.acrobot_step64(s, a)
        tie_h, tie_w = tce.acrobot_near_tie(r)
        return r["new"], r["term"], tie_h, tie_w
    r = tce.mountaincar_step64(s, a)
    ulp = np.array([np.spacing(np.float32(1.2)), np.spacing(np.float32(0.07))], np.float64)
    tol = tce.MC_ULPS * ulp
    tie = (np.abs(r["pre_p"] + 1.2) < tol[0]) | (np.abs(r["new"][:, 0] - 0.5) < tol[0]) | (np.abs(r["pre_v"]) < tol[1])
    return r["new"], r["term"], tie, np.zeros_like(tie)


def deviation(name, new32, ref64):
    if name == "acrobot":
        return tce.acrobot_dev(new32, ref64)
    return np.abs(np.asarray(new32, np.float64) - ref64) / tce.MC_RANGE


def hold_to_torch(name, dev_hip, dev_torch, where):
    """The CPU test's criteria with 4 x torch's own figure as the bound."""
    rows = []
    if name == "acrobot":
        groups = (("p99.9 angles", lambda d: np.percentile(d[:, :2], 99.9)),
                  ("p99.9 velocities", lambda d: np.percentile(d[:, 2:], 99.9)), ("max", lambda d: d.max()))
    else:
        groups = (("max position", lambda d: d[:, 0].max()), ("max velocity", lambda d: d[:, 1].max()))
    for label, f in groups:
        h, t = f(dev_hip), f(dev_torch)
        rows.append((label, t, h))
        print(f"{name} {where}: {label}: torch {t:.3e} hip {h:.3e} (bound {4 * t:.3e})")
    for label, t, h in rows:
        assert h <= 4.0 * t, (name, where, label, t, h)


def compare_step(name, et, eh, a, s_before, out_t, out_h, stats):
    """One compared step: discrete outputs bit-equal outside near-ties, reset states bit-equal, float deviations
    of the surviving states appended to ``stats``."""
    ot, rt, dt, it = out_t
    oh, rh, dh, ih = out_h
    ref_new, ref_term, tie, tie_w = ref_step(name, s_before.cpu().numpy(), a.cpu().numpy())
    ok = torch.from_numpy(~tie).to(DEV)
    stats["n"] += len(tie)
    stats["left_out"] += int(tie.sum())
    assert torch.equal(dt[ok], dh[ok]) and torch.equal(rt[ok], rh[ok])
    both = ok & (dt == dh)
    assert torch.equal(et.steps.int()[both], eh._steps32[both])
    assert torch.equal(et.counter.int()[both], eh._ctr32[both])
    done = both & dt
    assert torch.equal(it["episode_return"][done], ih["episode_return"][done])
    assert (ih["episode_return"][both & ~dt] == 0).all()
    assert torch.equal(et.state[done], eh.state[done])       # fresh episodes
    assert torch.allclose(ot[done], oh[done], atol=1e-6, rtol=0)
    live = (both & ~dt).cpu().numpy() & ~tie_w
    assert torch.equal(et.ep_ret[both], eh.ep_ret[both])
    if live.any():
        stats["torch"].append(deviation(name, et.state.cpu().numpy()[live], ref_new[live]))
        stats["hip"].append(deviation(name, eh.state.cpu().numpy()[live], ref_new[live]))
    # the observation rows are the env's own function of the state it holds
    assert torch.equal(oh, eh.observe())


@pytest.mark.parametrize("B", [1, 3, 255, 256, 257, 1000])
@pytest.mark.parametrize("name", ["acrobot", "mountaincar"])
def test_step_parity_on_a_torch_trajectory(hip_lib, name, B):
    cls = classes()[name]
    et = cls(B, device=DEV, seed=7, backend="torch")
    eh = cls(B, device=DEV, seed=7, backend="hip")
    et.set_id_base(5), eh.set_id_base(5)
    et.max_episode_steps = eh.max_episode_steps = 23          # the step limit ends episodes inside the run
    ot, oh = et.reset(), eh.reset()
    assert torch.equal(et.state, eh.state) and torch.allclose(ot, oh, atol=1e-6, rtol=0)
    gen = torch.Generator(device="cpu").manual_seed(B)
    stats = dict(n=0, left_out=0, torch=[], hip=[])
    for t in range(64):
        a = torch.randint(0, 5, (B,), generator=gen).to(DEV)          # 3 and 4 play 0
        s_before = et.state.clone()
        load_state(eh, et.state, et.steps, et.ep_ret, et.counter)
        compare_step(name, et, eh, a, s_before, et.step(a), eh.step(a), stats)
    assert stats["left_out"] <= 1e-3 * stats["n"]
    assert int(et.counter.min()) >= 3          # every env started at least two further episodes
    hold_to_torch(name, np.concatenate(stats["hip"]), np.concatenate(stats["torch"]), f"trajectory B={B}")


@pytest.mark.parametrize("name", ["acrobot", "mountaincar"])
def test_step_parity_over_the_state_box(hip_lib, name):
    """The CPU test's uniform states (terminal states, wraps and clamps included) in one launch of 391 workgroups."""
    N = 100_003
    cls = classes()[name]
    s, a = (tce.acrobot_states if name == "acrobot" else tce.mountaincar_states)(N, 21)
    et = cls(N, device=DEV, seed=1, backend="torch")
    eh = cls(N, device=DEV, seed=1, backend="hip")
    et.reset(), eh.reset()
    st = torch.from_numpy(s).to(DEV)
    for e in (et, eh):
        load_state(e, st, e.steps, e.ep_ret, e.counter)
    a = torch.from_numpy(a).to(DEV)
    stats = dict(n=0, left_out=0, torch=[], hip=[])
    out_t, out_h = et.step(a), eh.step(a)
    compare_step(name, et, eh, a, st, out_t, out_h, stats)
    assert stats["left_out"] <= 1e-3 * N
    assert bool(out_t[2].any()) and not bool(out_t[2].all())          # some episodes ended at the goal
    hold_to_torch(name, stats["hip"][0], stats["torch"][0], "state box")


def test_padded_cartpole_matches_the_torch_env(hip_lib):
    from pathnet_gym_amd.envs.cartpole import CartPoleVec
    for B in (3, 257):
        et = CartPoleVec(B, device=DEV, seed=3, backend="torch", obs_dim=8)
        eh = CartPoleVec(B, device=DEV, seed=3, backend="hip", obs_dim=8)
        ot, oh = et.reset(), eh.reset()
        assert torch.equal(ot, oh) and oh.shape == (B, 8)
        for i in range(40):
            a = (torch.arange(B, device=DEV) + i) % 3          # action 2 pushes left, as 0 does
            load_state(eh, et.state, et.steps, et.ep_ret, et.counter)
            ot, rt, dt, it = et.step(a)
            oh, rh, dh, ih = eh.step(a)
            assert torch.equal(dt, dh) and torch.equal(rt, rh)
            assert torch.equal(it["episode_return"], ih["episode_return"])
            assert torch.allclose(ot, oh, atol=1e-5) and (oh[:, 4:] == 0).all()
            assert torch.equal(ot[dt], oh[dt])          # fresh episodes: bit-equal resets
            assert torch.equal(et.counter.int(), eh._ctr32) and torch.equal(et.steps.int(), eh._steps32)
        assert int(et.counter.max()) > 1


# ---------------------------------------------------------------------------------------------------------------
# outputs, guard rows, launcher contract
# ---------------------------------------------------------------------------------------------------------------
def make_hip_env(name, B, seed=2, obs_dim=None):
    from pathnet_gym_amd.envs.cartpole import CartPoleVec
    if name == "cartpole":
        env = CartPoleVec(B, device=DEV, seed=seed, backend="hip", obs_dim=obs_dim or 4)
    else:
        env = classes()[name](B, device=DEV, seed=seed, backend="hip", obs_dim=obs_dim)
    env.reset()
    return env


def env_snapshot(env):
    from pathnet_gym_amd.ops import envs as henv
    if not hasattr(env, "_steps32"):
        henv.control_sync_to_device(env)
    return [x.clone() for x in (env.state, env._steps32, env.ep_ret, env._ctr32)]


def env_restore(env, snap):
    env.state.copy_(snap[0]), env._steps32.copy_(snap[1]), env.ep_ret.copy_(snap[2]), env._ctr32.copy_(snap[3])


GUARD = 3


def guarded(B, cols, dtype, fill):
    buf = torch.full((B + 2 * GUARD,) + ((cols,) if cols else ()), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + B]


def guards_untouched(buf, fill):
    g = torch.cat([buf[:GUARD].reshape(-1), buf[-GUARD:].reshape(-1)])
    return bool((g == fill).all())


@pytest.mark.parametrize("name,native", [("acrobot", 6), ("mountaincar", 2), ("cartpole", 4)])
def test_output_forms_and_guard_rows(hip_lib, name, native):
    from pathnet_gym_amd.ops import envs as henv
    B = 300
    env = make_hip_env(name, B)
    env.max_episode_steps = 4
    gen = torch.Generator().manual_seed(1)
    for step in range(6):          # the step limit resets every env inside the run
        a = torch.randint(0, 3, (B,), generator=gen).to(torch.int32).to(DEV)
        snap = env_snapshot(env)
        results = []
        for ld, want_f32, want_bf16 in ((native, True, True), (8, True, True), (8, True, False), (8, False, True),
                                        (7, True, True)):
            env_restore(env, snap)
            fbuf, f32 = guarded(B, ld, torch.float32, 77.0)
            bbuf, b16 = guarded(B, 8, torch.bfloat16, 77.0)
            rbuf, r = guarded(B, 0, torch.float32, 77.0)
            dbuf, d = guarded(B, 0, torch.uint8, 77)
            ebuf, e = guarded(B, 0, torch.float32, 77.0)
            henv.control_step_into(env, a, b16 if want_bf16 else None, r, d, e, obs_f32_out=f32 if want_f32 else None,
                                   obs_ld=ld)
            torch.cuda.synchronize()
            assert guards_untouched(fbuf, 77.0) and guards_untouched(bbuf, 77.0) and guards_untouched(rbuf, 77.0)
            assert guards_untouched(dbuf, 77) and guards_untouched(ebuf, 77.0)
            if want_f32:
                assert torch.equal(f32[:, :native], env.observe()[:, :native]) and (f32[:, native:] == 0).all()
                if want_bf16:
                    assert torch.equal(b16.view(torch.int16), henv.obs_to_bf16_padded(f32).view(torch.int16))
            else:
                assert (f32 == 77.0).all()          # a null pointer: nothing written
            if not want_bf16:
                assert (b16 == 77.0).all()
            else:
                assert torch.equal(b16.view(torch.int16),
                                   henv.obs_to_bf16_padded(env.observe()[:, :native]).view(torch.int16))
            results.append([x.clone() for x in (env.state, env._steps32, env.ep_ret, env._ctr32, r, d, e)])
        for other in results[1:]:          # the state and the scalar outputs do not depend on the output form
            assert all(torch.equal(x, y) for x, y in zip(results[0], other))
    assert int(env._ctr32.min()) >= 2


@pytest.mark.parametrize("name,native", [("acrobot", 6), ("mountaincar", 2), ("cartpole", 4)])
def test_launcher_contract(hip_lib, name, native):
    """Every refused call returns -22 and writes nothing."""
    from pathnet_gym_amd.ops import _lib, envs as henv
    B = 5
    env = make_hip_env(name, B)
    fn = getattr(_lib.lib(), henv.control_launcher(env))
    a = torch.zeros(B, dtype=torch.int32, device=DEV)
    f32 = torch.full((B, 8), 77.0, device=DEV)
    b16 = torch.full((B, 8), 77.0, dtype=torch.bfloat16, device=DEV)
    r = torch.full((B,), 77.0, device=DEV)
    d = torch.full((B,), 77, dtype=torch.uint8, device=DEV)
    e = torch.full((B,), 77.0, device=DEV)
    snap = env_snapshot(env)

    def args(**kw):
        v = dict(state=env.state.data_ptr(), steps=env._steps32.data_ptr(), epret=env.ep_ret.data_ptr(),
                 counter=env._ctr32.data_ptr(), actions=a.data_ptr(), B=B, seed=1, id_base=0, max_steps=10,
                 obs_f32=f32.data_ptr(), obs_ld=8, obs_bf16=b16.data_ptr(), reward=r.data_ptr(), done=d.data_ptr(),
                 epret_out=e.data_ptr(), stream=_lib.stream())
        v.update(kw)
        return list(v.values())

    bad = [dict(B=0), dict(B=-1), dict(max_steps=-1), dict(obs_ld=native - 1), dict(obs_ld=9), dict(obs_ld=0),
           dict(obs_ld=-8)]
    bad += [{k: None} for k in ("state", "steps", "epret", "counter", "actions", "reward", "done", "epret_out")]
    for kw in bad:
        assert fn(*args(**kw)) == -22, kw
    torch.cuda.synchronize()
    for x, y in zip(env_snapshot(env), snap):
        assert torch.equal(x, y)
    assert (f32 == 77.0).all() and (b16 == 77.0).all() and (r == 77.0).all() and (d == 77).all() and (e == 77.0).all()
    # the same buffers are accepted, and written, by a valid call; either observation pointer may be null
    assert fn(*args(obs_f32=None, obs_bf16=None)) == 0
    assert fn(*args()) == 0
    torch.cuda.synchronize()
    assert (r != 77.0).all() and (f32[:, native:] == 0).all()
    with pytest.raises(ValueError):
        henv.control_step_into(env, a, None, r, d, e, obs_f32_out=f32, obs_ld=9)
    with pytest.raises(TypeError):
        (henv.mountaincar_step_into if name == "acrobot" else henv.acrobot_step_into)(env, a, None, r, d, e)


@pytest.mark.parametrize("name", ["acrobot", "mountaincar", "cartpole"])
def test_600_step_device_run(hip_lib, name):
    B, T = 300, 600
    limit = {"acrobot": 500, "mountaincar": 200, "cartpole": 500}[name]
    gen = torch.Generator().manual_seed(5)
    acts = torch.randint(0, 3, (T, B), generator=gen).to(DEV)
    runs = []
    for _ in range(2):
        env = make_hip_env(name, B, seed=9, obs_dim=8)
        assert env.max_episode_steps == limit
        c0 = env.counter.clone()
        dones, rets = [], []
        for t in range(T):
            o, r, d, info = env.step(acts[t])
            dones.append(d)
            rets.append(info["episode_return"])
        torch.cuda.synchronize()
        dones, rets = torch.stack(dones), torch.stack(rets)
        ended = rets[dones]
        assert len(ended) >= B and (rets[~dones] == 0).all()
        if name == "cartpole":
            assert ended.min() >= 1 and ended.max() <= limit
        else:
            assert ended.min() >= -limit and ended.max() <= -1
        if name == "mountaincar":
            assert (ended == -200).all()          # a random policy never reaches the flag
        assert torch.equal(dones.sum(0).int(), env._ctr32 - c0.int())
        assert torch.isfinite(o).all() and o.shape == (B, 8)
        assert (o[:, {"acrobot": 6, "mountaincar": 2, "cartpole": 4}[name]:] == 0).all()
        runs.append((dones, rets, o, env.state.clone(), env._steps32.clone(), env._ctr32.clone(), env.ep_ret.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))


# ---------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------
CAP = 7          # episode cap in agent steps: episodes end inside every second rollout of T = 5


def trainer(name, dtype, graph, paths=4, monkeypatch=None, light_seed=1):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset(name)
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = paths, 4, 5
    cfg.backend = "hip"
    cfg.compute_dtype = dtype
    cfg.use_graph = graph
    cfg.deterministic = True          # ordered weight gradients: two runs are bit-equal
    cfg.seed = cfg.ga.seed = light_seed
    cfg.gc_freeze = False
    tr = PathNetTrainer(cfg, device="cuda:0")
    assert tr.compute_dtype == dtype and tr.engine.use_graph == graph and not tr.engine.pixels
    assert tr.env.obs_shape == (8,) and tr.env.backend == "hip"
    tr.env.max_episode_steps = CAP
    return tr


def engine_state(tr):
    from pathnet_gym_amd.ops import envs as henv
    env, eng = tr.env, tr.engine
    if not hasattr(env, "_steps32"):          # a restored env that has not stepped yet
        henv.control_sync_to_device(env)
    return [tr.model.store.flat.detach().clone(), env.state.clone(), env._steps32.clone(), env._ctr32.clone(),
            env.ep_ret.clone(), eng.fitness.clone(), eng.obs_stack(0).clone()]


PRESETS = ["acrobot", "mountaincar", "control3"]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", PRESETS)
def test_captured_updates_equal_eager_ones(hip_lib, name, dtype):
    out = []
    for graph in (False, True):
        tr = trainer(name, dtype, graph)
        w0 = tr.model.store.flat.detach().clone()
        for _ in range(3):
            st = tr.update()
            assert np.isfinite(st.loss_pi) and np.isfinite(st.loss_v)
        tr.flush()
        torch.cuda.synchronize()
        assert (tr.engine.g_rollout is not None) == graph
        out.append(engine_state(tr))
        assert torch.isfinite(out[-1][0]).all() and not torch.equal(out[-1][0], w0)
        assert int(tr.env._ctr32.min()) >= 3          # the cap ended episodes
        tr.env.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["acrobot", "control3"])
def test_fp32x_takes_the_fp32_engine(hip_lib, name):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset(name)
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 4, 4, 5
    cfg.backend, cfg.compute_dtype, cfg.gc_freeze = "hip", "fp32x", False
    with pytest.warns(UserWarning, match="fp32 engine"):
        tr = PathNetTrainer(cfg, device="cuda:0")
    assert tr.compute_dtype == "fp32" and tr.precision_note.startswith("fp32x -> fp32")
    assert tr.engine._obs_bufs[0].dtype == torch.float32 and tr.engine._obs_bufs[0].shape[-1] == 8
    st = tr.update()
    tr.flush()
    assert np.isfinite(st.loss_pi)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", PRESETS)
def test_rollout_equals_stepping_the_env_by_hand(hip_lib, name, dtype):
    from pathnet_gym_amd.ops import envs as henv
    tr = trainer(name, dtype, False)
    eng, env = tr.engine, tr.env
    tr.update()
    for rollout in range(2):          # both parities of the observation double buffer
        torch.cuda.synchronize()
        snap = env_snapshot(env)
        obs0 = eng.obs_stack(0).clone()
        eng._rollout_backward_body()
        torch.cuda.synchronize()
        after = env_snapshot(env)
        obs = eng.obs_stacks().clone()
        assert torch.equal(obs[0], obs0)
        env_restore(env, snap)
        B, ended = eng.B, 0
        for t in range(eng.T):
            f32 = torch.empty(B, 8, device=DEV)
            r, e = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
            d = torch.empty(B, dtype=torch.uint8, device=DEV)
            henv.control_step_into(env, eng.actions[t].contiguous(), None, r, d, e, obs_f32_out=f32, obs_ld=8)
            want = f32 if dtype == "fp32" else henv.obs_to_bf16_padded(f32)
            assert torch.equal(obs[t + 1].view(torch.int32 if dtype == "fp32" else torch.int16),
                               want.view(torch.int32 if dtype == "fp32" else torch.int16)), t
            assert torch.equal(eng.rewards[t], r) and torch.equal(eng.dones[t], d) and torch.equal(eng.epret[t], e)
            ended += int(d.sum())
        for x, y in zip(env_snapshot(env), after):
            assert torch.equal(x, y)
        assert int(eng.actions[:eng.T].max()) <= 2 and len(set(eng.actions[:eng.T].reshape(-1).tolist())) > 1
        eng._par ^= 1          # what the optimizer step does: the next rollout starts in the other buffer
        eng.ctr.add_(1)
    assert ended > 0
    # the slot-0 observation of a fresh engine is the env's padded observation, not its state
    assert torch.equal(eng._vector_obs(env), env.observe()) and env.observe().shape == (eng.B, 8)


@pytest.mark.parametrize("name,dtype,light", [("acrobot", "bf16", False), ("acrobot", "fp32", True),
                                              ("mountaincar", "fp32", False), ("mountaincar", "bf16", True),
                                              ("control3", "bf16", True), ("control3", "fp32", False)])
def test_checkpoint_resume_is_exact(hip_lib, tmp_path, name, dtype, light):
    from pathnet_gym_amd.utils import checkpoint
    tr = trainer(name, dtype, True)
    if name == "control3":          # resume inside the second task
        tr.update()
        tr.end_task()
        tr._start_task(1)
        tr.env.max_episode_steps = CAP
        assert tr.env.id == "Acrobot-v1"
    for _ in range(3):          # an odd count: the saved observation sits in the second buffer
        tr.update()
    tr.flush()
    path = checkpoint.save(tr, str(tmp_path / "ck.safetensors"), light=light)
    saved = engine_state(tr)
    for _ in range(2):
        tr.update()
    tr.flush()
    torch.cuda.synchronize()
    tr2 = trainer(name, dtype, True)
    checkpoint.load(tr2, path)
    tr2.env.max_episode_steps = CAP
    assert tr2.task_idx == tr.task_idx and tr2.env.id == tr.env.id
    for x, y in zip(engine_state(tr2), saved):
        assert torch.equal(x, y)
    for _ in range(2):
        tr2.update()
    tr2.flush()
    torch.cuda.synchronize()
    for x, y in zip(engine_state(tr2), engine_state(tr)):
        assert torch.equal(x, y)
    assert not torch.equal(saved[0], tr.model.store.flat)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_control3_crosses_both_task_boundaries(hip_lib, monkeypatch, dtype):
    from pathnet_gym_amd.envs.cartpole import CartPoleVec
    for cls in (CartPoleVec,) + tuple(classes().values()):
        monkeypatch.setattr(cls, "max_episode_steps", CAP)          # every task's env ends episodes early
    tr = trainer("control3", dtype, True)
    lay = tr.model.store.layout
    seen = []
    frozen_prev = np.zeros((3, 8), bool)
    for task, env_id in enumerate(["CartPole-v1", "Acrobot-v1", "MountainCar-v0"]):
        if task:
            tr._start_task(task)
        assert tr.env.id == env_id and tr.env.obs_shape == (8,)
        kept = tr.model.store.flat.detach().clone()
        for _ in range(4):
            tr.update()
        tr.flush()
        torch.cuda.synchronize()
        assert tr.engine.g_rollout is not None
        now = tr.model.store.flat.detach()
        assert torch.isfinite(now).all()
        for s in lay.segments:
            if s.layer >= 0 and frozen_prev[s.layer, s.module]:
                assert torch.equal(now[s.offset:s.offset + s.numel], kept[s.offset:s.offset + s.numel]), s.name
        before = now.clone()
        winner, frozen = tr.end_task()
        after = tr.model.store.flat.detach()
        for s in lay.segments:
            sl = slice(s.offset, s.offset + s.numel)
            if s.layer >= 0 and frozen[s.layer, s.module] > 0.5:
                assert torch.equal(after[sl], before[sl]), s.name
            else:
                assert torch.equal(after[sl], tr.init_flat[sl]), s.name
        frozen_prev = frozen > 0.5
        seen.append(env_id)
    assert len(seen) == 3 and (~frozen_prev).any(1).all()
    # and the trainer's own loop
    tr2 = trainer("control3", dtype, True)
    solved = tr2.train(steps_per_task=3 * 4 * 4 * 5)
    assert set(solved) == {0, 1, 2} and tr2.task_idx == 2 and tr2.env.id == "MountainCar-v0"
    assert tr2.global_step == 3 * 3 * 4 * 4 * 5 and torch.isfinite(tr2.model.store.flat).all()


@pytest.mark.parametrize("name,dtype", [("acrobot", "bf16"), ("mountaincar", "fp32"), ("control3", "bf16")])
def test_two_half_populations_reproduce_the_whole(hip_lib, name, dtype):
    """Envs and sampling rows are keyed by their global index: paths [2k, 2k + 2) with id_base = row_base = 8 k
    roll out exactly what they do inside the population of four."""
    from pathnet_gym_amd.runtime.engine import HipEngine
    whole = trainer(name, dtype, False)
    masks = whole.model.mask.cpu().numpy().copy()
    flat = whole.model.store.flat.detach().clone()
    E, T = 4, 5

    def roll(tr, n):
        rec = []
        for _ in range(n):
            tr.engine._rollout_backward_body()
            torch.cuda.synchronize()
            e = tr.engine
            rec.append([x.clone() for x in (e.obs_stacks(), e.actions[:T], e.rewards, e.dones, e.epret, e.logits[:T])])
            e._par ^= 1
            e.ctr.add_(1)
        return rec

    want = roll(whole, 3)
    assert sum(int(r[3].sum()) for r in want) > 0
    for k in range(2):
        half = trainer(name, dtype, False, paths=2)
        base = k * 2 * E
        half.env_base = base
        half.env = half._make_env(0)
        assert half.env.id_base == base
        half.env.reset()
        half.env.max_episode_steps = CAP
        with torch.no_grad():
            half.model.store.flat.copy_(flat)
        half.model.set_paths(masks[2 * k:2 * k + 2])
        half.model.hip.refresh_weights()
        half.engine = HipEngine(half.model, half.env, half.cfg, half.opt, seed=half._sample_seed(0), row_base=base)
        got = roll(half, 3)
        sl = slice(base, base + 2 * E)
        for w, g in zip(want, got):
            for x, y in zip(w, g):
                assert torch.equal(x[:, sl], y)
    wrong = trainer(name, dtype, False, paths=2)          # the second half's paths under the first half's indices
    wrong.model.set_paths(masks[2:4])
    wrong.model.hip.refresh_weights()
    assert not torch.equal(roll(wrong, 1)[0][0], want[0][0][:, 8:16])


# ---------------------------------------------------------------------------------------------------------------
# evaluator
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre,env_id,dtype", [("acrobot", "Acrobot-v1", "bf16"), ("acrobot", "Acrobot-v1", "fp32"),
                                              ("mountaincar", "MountainCar-v0", "bf16"),
                                              ("mountaincar", "MountainCar-v0", "fp32"),
                                              ("control3", "CartPole-v1", "bf16"), ("control3", "CartPole-v1", "fp32"),
                                              ("control3", "MountainCar-v0", "fp32")])
def test_hip_evaluator(hip_lib, pre, env_id, dtype):
    from pathnet_gym_amd.envs.registry import make
    from pathnet_gym_amd.runtime.evaluator import HipEvaluator, unsupported_reason
    from test_hip_evaluator import masks, same, snapshot
    net = preset(pre).net
    P, E, T = 4, 2, 5
    assert unsupported_reason(net, env_id, dtype, E) is None

    def build(use_graph):
        ev = HipEvaluator(net, env_id, P, E, chunk=T, device=DEV, compute_dtype=dtype, env_seed=3,
                          use_graph=use_graph)
        ev.env.max_episode_steps = 9
        assert ev.env.obs_shape == (8,) and ev.compute_dtype == dtype
        ev.load(ev.model.store.flat.detach().clone(), masks(P, net, 0), 0)
        return ev

    kw = dict(quota=3, max_steps=200, sample=True, seed=11)
    g, e = build(True), build(False)
    try:
        a = snapshot(g, **kw)
        assert g._graphs is not None
        b = snapshot(e, **kw)
        assert same(a, b) and same(a, snapshot(g, **kw)) and a[1].min() >= 3
        assert not same(a, snapshot(g, **dict(kw, seed=12)))
        # the same episodes on a HIP env of its own, driven by the recorded actions: the ledger's returns
        rec = []
        rets = e.run(record=rec, **kw)
        twin = make(env_id, num_envs=P * E, device=DEV, seed=3, backend="hip", obs_dim=8)
        twin.max_episode_steps = 9
        obs = twin.reset()
        want = [[] for _ in range(P * E)]
        for chunk in rec:
            for t in range(T):
                seen = chunk["obs"][t]
                exp = obs if dtype == "fp32" else obs.to(torch.bfloat16)
                assert torch.equal(seen.float()[:, :8], exp.float())
                obs, _, d, info = twin.step(chunk["actions"][t])
                assert torch.equal(d, chunk["dones"][t].bool())
                assert torch.equal(info["episode_return"], chunk["epret"][t])
                for i in d.nonzero().flatten().tolist():
                    want[i].append(float(info["episode_return"][i]))
        for i in range(P * E):
            assert rets[i] == want[i][:3], i
    finally:
        g.close()
        e.close()
