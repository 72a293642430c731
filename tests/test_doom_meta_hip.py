"""Synthetic meta-Doom on the device: the mixed-level step kernel (csrc/games.hip meta_step_kernel) against the torch
oracle (envs/doom_meta_games.py) on the run that tests/test_doom_meta_games.py builds and checks, the reset by mask,
the rasteriser with one gray table per level (csrc/preprocess.hip, the ``_lv`` launchers) against the single-table
launchers, the launchers' contracts, the global-index RNG identity, the engine on ``doom-meta`` and the evaluator."""
import numpy as np
import pytest
import torch

from pathnet_gym_amd.envs import registry
from pathnet_gym_amd.envs.doom_meta_games import NH, NL
from test_doom_meta_games import CAP, ENV_FULL, ENV_SHORT, ID_BASE, N_MIX, mixed_actions, mixed_env, play_mixed

pytestmark = pytest.mark.gpu
DEV = "cuda"


def scene16(env):
    return env.scene_rects().clamp(-32768, 32767).to(torch.int16)


def hip_twin(cpu, n=None, lo=0, id_base=ID_BASE):
    """A HIP env that adopts rows [lo, lo + n) of the oracle's packed state (taken before its first reset)."""
    n = cpu.num_envs if n is None else n
    hip = mixed_env(n=n, id_base=id_base, device=DEV, backend="hip")
    assert hip._hip and hip.supports_ring
    hip.load_packed(cpu._hip_pack()[lo:lo + n].to(DEV))
    return hip


def same_state(cpu, hip):
    assert torch.equal(hip._st32.cpu(), cpu._hip_pack())
    assert torch.equal(hip._lv8.cpu().long(), cpu.level)
    assert torch.equal(hip._rects.cpu(), scene16(cpu))
    assert torch.equal(hip.obs.cpu(), cpu.obs)


def test_hip_mixed_levels_match_the_oracle(hip_lib):
    cpu = mixed_env(reset=False)
    hip = hip_twin(cpu)
    assert torch.equal(cpu.reset(), hip.reset().cpu())
    same_state(cpu, hip)
    assert sorted(hip._lv8.tolist()) == sorted(list(range(NL)) * 4)

    def on_step(t, a, out):
        oc, rc, dc, ic = out
        oh, rh, dh, ih = hip.step(a.to(DEV))
        assert torch.equal(oh.cpu(), oc), t
        assert torch.equal(rh.cpu(), rc) and torch.equal(dh.cpu(), dc), t
        assert torch.equal(ih["episode_return"].cpu(), ic["episode_return"]), t
        same_state(cpu, hip)

    into, unlocks = play_mixed(cpu, on_step)
    assert min(into) >= 1, into                                # a level change into each of the nine levels
    assert unlocks >= 1
    assert int(cpu.unlocked[ENV_SHORT]) & 0b10 and int(cpu.total5[ENV_FULL]) == 47250
    hi, ci = hip.meta_info(), cpu.meta_info()
    for k in ci:
        assert torch.equal(hi[k].cpu(), ci[k]), k
    for l, (sub_h, sub_c) in enumerate(zip(hip.subs, cpu.subs)):      # the unpacker: the states of the envs on level l
        on = cpu.level == l
        for name, _ in sub_c.HIP_FIELDS:
            assert torch.equal(getattr(sub_h, name).cpu()[on], getattr(sub_c, name)[on]), name


def test_reset_by_mask_leaves_the_other_rows_alone(hip_lib):
    cpu = mixed_env(reset=False)
    hip = hip_twin(cpu)
    cpu.reset()
    hip.reset()
    acts = mixed_actions()
    for t in range(5):
        cpu.step(acts[t])
        hip.step(acts[t].to(DEV))
    before = hip._st32.clone()
    m = torch.zeros(N_MIX, dtype=torch.bool)
    m[::3] = True
    m[ENV_FULL] = True
    cpu.reset_where(m)
    hip.reset_where(m.to(DEV))
    same_state(cpu, hip)
    after = hip._st32.cpu()
    assert torch.equal(after[~m], before.cpu()[~m])
    j = hip.NSU
    assert torch.equal(after[:, j:j + 4 + NL * NH], before.cpu()[:, j:j + 4 + NL * NH])      # the ledger stays
    assert (after[m][:, -2:] == 0).all() and torch.equal(after[m][:, -3], before.cpu()[m][:, -3] + 1)
    assert not torch.equal(after[m][:, :j], before.cpu()[m][:, :j])


def test_change_level_reaches_the_kernel(hip_lib):
    cpu = mixed_env(reset=False)
    hip = hip_twin(cpu)
    cpu.reset()
    hip.reset()
    want = torch.arange(N_MIX) % 5                              # levels 0..4: locked for some envs, open for others
    m = torch.arange(N_MIX) % 2 == 0
    cpu.change_level(want, m)
    hip.change_level(want.to(DEV), m.to(DEV))
    assert torch.equal(hip._st32.cpu(), cpu._hip_pack())
    acts = mixed_actions()
    for t in range(CAP + 1):
        cpu.step(acts[t])
        hip.step(acts[t].to(DEV))
        same_state(cpu, hip)
    used = m & (cpu.req == -1)
    assert used.any() and torch.equal(cpu.level[used], want[used])     # one step after the cap: still on that level
    assert (m & (cpu.req != -1)).any()                         # and a request for a locked level is still pending
    hip.sync_from_device()
    assert torch.equal(hip.req.cpu(), cpu.req)


# ------------------------------------------------------------------------------------------- rasteriser
def _scenes(n=19):
    """Real scenes of n envs on mixed levels, a few steps into their episodes."""
    cpu = mixed_env(reset=False)
    hip = hip_twin(cpu, n=n)
    hip.reset()
    acts = mixed_actions()
    for t in range(4):
        hip.step(acts[t, :n].to(DEV))
    return hip


@pytest.mark.parametrize("banded", [0, 2])
def test_per_level_gray_tables_against_the_single_table_launcher(hip_lib, banded):
    from pathnet_gym_amd.ops import envs as henv
    env = _scenes()
    N, RU = 19, env.RU
    rects, lv, tab = env._rects, env._lv8, env._gray_tab
    assert tab.shape == (NL, RU) and len(set(lv.tolist())) == NL
    g = torch.Generator().manual_seed(1)
    obs_in = torch.randint(0, 256, (N, 160, 120, 4), dtype=torch.uint8, generator=g).to(DEV)
    reset = (torch.arange(N) % 2 == 0).to(torch.uint8).to(DEV)
    S, slot = 6, 4
    fc_in = torch.randint(0, 4, (N,), dtype=torch.uint8, generator=g).to(DEV)

    def packed(levels, table, rs):
        out = torch.zeros_like(obs_in)
        henv.rects16_stack_push_lv(rects, table, levels, env._bg_gray, obs_in, out, rs, env._tab32)
        return out

    def ring(levels, table, rs):
        frames = torch.zeros(N, S, 160 * 120, dtype=torch.uint8, device=DEV)
        fc = torch.zeros(N, dtype=torch.uint8, device=DEV)
        henv.rects16_ring_push_lv(rects, table, levels, env._bg_gray, frames, slot, fc_in, fc, rs, env._tab32)
        return frames, fc

    hip_lib.rects_set_banded(banded)
    try:
        for rs in (reset, None):
            want = torch.zeros_like(obs_in)
            want_fr = torch.zeros(N, S, 160 * 120, dtype=torch.uint8, device=DEV)
            want_fc = torch.zeros(N, dtype=torch.uint8, device=DEV)
            for l in range(NL):                                # the existing launcher, level by level, padded RU
                on = (lv == l).nonzero().flatten()
                sub_rs = None if rs is None else rs[on].contiguous()
                o = torch.zeros(len(on), 160, 120, 4, dtype=torch.uint8, device=DEV)
                henv.rects16_stack_push(rects[on].contiguous(), tab[l].contiguous(), env._bg_gray,
                                        obs_in[on].contiguous(), o, sub_rs, env._tab32)
                want[on] = o
                fr = torch.zeros(len(on), S, 160 * 120, dtype=torch.uint8, device=DEV)
                fc = torch.zeros(len(on), dtype=torch.uint8, device=DEV)
                henv.rects16_ring_push(rects[on].contiguous(), tab[l].contiguous(), env._bg_gray, fr, slot,
                                       fc_in[on].contiguous(), fc, sub_rs, env._tab32)
                want_fr[on], want_fc[on] = fr, fc
            got = packed(lv, tab, rs)
            assert torch.equal(got, want)
            fr, fc = ring(lv, tab, rs)
            assert torch.equal(fr, want_fr) and torch.equal(fc, want_fc)
            assert torch.equal(fr[:, slot].view(N, 160, 120), got[..., 3])
            # NL = 1: every level word is clamped to the only row
            one = tab[4:5].contiguous()
            o1 = torch.zeros_like(obs_in)
            henv.rects16_stack_push(rects, one[0].contiguous(), env._bg_gray, obs_in, o1, rs, env._tab32)
            assert torch.equal(packed(lv, one, rs), o1)
            f1 = torch.zeros_like(want_fr)
            c1 = torch.zeros_like(want_fc)
            henv.rects16_ring_push(rects, one[0].contiguous(), env._bg_gray, f1, slot, fc_in, c1, rs, env._tab32)
            r1 = ring(lv, one, rs)
            assert torch.equal(r1[0], f1) and torch.equal(r1[1], c1)
            # negative controls: levels rotated by one, two rows of the table swapped
            rot = ((lv + 1) % NL).contiguous()
            assert not torch.equal(packed(rot, tab, rs), want)
            assert not torch.equal(ring(rot, tab, rs)[0], want_fr)
            swapped = tab.clone()
            swapped[[0, 8]] = tab[[8, 0]]
            assert not torch.equal(packed(lv, swapped, rs), want)
            assert not torch.equal(ring(lv, swapped, rs)[0], want_fr)
    finally:
        hip_lib.rects_set_banded(1)                            # the default (auto)


# ------------------------------------------------------------------------------------------- launcher contracts
def test_launchers_refuse_bad_arguments(hip_lib):
    from pathnet_gym_amd.ops import _lib
    env = _scenes(4)
    N, st = 4, _lib.stream()
    a = torch.zeros(N, dtype=torch.int32, device=DEV)
    m8 = torch.ones(N, dtype=torch.uint8, device=DEV)
    rw, ep = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    dn = torch.zeros(N, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()                                                   # noqa: E731

    def meta(state=p(env._st32), table=p(env._level_tab), actions=p(a), mask=None, mode=0, n=N, rects=p(env._rects),
             level_out=p(env._lv8)):
        return hip_lib.launch_meta_step(state, table, actions, mask, mode, n, 1, 0, 4, CAP, p(rw), p(dn), p(ep), rects,
                                        level_out, st)

    before = env._st32.clone()
    assert meta(n=0) == -22 and meta(n=-3) == -22
    assert meta(state=None) == -22 and meta(table=None) == -22
    assert meta(rects=None) == -22 and meta(level_out=None) == -22
    assert meta(actions=None) == -22                           # mode 0 without actions
    assert meta(mode=1, mask=None) == -22                      # mode 1 without a mask
    assert meta(mode=2, mask=p(m8)) == -22
    torch.cuda.synchronize()
    assert torch.equal(env._st32, before)
    assert meta() == 0 and meta(mode=1, actions=None, mask=p(m8)) == 0
    ns, nr, nl = (torch.zeros(1, dtype=torch.int32).numpy() for _ in range(3))
    assert hip_lib.meta_layout(ns.ctypes.data, nr.ctypes.data, nl.ctypes.data) == 0
    assert (int(ns[0]), int(nr[0]), int(nl[0])) == (env._st32.shape[1], env.RU, NL)
    assert hip_lib.meta_layout(None, nr.ctypes.data, nl.ctypes.data) == -22

    obs = torch.zeros(N, 160, 120, 4, dtype=torch.uint8, device=DEV)
    out = torch.zeros_like(obs)
    fr = torch.zeros(N, 5, 160 * 120, dtype=torch.uint8, device=DEV)
    fc = torch.zeros(N, dtype=torch.uint8, device=DEV)

    def push(level=p(env._lv8), nl=NL, r=env.RU, n=N):
        return hip_lib.launch_rects_stack_push_lv(p(env._rects), p(env._gray_tab), level, nl, r, env._bg_gray, p(obs),
                                                  p(out), None, p(env._tab32), n, st)

    def ring(level=p(env._lv8), nl=NL, r=env.RU, n=N, frames=p(fr), stride=fr.stride(0), fi=p(fc), fo=p(fc)):
        return hip_lib.launch_rects_ring_push_lv(p(env._rects), p(env._gray_tab), level, nl, r, env._bg_gray, frames,
                                                 stride, fi, fo, None, p(env._tab32), n, st)

    for f in (push, ring):
        assert f(nl=0) == -22 and f(nl=-1) == -22 and f(level=None) == -22
        assert f(r=-1) == -22 and f(r=513) == -22 and f(n=0) == -22
        assert f() == 0
    assert ring(frames=None) == -22 and ring(fi=None) == -22 and ring(fo=None) == -22
    assert ring(stride=160 * 120 - 4) == -22 and ring(stride=160 * 120 + 2) == -22
    torch.cuda.synchronize()


def test_a_corrupt_level_word_stays_inside_its_row(hip_lib):
    """``level = 250`` plays as the last level and touches nothing outside the env's row, scene and level byte:
    sentinel rows around all three."""
    from pathnet_gym_amd.ops import _lib
    env = _scenes(9)
    N, NS, RU, BAD = 9, env._st32.shape[1], env.RU, 9         # env 8 sits on level 8: row 9 of the padded buffers
    j = env.NSU
    assert int(env._st32[8, j]) == 8

    def run(level_word):
        state = torch.full((N + 2, NS), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        state[1:N + 1] = env._st32
        state[BAD, j] = level_word
        rects = torch.full((N + 2, RU, 4), 0x5A5A, dtype=torch.int16, device=DEV)
        lvo = torch.full((N + 2,), 0xA5, dtype=torch.uint8, device=DEV)
        rw, ep = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        dn = torch.zeros(N, dtype=torch.uint8, device=DEV)
        a = torch.arange(N, dtype=torch.int32, device=DEV)
        for t in range(CAP + 1):                               # across an episode end: the ledger runs too
            rc = hip_lib.launch_meta_step(state[1].data_ptr(), env._level_tab.data_ptr(), a.data_ptr(), None, 0, N, 5,
                                          ID_BASE, 4, CAP, rw.data_ptr(), dn.data_ptr(), ep.data_ptr(),
                                          rects[1].data_ptr(), lvo[1:].data_ptr(), _lib.stream())
            assert rc == 0
            if t == 0:
                first = (state.clone(), rects.clone(), lvo.clone())
        torch.cuda.synchronize()
        for s in (first[0], state):
            assert (s[0] == 0x5A5A5A5A).all() and (s[N + 1] == 0x5A5A5A5A).all()
        for r in (first[1], rects):
            assert (r[0] == 0x5A5A).all() and (r[N + 1] == 0x5A5A).all()
        for v in (first[2], lvo):
            assert v[0] == 0xA5 and v[N + 1] == 0xA5 and (v[1:N + 1] < NL).all()
        return first, (state, rects, lvo)

    (s250, r250, l250), end250 = run(250)
    (s8, r8, l8), end8 = run(8)
    assert int(s250[BAD, j]) == 250 and int(l250[BAD]) == 8    # the word is only read; the scene is level 8's
    s250[BAD, j] = 8
    assert torch.equal(s250, s8) and torch.equal(r250, r8) and torch.equal(l250, l8)
    for x, y in zip(end250, end8):                             # after the episode end the ledger wrote a valid level
        assert torch.equal(x, y)
    assert 0 <= int(end250[0][BAD, j]) < NL


# ------------------------------------------------------------------------------------------- RNG identity
def test_two_halves_with_their_id_base_equal_one_batch(hip_lib):
    H = N_MIX // 2
    cpu = mixed_env(id_base=0, reset=False)
    full = hip_twin(cpu, id_base=0)
    halves = [hip_twin(cpu, n=H, lo=0, id_base=0), hip_twin(cpu, n=H, lo=H, id_base=H)]
    of = full.reset()
    assert torch.equal(of[:H], halves[0].reset()) and torch.equal(of[H:], halves[1].reset())
    acts = mixed_actions().to(DEV)
    ndone = 0
    for t in range(30):
        of, rf, df, inf = full.step(acts[t])
        for k, h in enumerate(halves):
            sl = slice(k * H, (k + 1) * H)
            oh, rh, dh, inh = h.step(acts[t, sl].contiguous())
            assert torch.equal(of[sl], oh) and torch.equal(rf[sl], rh) and torch.equal(df[sl], dh), (t, k)
            assert torch.equal(inf["episode_return"][sl], inh["episode_return"]), (t, k)
            assert torch.equal(full._st32[sl], h._st32), (t, k)
        ndone += int(df.sum())
    assert ndone >= 2 * N_MIX
    wrong = hip_twin(cpu, n=H, lo=H, id_base=0)                # the second half under the first half's indices
    wrong.reset()
    assert not torch.equal(wrong._st32, halves[1]._st32)


# ------------------------------------------------------------------------------------------- engine
def _meta_trainer(graph, ring, seed=1):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.config import preset
    cfg = preset("doom-meta")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 2, 16, 5       # 16 envs per path is the engine's smallest
    cfg.ga.B = 2                                                 # a tournament of the two paths
    cfg.backend = "hip"
    cfg.compute_dtype = "fp32x"
    cfg.frame_ring = ring
    cfg.use_graph = graph
    cfg.deterministic = True
    cfg.seed = cfg.ga.seed = seed
    cfg.gc_freeze = False
    tr = PathNetTrainer(cfg, device="cuda:0")
    assert tr.env.id == "DoomMeta" and tr.env._hip and tr.env.num_actions == 8 and tr.cfg.net.num_actions == 8
    assert tr.engine.ring == ring and tr.engine.use_graph == graph
    tr.env.max_episode_steps = 4                                 # episodes, and level changes, inside every rollout
    return tr


@pytest.mark.parametrize("ring", [False, True])
def test_engine_eager_update_equals_captured_update_and_replay(hip_lib, ring):
    out = []
    for graph in (False, True):
        tr = _meta_trainer(graph, ring)
        for _ in range(4):                                       # with graphs: eager, captured, replayed twice
            tr.update()
        tr.flush()
        torch.cuda.synchronize()
        assert (tr.engine.g_opt is not None) == graph
        flat = tr.model.store.flat.detach().clone()
        assert torch.isfinite(flat).all()
        info = tr.env.meta_info()
        out.append((flat, tr.env._st32.clone(), tr.engine.fitness.clone()))
        tr.env.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert info["scores"].sum() > 0 and bool((info["level"] != 0).any())         # episodes ended, levels changed


def test_engine_checkpoint_resume_reproduces_the_next_update(hip_lib, tmp_path):
    from pathnet_gym_amd.utils import checkpoint
    tr = _meta_trainer(True, True)
    for _ in range(2):
        tr.update()
    tr.flush()
    path = checkpoint.save(tr, str(tmp_path / "ck.safetensors"))
    saved = tr.env._st32.clone()
    tr.update()
    tr.flush()
    torch.cuda.synchronize()
    tr2 = _meta_trainer(True, True)
    checkpoint.load(tr2, path)
    assert torch.equal(tr2.env._st32, saved)
    assert torch.equal(tr2.env.level, saved[:, tr2.env.NSU].long())
    tr2.update()
    tr2.flush()
    torch.cuda.synchronize()
    assert torch.equal(tr2.model.store.flat, tr.model.store.flat)
    assert torch.equal(tr2.env._st32, tr.env._st32)
    assert not torch.equal(tr.env._st32, saved)


# ------------------------------------------------------------------------------------------- evaluator
def test_evaluator_captured_equals_eager_and_reports_the_meta_total(hip_lib):
    from pathnet_gym_amd.config import preset
    from pathnet_gym_amd.runtime.evaluator import HipEvaluator, unsupported_reason
    from test_hip_evaluator import masks, same, snapshot
    net = preset("doom-meta").net
    P, E, T = 2, 16, 5
    assert unsupported_reason(net, "SynthDoomMeta-v0", "fp32x", E) is None

    def make(use_graph):
        ev = HipEvaluator(net, "SynthDoomMeta-v0", P, E, chunk=T, device=DEV, compute_dtype="fp32x", env_seed=3,
                          use_graph=use_graph, frame_ring=True)
        ev.env.max_episode_steps = CAP
        ev.load(ev.model.store.flat.detach().clone(), masks(P, net, 0), 0)
        return ev

    kw = dict(quota=4, max_steps=200, sample=True, seed=11)
    g, e = make(True), make(False)
    try:
        a = snapshot(g, **kw)
        assert g._graphs is not None
        b = snapshot(e, **kw)
        assert same(a, b) and same(a, snapshot(g, **kw))
        assert a[1].min() >= 4
        # the same episodes on a HIP env of its own, driven by the recorded actions: the returns the ledger holds
        # are float32(total5) * 0.2f of the state at those episode ends
        rec = []
        rets = e.run(record=rec, **kw)
        twin = registry.make("SynthDoomMeta-v0", num_envs=P * E, device=DEV, seed=3, backend="hip")
        twin.max_episode_steps = CAP
        twin.reset()
        want = [[] for _ in range(P * E)]
        for chunk in rec:
            for t in range(T):
                _, _, d, info = twin.step(chunk["actions"][t])
                assert torch.equal(d, chunk["dones"][t].bool()) and torch.equal(info["episode_return"], chunk["epret"][t])
                total5 = twin._st32[:, twin.NSU + 3].cpu().numpy()
                for b in d.nonzero().flatten().tolist():
                    want[b].append(float(np.float32(total5[b]) * np.float32(0.2)))
        for b in range(P * E):
            assert rets[b] == want[b][:4], b
        assert max(max(r) for r in rets) >= 200.0                # a Basic episode under the cap scores 1000: 200 points
    finally:
        g.close()
        e.close()
