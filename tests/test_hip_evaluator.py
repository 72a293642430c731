"""The forward-only HIP engine (runtime/evaluator.py) on an MI355X: captured = eager = repeat, the policy it plays,
the ledger's wiring, the LSTM state across episode ends and chunk boundaries, path selection, the weights' copy, the
statistical agreement of ``evaluate_path(backend="hip")`` with today's torch evaluator, and the refusals.

Shapes: the conv kernels of every precision take envs per path in multiples of 16 on the reference pixel trunk
(E * Ho * Wo must be a multiple of 16; its first layer has 39 x 29 outputs), so the pixel configs run 2 paths x 16
envs; the vector net runs 4 paths x 2 envs.
"""
import numpy as np
import pytest
import torch

from pathnet_gym_amd.algo.ga import get_geopath
from pathnet_gym_amd.config import preset

pytestmark = pytest.mark.gpu
DEV = "cuda"

# forward-vs-oracle budgets of the stand-alone engine tests, per compute_dtype: relative L2 error of logits and of
# values against the fp32 torch oracle on the engine's own observations
#   fp32x: tests/test_x3_engine.py _oracle_grad          (rel < 1e-5)
#   fp32:  tests/test_f32_engine.py _oracle_grad          (rel < 1e-4)
#   bf16:  tests/test_hip_kernels.py test_engine_gradient_matches_oracle, budget.check(test + "_fwd", ..., 3e-2),
#          against the oracle that rounds weights and layer outputs to bf16 (trunk_forward_ref(emulate_bf16=True))
#   fp32 LSTM net: tests/test_f32_lstm_engine.py docstring ("forward logits and values agree with the oracle to 1e-5")
FWD_BUDGET = {"fp32x": 1e-5, "fp32": 1e-4, "bf16": 3e-2}
LSTM_F32_BUDGET = 1e-5


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-12))


def masks(P, net, seed=0):
    rng = np.random.RandomState(seed)
    return np.stack([get_geopath(net.L, net.M, net.N, rng) for _ in range(P)]).astype(np.float32)


CONFIGS = {
    # name: (preset, env, P, E, T, compute_dtype, frame_ring, episode cap in agent steps or None)
    "cartpole-bf16": ("cartpole", "CartPole-v1", 4, 2, 5, "bf16", False, None),
    "cartpole-fp32": ("cartpole", "CartPole-v1", 4, 2, 5, "fp32", False, None),
    "doom-basic-bf16-packed": ("doom-basic", "DoomBasic", 2, 16, 5, "bf16", False, None),
    "doom-basic-fp32-packed": ("doom-basic", "DoomBasic", 2, 16, 5, "fp32", False, None),
    "doom-basic-fp32x-ring": ("doom-basic", "DoomBasic", 2, 16, 5, "fp32x", True, None),
    # Pong keeps its kernel state in buffers of its own (made by the first step unless the evaluator makes them before
    # its snapshot): the repeat must restore them
    "pong-bf16-packed": ("pong", "Pong", 2, 16, 5, "bf16", False, 7),
    "pong-fp32x-ring": ("pong", "Pong", 2, 16, 5, "fp32x", True, 7),
    # tests/test_f32_lstm_engine.py reference_cfg: the reference preset (L=4 trunk + LSTM 256), 3 paths x 16 envs,
    # T = 4, short episodes
    "lstm-fp32": ("reference", "Alien", 3, 16, 4, "fp32", False, 5),
}


def make_evaluator(name, use_graph=True, nvalid=None, mask_seed=0):
    from pathnet_gym_amd.runtime.evaluator import HipEvaluator
    pre, env_id, P, E, T, dtype, ring, cap = CONFIGS[name]
    net = preset(pre).net
    ev = HipEvaluator(net, env_id, P, E, chunk=T, device=DEV, compute_dtype=dtype, env_seed=3, nvalid=nvalid,
                      use_graph=use_graph, frame_ring=ring)
    if cap is not None:
        ev.env.max_episode_steps = cap          # read at every launch / at capture
    assert ev.engine.ring == ring and ev.compute_dtype == dtype
    ev.load(ev.model.store.flat.detach().clone(), masks(P, net, mask_seed), 0)
    return ev


def snapshot(ev, **kw):
    out = ev.run(**kw)
    last = ev.last
    # ... and the last chunk's actions: with episodes cut by a step cap (Pong) the ledger alone cannot tell two
    # sampling seeds apart
    return (out, last["cnt"].copy(), last["ret"].copy(), last["endstep"].copy(), last["steps"],
            ev.engine.actions[:ev.T].cpu().numpy())


def same(a, b):
    return (a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
            and np.array_equal(a[3], b[3]) and a[4] == b[4] and np.array_equal(a[5], b[5]))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_captured_equals_eager_equals_repeat(hip_lib, name):
    kw = dict(quota=2, max_steps=120, sample=True, seed=11)
    g = make_evaluator(name, use_graph=True)
    e = make_evaluator(name, use_graph=False)
    try:
        assert g.use_graph and not e.use_graph
        a = snapshot(g, **kw)
        assert g._graphs is not None and len(g._graphs) == (2 if g.engine._parities else 1)
        graphs = list(g._graphs)
        b = snapshot(e, **kw)
        assert a[1].max() >= 1, "no episode finished: the comparison would be empty"
        assert same(a, b), (a[1], b[1])
        a2 = snapshot(g, **kw)
        assert all(x is y for x, y in zip(graphs, g._graphs)), "recaptured"
        assert same(a, a2) and same(b, snapshot(e, **kw))
        other = snapshot(g, **dict(kw, seed=12))
        assert all(x is y for x, y in zip(graphs, g._graphs)), "a new seed must not recapture"
        assert not same(a, other)
        # check_every only changes when the host looks: the ledger's records are the same
        a3 = snapshot(g, **dict(kw, check_every=3))
        assert a3[0] == a[0] and a3[4] >= a[4]          # (it may play further chunks before it looks)
    finally:
        g.close()
        e.close()


POLICY_CONFIG = {"fp32x": "doom-basic-fp32x-ring", "fp32": "doom-basic-fp32-packed", "bf16": "doom-basic-bf16-packed"}


@pytest.mark.parametrize("dtype", ["fp32x", "fp32", "bf16"])
@pytest.mark.parametrize("sample", [False, True])
def test_the_policy_is_the_oracles_and_the_actions_follow_its_own_logits(hip_lib, dtype, sample):
    """Eager record mode on the pixel config, 20 steps: on the recorded observation stacks the torch oracle's logits
    and values agree with the evaluator's within the stand-alone forward tests' budget for the precision (bf16, the
    evaluator's default: packed stacks, unfused heads, against the bf16-emulating oracle as that test does); greedy
    actions are the argmax of the evaluator's own logits; sampled actions are the torch mirror of the counter-hash
    Gumbel draw on those logits with the same key, outside near-ties (tests/test_heads_kernels.py: top-two gap of the
    perturbed logits below 8 e32; at most 0.2 % of the rows may be near-ties)."""
    import test_heads_kernels as thk
    from pathnet_gym_amd.algo.a2c_math import sample_actions_keyed
    from pathnet_gym_amd.models.pathnet import heads_ref, trunk_forward_ref
    pre, env_id, P, E, T, cdt, ring, _ = CONFIGS[POLICY_CONFIG[dtype]]
    assert cdt == dtype
    from pathnet_gym_amd.runtime.evaluator import HipEvaluator
    net = preset(pre).net
    ev = HipEvaluator(net, env_id, P, E, chunk=T, device=DEV, compute_dtype=dtype, env_seed=3, use_graph=False,
                      frame_ring=ring)
    try:
        ev.load(ev.model.store.flat.detach().clone(), masks(P, net), 0)
        rec = []
        ev.run(quota=10 ** 6, max_steps=20, sample=sample, seed=4, record=rec)
        assert len(rec) == 4 and ev.last["steps"] == 20
        B = P * E
        obs = torch.cat([r["obs"] for r in rec]).reshape(20 * B, 160, 120, 4)
        logits = torch.cat([r["logits"] for r in rec]).reshape(20 * B, -1)
        values = torch.cat([r["values"] for r in rec]).reshape(-1)
        actions = torch.cat([r["actions"] for r in rec]).reshape(20, B)
        assert len({bytes(o.cpu().numpy().tobytes()) for o in obs[::B]}) > 1, "the observations never changed"
        with torch.no_grad():
            mask = ev.model.mask.repeat_interleave(E, 0).repeat(20, 1, 1)
            feat = trunk_forward_ref(ev.model.store, obs.float() / 255.0, mask, emulate_bf16=dtype == "bf16")
            lr_, vr_ = heads_ref(ev.model.store, feat)
        el, evl = rel(logits, lr_), rel(values, vr_)
        print(f"{dtype}: logits rel {el:.3g}, values rel {evl:.3g} (budget {FWD_BUDGET[dtype]:g})")
        assert el < FWD_BUDGET[dtype] and evl < FWD_BUDGET[dtype], (el, evl)
        if not sample:
            assert torch.equal(actions.long(), logits.argmax(-1).reshape(20, B))
            return
        near_rows = dis_rows = 0
        for s in range(20):
            k, t = divmod(s, T)
            key = ev.stepkey(rec[k]["ctr"], t)
            lg = logits[s * B:(s + 1) * B]
            mirror = sample_actions_keyed(lg, ev.engine.seed, key, 0)
            _, _, gap, e32 = thk.gumbel_reference(lg.cpu().float(), ev.engine.seed, key, 0)
            near = gap < 8.0 * e32
            dis = (actions[s].long() != mirror).cpu()
            assert not bool((dis & ~near).any()), (s, int(dis.sum()))
            near_rows += int(near.sum())
            dis_rows += int(dis.sum())
        print(f"{dtype}: {near_rows} near-tie rows of {20 * B}, {dis_rows} disagreeing")
        assert near_rows <= 0.002 * 20 * B
        assert len(set(actions.reshape(-1).tolist())) > 1
    finally:
        ev.close()


@pytest.mark.parametrize("name", ["cartpole-fp32", "doom-basic-bf16-packed"])
def test_the_returned_lists_are_the_ledger_over_the_recorded_rollout(hip_lib, name):
    from pathnet_gym_amd.algo.evaluate import ledger_ref
    B = CONFIGS[name][2] * CONFIGS[name][3]
    nvalid, quota, max_steps = B - 3, 2, 93          # max_steps cuts inside a chunk (T = 5)
    ev = make_evaluator(name, use_graph=False, nvalid=nvalid)
    try:
        rec = []
        out = ev.run(quota=quota, max_steps=max_steps, sample=True, seed=2, record=rec)
        cnt = np.zeros(B, np.int32)
        ret = np.zeros((B, quota), np.float32)
        end = np.zeros((B, quota), np.int32)
        clock = 0
        for r in rec:
            clock, pending = ledger_ref(r["dones"].cpu().numpy(), r["epret"].cpu().numpy(), nvalid, quota, max_steps,
                                        cnt, ret, end, clock)
        assert clock == ev.last["steps"] and len(out) == nvalid and cnt.max() >= 1
        assert out == [[float(x) for x in ret[b, :cnt[b]]] for b in range(nvalid)]
        assert np.array_equal(ev.last["cnt"], cnt[:nvalid]) and np.array_equal(ev.last["endstep"], end[:nvalid])
        assert int(ev.pending.item()) == pending
        assert not ev.cnt[nvalid:].any()          # the padding envs are never accounted
    finally:
        ev.close()


def test_lstm_state_entering_the_step_after_a_done_is_zero(hip_lib):
    """Reference LSTM net in fp32, T = 4, episodes capped at 3 agent steps: episodes end at steps 2, 5, 8, 11, ..., i.e.
    inside chunks and, at step 11, on a chunk's last step (T - 1).  The state carried into the next chunk's step 0 is
    then exactly zero, and at every step the cell's output is the oracle cell's on the recorded features from a zero
    state after a done, from the recorded previous state otherwise."""
    from pathnet_gym_amd.models.pathnet import lstm_cell_ref
    ev = make_evaluator("lstm-fp32", use_graph=False)
    ev.env.max_episode_steps = 3
    try:
        T = ev.T
        rec = []
        ev.run(quota=10 ** 6, max_steps=16, sample=True, seed=1, record=rec)
        assert len(rec) == 4
        k, b = ev.model.store.lstm()
        dones = torch.cat([r["dones"] for r in rec]).bool()          # [16, B]
        assert bool(dones[T - 1::T].any()), "no episode ended on a chunk's last step"
        assert bool(dones.reshape(4, T, -1)[:, :T - 1].any()), "no episode ended inside a chunk"
        checked_done = checked_boundary = carried = 0
        for s in range(16):
            c, t = divmod(s, T)
            r = rec[c]
            h_in, c_in = r["h"][t], r["c"][t]
            after_done = dones[s - 1] if s > 0 else torch.zeros_like(dones[0])
            if t == 0 and s > 0:
                # slot 0 is written by the carry: zero where the previous chunk's last step ended an episode, the
                # previous chunk's last state everywhere else
                if bool(after_done.any()):
                    assert float(h_in[after_done].abs().max()) == 0.0 and float(c_in[after_done].abs().max()) == 0.0
                    checked_boundary += int(after_done.sum())
                live = ~after_done
                if bool(live.any()):
                    assert torch.equal(h_in[live], rec[c - 1]["h"][T][live]) and float(h_in[live].abs().max()) > 0.0
                    carried += int(live.sum())
            keep = (~after_done).float()[:, None]
            with torch.no_grad():
                h_ref, c_ref = lstm_cell_ref(r["feat"][t], h_in * keep, c_in * keep, k, b)
                h_bad, _ = lstm_cell_ref(r["feat"][t], h_in, c_in, k, b)
            assert rel(r["h"][t + 1], h_ref) < LSTM_F32_BUDGET and rel(r["c"][t + 1], c_ref) < LSTM_F32_BUDGET, s
            if t > 0 and bool(after_done.any()):
                # the check discriminates: carrying the state over the episode end gives another output
                assert rel(r["h"][t + 1][after_done], h_bad[after_done]) > 100 * LSTM_F32_BUDGET, s
                checked_done += int(after_done.sum())
        assert checked_done > 0 and checked_boundary > 0 and carried > 0
    finally:
        ev.close()


def test_path_selection_and_all_ones_path(hip_lib):
    ev = make_evaluator("cartpole-fp32")
    try:
        net = ev.model.cfg
        flat = ev.model.store.flat.detach().clone()
        kw = dict(quota=3, max_steps=2000, sample=False)
        a = ev.run(**kw)
        ev.load(flat, masks(ev.P, net, seed=7), 0)
        b = ev.run(**kw)
        assert a != b, "two different sets of expressed paths played the same episodes"
        ev.load(flat, masks(ev.P, net, seed=0), 0)
        assert ev.run(**kw) == a
        one = masks(1, net, seed=5)[0]
        ev.load(flat, one, 0)          # one [L, M] path for every row
        c = ev.run(**kw)
        assert all(len(x) == 3 for x in c)
        ev.load(flat, np.ones((net.L, net.M), np.float32), 0)
        d = ev.run(**kw)
        assert all(len(x) == 3 for x in d) and d != c
    finally:
        ev.close()


def test_the_weights_are_a_copy(hip_lib):
    ev = make_evaluator("cartpole-bf16")
    try:
        flat = (ev.model.store.flat.detach().clone() * 1.5).requires_grad_(True)
        before = flat.detach().clone()
        ev.load(flat, masks(ev.P, ev.model.cfg), 0)
        ev.run(quota=1, max_steps=600, sample=True, seed=3)
        assert torch.equal(flat.detach(), before) and flat.grad is None and flat.requires_grad
        assert ev.model.store.flat.data_ptr() != flat.data_ptr() and torch.equal(ev.model.store.flat, before)
        assert not ev.model.store.flat.requires_grad
        eng = ev.engine
        assert not hasattr(eng, "grad_flat") and eng.grads == [] and not hasattr(eng, "blk_seg")
    finally:
        ev.close()
    assert ev.engine is None and ev.model is None and ev.ret is None


def test_evaluate_path_hip_agrees_with_the_torch_evaluator_statistically(hip_lib):
    """CartPole, one randomly initialised path, 256 episodes, both sampled: the means differ by at most 5 standard
    errors of the difference, from the two samples' own variances (the heads tests' 5-sigma rule)."""
    from pathnet_gym_amd.algo.evaluate import evaluate_path
    from pathnet_gym_amd.models.pathnet import ParamStore
    net = preset("cartpole").net
    flat = ParamStore(net, DEV, seed=9).flat.detach()
    path = masks(1, net, seed=4)[0]
    kw = dict(episodes=256, seed=77, device=DEV, max_steps=2000)
    th = evaluate_path(net, flat, path, "CartPole-v1", backend="torch", **kw)
    hp = evaluate_path(net, flat, path, "CartPole-v1", backend="hip", compute_dtype="fp32", **kw)
    assert th["finished"] == 256 and hp["finished"] == 256
    assert th["backend"] == "torch" and hp["backend"] == "hip" and hp["compute_dtype"] == "fp32"
    assert 0 < hp["last_finish_step"] <= hp["steps"] <= 2000
    a, b = np.asarray(th["returns"]), np.asarray(hp["returns"])
    se = float(np.sqrt(a.var(ddof=1) / a.size + b.var(ddof=1) / b.size))
    print(f"torch mean {a.mean():.3f}, hip mean {b.mean():.3f}, se of the difference {se:.3f}")
    assert se > 0 and abs(a.mean() - b.mean()) <= 5.0 * se
    again = evaluate_path(net, flat, path, "CartPole-v1", backend="hip", compute_dtype="fp32", **kw)
    assert again["returns"] == hp["returns"]


def test_evaluate_model_hip_counts_the_first_episodes_of_every_path(hip_lib):
    from pathnet_gym_amd.algo.evaluate import evaluate_model
    from pathnet_gym_amd.models.acnet import ACPathNet
    net = preset("cartpole").net
    model = ACPathNet(net, 5, "cpu", "torch", seed=2)
    model.set_paths(masks(5, net, seed=1))
    info = {}
    rets = evaluate_model(model, "CartPole-v1", episodes=3, max_steps=2000, backend="hip", info=info)
    assert len(rets) == 5 and all(np.isfinite(rets)) and info["backend"] == "hip" and info["steps"] % 20 == 0
    short = evaluate_model(model, "CartPole-v1", episodes=3, max_steps=5, backend="hip")
    assert len(short) == 5 and all(np.isnan(short))          # no episode of CartPole ends within 5 steps


def test_evaluate_model_hip_on_a_conv_net_reads_one_env_per_path(hip_lib):
    """The conv kernels take 16 envs per path: the row is padded, and ``episodes`` still means the first episodes of
    ONE env per path -- env p * 16 of a direct evaluator run with the same seeds."""
    from pathnet_gym_amd.algo.evaluate import HIP_CHUNK, evaluate_model
    from pathnet_gym_amd.models.acnet import ACPathNet
    from pathnet_gym_amd.runtime.evaluator import HipEvaluator, min_envs_per_path
    net = preset("doom-basic").net
    P, E = 3, min_envs_per_path(net)
    assert E == 16
    model = ACPathNet(net, P, "cpu", "torch", seed=2)
    model.set_paths(masks(P, net, seed=1))
    info = {}
    kw = dict(episodes=2, max_steps=400, seed=21, sample=True)
    rets = evaluate_model(model, "DoomBasic", backend="hip", compute_dtype="bf16", info=info, **kw)
    assert len(rets) == P and all(np.isfinite(rets)) and info["backend"] == "hip" and info["compute_dtype"] == "bf16"
    ev = HipEvaluator(net, "DoomBasic", P, E, chunk=HIP_CHUNK, device=DEV, compute_dtype="bf16", env_seed=21)
    try:
        ev.load(model.store.flat, model.mask.numpy(), 0)
        every = ev.run(quota=2, max_steps=400, sample=True, seed=21)
        steps_all = ev.last["steps"]
        assert len(every) == P * E
        assert rets == [float(np.mean(every[p * E])) for p in range(P)]
        one = ev.run(quota=2, max_steps=400, sample=True, seed=21, env_stride=E)
        assert one == [every[p * E] for p in range(P)] and all(len(x) == 2 for x in one)
        assert ev.last["steps"] == info["steps"] <= steps_all          # it waits for the wanted envs only
    finally:
        ev.close()


def test_refusals_name_the_reason_and_auto_falls_back(hip_lib):
    from pathnet_gym_amd.algo.evaluate import evaluate_path, resolve_eval_backend
    from pathnet_gym_amd.models.pathnet import ParamStore
    from pathnet_gym_amd.runtime.evaluator import HipEvaluator
    cart = preset("cartpole").net
    flat = ParamStore(cart, DEV, seed=1).flat.detach()
    path = masks(1, cart)[0]
    # a host-stepped Gym env
    with pytest.raises(NotImplementedError, match="host"):
        evaluate_path(cart, flat, path, "PyCartPole-v1", episodes=4, device=DEV, max_steps=50, backend="hip")
    r = evaluate_path(cart, flat, path, "PyCartPole-v1", episodes=4, device=DEV, max_steps=50, backend="auto")
    assert r["backend"] == "torch"
    assert evaluate_path(cart, flat, path, "CartPole-v1", episodes=4, device=DEV, max_steps=50,
                         backend="auto")["backend"] == "hip"
    # the hybrid LSTM: widths that are no multiples of 64
    hyb = preset("reference").net
    hyb.lstm_size = 100
    with pytest.raises(NotImplementedError, match="hybrid"):
        HipEvaluator(hyb, "Alien", 1, 16, chunk=4, device=DEV, compute_dtype="fp32")
    assert resolve_eval_backend("auto", hyb, "Alien") == "torch"
    hflat = ParamStore(hyb, DEV, seed=1).flat.detach()
    r = evaluate_path(hyb, hflat, masks(1, hyb)[0], "Alien", episodes=2, device=DEV, max_steps=3, backend="auto")
    assert r["backend"] == "torch" and r["steps"] == 3
    # envs per path the conv kernels do not take
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        HipEvaluator(preset("pong").net, "Pong", 2, 4, device=DEV)
