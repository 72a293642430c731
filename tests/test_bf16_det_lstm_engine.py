"""The `reference` preset (L=4 trunk + BasicLSTMCell(256), 18 actions) in the bf16 engine with deterministic=True: the
fused bf16 cell of csrc/lstm.hip with the ordered weight gradient (launch_lstm_wgrad_ord) inside the rollout hipGraph,
instead of the autograd hybrid, on an MI355X.

Pong, 3 paths x 16 envs (4 in the reproducibility run), T = 4 or 5, episodes of 3 to 7 steps so that they end inside
the rollouts, device GA, no frame ring.  The oracle is tests/test_hip_kernels.py's (``lstm_dones_rollout``): the
bf16-emulating trunk, ``lstm_cell_ref`` with keep from ``eng.dones`` and ``a2c_loss``; the per-layer budget is the 8e-2
the project applies to this network in bf16 (``engine_lstm_dones``), asserted directly.  The weight gradient's wiring
is checked against float64 with the derived bound of tests/test_lstm_ord_kernels.py at g0 = 0.
"""
import pytest
import torch

from pathnet_gym_amd.algo.a2c_math import a2c_loss, nstep_returns
from pathnet_gym_amd.config import preset
from pathnet_gym_amd.models.pathnet import heads_ref, trunk_forward_ref
from test_hip_kernels import grad_errors
from test_lstm_kernels import ref_wgrad, within
from test_lstm_ord_kernels import ONE_ADD

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYER_BUDGET = 8e-2


def det_cfg(paths=3, envs=16, tmax=5, graph=True):
    cfg = preset("reference")
    cfg.tasks = ["Pong"]
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = paths, envs, tmax
    cfg.compute_dtype = "bf16"
    cfg.deterministic = True
    cfg.frame_ring = False
    cfg.use_graph = graph
    cfg.ga.backend = "device"
    return cfg


def is_routed(tr, graph=True):
    eng = tr.engine
    return bool(eng.lstm_hip and not eng.hybrid and eng.use_graph == graph and tr.model.hip.deterministic
                and not tr.model.hip.f32 and tr.model.hip.lstm["ord"] and eng.hst.dtype == torch.bfloat16
                and eng.grads[-1].dtype == torch.float32)


@pytest.fixture(scope="module", params=["eager", "graph"])
def det_lstm_rollout(hip_lib, request):
    """T = 5, episodes capped at 3 agent steps (coprime to T: ends at interior steps and at the last one), the
    per-env step counters offset by env % 3 so the rows end at different steps.  "graph": hipGraph capture + replays,
    the last replay is the one compared.  -> the engine's gradient, the oracle's, and the oracle with keep forced
    to 1."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.envs.pong import STEPS
    from pathnet_gym_amd.models.pathnet import ParamStore, bf16_ste, lstm_cell_ref
    from pathnet_gym_amd.ops import envs as henv
    graph = request.param == "graph"
    cfg = det_cfg(graph=graph)
    tr = PathNetTrainer(cfg, device=DEV)
    eng, env = tr.engine, tr.env
    assert is_routed(tr, graph)
    env.max_episode_steps = 3
    if not hasattr(env, "_st32"):
        henv.pong_sync_to_device(env)
    env._st32[:, STEPS] += (torch.arange(eng.B, device=DEV) % 3).to(torch.int32)     # in place: the graphs keep it
    for _ in range(3 if graph else 2):
        tr.update()
    tr.flush()
    torch.cuda.synchronize()
    assert not graph or eng.g_rollout is not None
    T, E, B = eng.T, eng.E, eng.B
    h0, c0 = eng.hst[0].float().clone(), eng.cst[0].clone()
    eng.rollout_backward()
    torch.cuda.synchronize()
    dones = eng.dones.bool()
    assert dones[:T - 1].any() and dones[T - 1].any()
    a2c = cfg.a2c
    flat = tr.model.store.flat.detach().clone().requires_grad_(True)
    st = ParamStore(cfg.net, DEV, flat=flat)
    k, bb = st.lstm()
    kq = bf16_ste(k)
    x = eng.obs_stacks().reshape((T + 1) * B, 160, 120, 4).float() / 255.0
    mask = tr.model.mask.repeat_interleave(E, 0).repeat(T + 1, 1, 1)
    feat = trunk_forward_ref(st, x, mask, emulate_bf16=True).view(T + 1, B, -1)
    R, adv = nstep_returns(eng.rewards, eng.values[:T], dones, eng.values[T], a2c.gamma, a2c.gae_lambda,
                           a2c.reward_clip)

    def oracle(keep_of):
        h, c = h0, c0
        hs = []
        for t in range(T + 1):
            if t > 0:
                keep = keep_of(t)[:, None]
                h, c = h * keep, c * keep
            h, c = lstm_cell_ref(bf16_ste(feat[t]), bf16_ste(h), c, kq, bb)
            hs.append(h)
        logits, values = heads_ref(st, bf16_ste(torch.stack(hs)).reshape((T + 1) * B, -1))
        loss, _, _, _ = a2c_loss(logits[:T * B], values[:T * B], eng.actions[:T].reshape(-1).long(), R.reshape(-1),
                                 adv.reshape(-1), a2c.entropy_beta, a2c.value_coef,
                                 torch.full((T * B,), eng.weight, device=DEV))
        return torch.autograd.grad(loss, flat, retain_graph=True)[0]

    kf = 1.0 - eng.dones.float()
    return dict(mode=request.param, tr=tr, eng=eng, g_hip=eng.grad_flat.clone(), g_ref=oracle(lambda t: kf[t - 1]),
                g_keep1=oracle(lambda t: torch.ones_like(kf[0])))


def test_bf16_det_lstm_runs_the_fused_cell_in_the_rollout_graph(hip_lib):
    """deterministic=True on the LSTM preset keeps the captured HIP engine: no hybrid, no eager fallback."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    tr = PathNetTrainer(det_cfg(tmax=4), device=DEV)
    eng = tr.engine
    assert (eng.lstm_hip and not eng.hybrid and eng.use_graph and tr.model.hip.deterministic
            and eng.hst.dtype == torch.bfloat16)
    assert is_routed(tr) and tr.model.hip.lstm["part"] is not None        # the slabs exist before any capture
    tr.env.max_episode_steps = 5
    for _ in range(3):
        tr.update()
    tr.flush()
    torch.cuda.synchronize()
    assert eng.g_rollout is not None
    assert bool(torch.isfinite(tr.model.store.flat).all()) and bool(torch.isfinite(eng.hst.float()).all())


def test_bf16_det_lstm_weight_gradient_is_the_float64_product_of_the_saved_rows(det_lstm_rollout):
    """grad_flat's lstm.kernel / lstm.bias segments == xh^T bf(dz) / sum dz in float64 of the rows the engine saved,
    inside the derived bound (grad_flat starts at zero: g0 = 0); either segment scaled by 2 % is outside."""
    r = det_lstm_rollout
    tr, eng = r["tr"], r["eng"]
    T, B = eng.T, eng.B
    ls = tr.model.hip.lstm
    KK, G4 = ls["F"] + ls["H"], 4 * ls["H"]
    xh, dz = eng.xh.reshape(T * B, KK).cpu(), eng.dz.reshape(T * B, G4).cpu()
    assert xh.dtype == torch.bfloat16 and float(dz.abs().sum()) > 0
    dK, bK, db, bb = ref_wgrad(xh, dz)
    tolK = bK + ONE_ADD * (xh.double().abs().t() @ dz.to(torch.bfloat16).double().abs())
    tolb = bb + ONE_ADD * dz.double().abs().sum(0)
    by = tr.model.store.layout.by_name
    sk, sb = by["lstm.kernel"], by["lstm.bias"]
    assert (sk.offset, sb.offset) == (ls["k_off"], ls["b_off"])
    gK = r["g_hip"][sk.offset:sk.offset + sk.numel].view(KK, G4).cpu()
    gb = r["g_hip"][sb.offset:sb.offset + sb.numel].cpu()
    within(f"engine lstm.kernel ({r['mode']})", gK, dK, tolK)
    within(f"engine lstm.bias ({r['mode']})", gb, db, tolb)
    with pytest.raises(AssertionError):
        within("lstm.kernel x 1.02", gK * 1.02, dK, tolK)
    with pytest.raises(AssertionError):
        within("lstm.bias x 1.02", gb * 1.02, db, tolb)


def test_bf16_det_lstm_gradient_matches_the_bf16_oracle_with_episode_ends(det_lstm_rollout):
    """Every layer of the whole gradient within the bf16 budget of this network; the oracle that ignores the episode
    ends leaves it on the lstm layer."""
    r = det_lstm_rollout
    errs = grad_errors(r["tr"], r["g_hip"], r["g_ref"])
    print(r["mode"], {k_: round(v, 4) for k_, v in sorted(errs.items(), key=lambda kv: -kv[1])[:8]})
    assert "lstm" in errs
    for name, v in errs.items():
        assert v < LAYER_BUDGET, (name, v)
    wrong = grad_errors(r["tr"], r["g_keep1"], r["g_ref"])["lstm"]
    print("lstm error of the keep = 1 oracle:", wrong, "of the engine:", errs["lstm"])
    assert wrong > LAYER_BUDGET


def test_bf16_det_lstm_updates_are_bit_reproducible(hip_lib):
    """Two trainers from one seed: 4 graph-replayed updates with episode ends give the same bits in the weights, the
    gradient and the carried recurrent state (ordered sums everywhere, the LSTM weight gradient included)."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer

    def run():
        cfg = det_cfg(paths=4, envs=16, tmax=5, graph=True)
        cfg.ga.concurrent_tournaments = 1
        tr = PathNetTrainer(cfg, device=DEV)
        eng = tr.engine
        assert is_routed(tr)
        tr.env.max_episode_steps = 7
        for _ in range(4):
            tr.update()
        tr.flush()
        torch.cuda.synchronize()
        assert eng.g_rollout is not None          # 20 steps of 7-step episodes: ends inside updates 2 and 3
        return (tr.model.store.flat.detach().clone(), eng.grad_flat.clone(), eng.hst[0].clone(), eng.cst[0].clone())

    a, b = run(), run()
    assert float(a[2].float().abs().sum()) > 0 and float(a[1].abs().sum()) > 0
    for name, x, y in zip(("weights", "grad_flat", "hst[0]", "cst[0]"), a, b):
        assert torch.equal(x, y), (name, float((x.float() - y.float()).abs().max()))


def test_bf16_det_lstm_checkpoint_round_trip_gives_a_bit_equal_update(hip_lib, tmp_path):
    """State saved after 2 updates and loaded into a fresh trainer: the third update has the same bits."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.utils import checkpoint

    def make():
        tr = PathNetTrainer(det_cfg(tmax=4, graph=False), device=DEV)
        assert is_routed(tr, graph=False)
        tr.env.max_episode_steps = 5
        return tr

    tr = make()
    for _ in range(2):
        tr.update()
    tr.flush()
    h, c = (t.clone() for t in tr.engine.lstm_state_tensors())
    assert float(h.abs().sum()) > 0
    path = checkpoint.save(tr, str(tmp_path / "ck.safetensors"))
    tr.update()
    tr.flush()
    torch.cuda.synchronize()
    tr2 = make()
    checkpoint.load(tr2, path)
    h2, c2 = tr2.engine.lstm_state_tensors()
    assert torch.equal(h2, h) and torch.equal(c2, c)
    tr2.update()
    tr2.flush()
    torch.cuda.synchronize()
    assert torch.equal(tr2.model.store.flat, tr.model.store.flat)
    assert torch.equal(tr2.engine.grad_flat, tr.engine.grad_flat)
    assert torch.equal(tr2.engine.hst[0], tr.engine.hst[0]) and torch.equal(tr2.engine.cst[0], tr.engine.cst[0])


def test_bf16_det_lstm_switch_keeps_the_hybrid_path(hip_lib, monkeypatch):
    """PATHNET_BF16_DET_LSTM=0 (A/B runs): no fused cell, the autograd hybrid, eagerly."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    monkeypatch.setenv("PATHNET_BF16_DET_LSTM", "0")
    tr = PathNetTrainer(det_cfg(tmax=4, graph=True), device=DEV)
    eng = tr.engine
    assert tr.model.hip.lstm is None and eng.hybrid and not eng.lstm_hip and not eng.use_graph
    tr.env.max_episode_steps = 5
    tr.update()
    tr.flush()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.model.store.flat).all())
