"""The reference's default network (L=4 trunk + BasicLSTMCell(256), 18 actions) in the fp32 engine: the fused
fixed-order cell of csrc/lstm_f32.hip instead of the autograd hybrid, on an MI355X.

The gradient checks use the float64 truth and the plain fp32 autograd oracle of tests/test_x3_engine.py
(``_oracle_grad_lstm`` / ``check_layers``) and the project's rule for this network: per layer, the error against
float64 is below max(2e-5, 1.25 x the plain fp32 oracle's own error against float64); forward logits and values
agree with the oracle to 1e-5 (asserted inside ``_oracle_grad_lstm``).  The per-layer values are printed and, with
``PATHNET_RECORD_LSTM_F32=<file>``, recorded (tests/data/lstm_f32_measured.json).
"""
import json
import os

import pytest
import torch

from pathnet_gym_amd.config import LayerSpec, preset
from test_x3_engine import X3_LAYER_TOL, _oracle_grad_lstm, _oracles, check_layers, layer_errors, masks_with_edges

pytestmark = pytest.mark.gpu
DEV = "cuda"


def reference_cfg(paths=3, envs=16, tmax=4, graph=False, dtype="fp32"):
    cfg = preset("reference")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = paths, envs, tmax
    cfg.compute_dtype = dtype
    cfg.frame_ring = False
    cfg.use_graph = graph
    cfg.ga.backend = "device"
    return cfg


def record_layers(label, errs):
    rec = os.environ.get("PATHNET_RECORD_LSTM_F32")
    if not rec:
        return
    d = {}
    if os.path.exists(rec):
        with open(rec) as f:
            d = json.load(f)
    d.setdefault("engine_layer_err_vs_float64", {})[label] = {str(k): float(v) for k, v in errs.items()}
    with open(rec, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module", params=["eager", "graph"])
def f32_lstm_rollout(hip_lib, request):
    """3 paths x 16 envs, T = 4, episodes of 5 steps (they end inside the rollout), device GA.  "graph": hipGraph
    capture + replays, the last of 3 replays compared."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    mode = request.param
    cfg = reference_cfg(graph=mode == "graph")
    tr = PathNetTrainer(cfg, device=DEV)
    eng = tr.engine
    assert tr.compute_dtype == "fp32" and tr.model.hip.f32
    assert eng.lstm_hip and not eng.hybrid and eng.hst.dtype == torch.float32
    assert eng.use_graph == (mode == "graph")
    tr.env.max_episode_steps = 5
    for _ in range(3 if cfg.use_graph else 1):
        tr.update()
    tr.flush()
    if not cfg.use_graph:
        tr.model.set_paths(masks_with_edges(3, cfg.net.L, cfg.net.M, cfg.net.N, seed=2))
    else:
        assert eng.g_rollout is not None
    eng.rollout_backward()
    torch.cuda.synchronize()
    assert eng.dones.any()
    return (tr, eng, *_oracles(_oracle_grad_lstm, tr, eng), eng.grad_flat.clone(), mode)


def test_f32_lstm_engine_gradient_vs_float64_and_plain_fp32_oracle(f32_lstm_rollout):
    tr, eng, g64, g32, g_hip, mode = f32_lstm_rollout
    err = check_layers(f"fp32 LSTM engine ({mode})", tr, g_hip, g64, g32)
    assert "lstm" in err
    record_layers(mode, err)


def test_f32_lstm_gradient_check_detects_a_two_percent_error(f32_lstm_rollout):
    """Negative control: the LSTM kernel's (and bias') gradient scaled by 1.02 must fail the per-layer budget."""
    tr, eng, g64, g32, g_hip, _ = f32_lstm_rollout
    o32 = layer_errors(tr, g32, g64)["lstm"]
    for name in ("lstm.kernel", "lstm.bias"):
        s = tr.model.store.layout.by_name[name]
        bad = g_hip.clone()
        bad[s.offset:s.offset + s.numel] *= 1.02
        assert layer_errors(tr, bad, g64)["lstm"] > max(X3_LAYER_TOL, 1.25 * o32), name


def test_f32_lstm_updates_are_bit_reproducible(hip_lib):
    """Two trainers from one seed: 4 graph-replayed updates with episode ends give the same bits in the weights, the
    gradient and the carried recurrent state (no float atomics anywhere in the fp32 engine, sampler included)."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer

    def run():
        cfg = reference_cfg(paths=4, envs=16, tmax=5, graph=True)
        cfg.ga.concurrent_tournaments = 1
        tr = PathNetTrainer(cfg, device=DEV)
        eng = tr.engine
        assert tr.model.hip.deterministic and eng.lstm_hip and eng.use_graph
        tr.env.max_episode_steps = 7
        for _ in range(4):
            tr.update()
        tr.flush()
        torch.cuda.synchronize()
        assert eng.g_rollout is not None          # 20 steps of 7-step episodes: ends inside updates 2 and 3
        return (tr.model.store.flat.detach().clone(), eng.grad_flat.clone(), eng.hst[0].clone(), eng.cst[0].clone())

    a, b = run(), run()
    assert float(a[2].abs().sum()) > 0 and float(a[1].abs().sum()) > 0
    for name, x, y in zip(("weights", "grad_flat", "hst[0]", "cst[0]"), a, b):
        assert torch.equal(x, y), (name, float((x - y).abs().max()))


def test_fp32x_config_without_split_operand_trunk_lands_on_the_fused_fp32_lstm(hip_lib):
    """The LSTM preset at fp32x with a third conv layer of 4x4 / stride 1 (no fp32x kernel): the trainer warns, runs
    the fp32 engine, and that engine runs the fused, captured LSTM."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = reference_cfg(graph=True, dtype="fp32x")
    cfg.net.layers[2] = LayerSpec("conv", 8, 4, 1)
    with pytest.warns(UserWarning, match="fp32x"):
        tr = PathNetTrainer(cfg, device=DEV)
    eng = tr.engine
    assert tr.compute_dtype == "fp32" and tr.precision_note
    assert eng.lstm_hip and not eng.hybrid and eng.use_graph
    tr.env.max_episode_steps = 5
    for _ in range(2):
        tr.update()
    tr.flush()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.model.store.flat).all()) and bool(torch.isfinite(eng.hst).all())


def test_f32_lstm_checkpoint_round_trip_gives_a_bit_equal_update(hip_lib, tmp_path):
    """State saved after 2 updates and loaded into a fresh trainer: the third update has the same bits."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.utils import checkpoint

    def make():
        tr = PathNetTrainer(reference_cfg(graph=False), device=DEV)
        tr.env.max_episode_steps = 5
        return tr

    tr = make()
    for _ in range(2):
        tr.update()
    tr.flush()
    h, c = (t.clone() for t in tr.engine.lstm_state_tensors())
    assert h.dtype == torch.float32 and float(h.abs().sum()) > 0
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


def test_f32_lstm_switch_keeps_the_hybrid_path(hip_lib, monkeypatch):
    """PATHNET_F32_LSTM=0 (A/B runs): the fp32 engine builds no fused cell and runs the autograd hybrid, eagerly."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    monkeypatch.setenv("PATHNET_F32_LSTM", "0")
    tr = PathNetTrainer(reference_cfg(graph=True), device=DEV)
    eng = tr.engine
    assert tr.model.hip.lstm is None and eng.hybrid and not eng.lstm_hip and not eng.use_graph
    tr.update()
    tr.flush()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.model.store.flat).all())
