"""The ``backend`` argument of the evaluate_* functions, ``cli eval``'s flags and the solve tracker's pass-through,
without a GPU: "torch" is the code it always was, "hip" needs a GPU, "auto" falls back."""
import json
import math

import numpy as np
import pytest
import torch

from pathnet_gym_amd.algo import evaluate
from pathnet_gym_amd.config import preset
from pathnet_gym_amd.models.acnet import ACPathNet


def cart_model(P=3, seed=4):
    from pathnet_gym_amd.algo.ga import get_geopath
    net = preset("cartpole-cpu").net
    m = ACPathNet(net, P, "cpu", "torch", seed=seed)
    rng = np.random.RandomState(1)
    m.set_paths(np.stack([get_geopath(net.L, net.M, net.N, rng) for _ in range(P)]).astype(np.float32))
    return net, m


def test_torch_backend_is_the_call_without_the_argument():
    net, m = cart_model()
    for sample in (False, True):
        a = evaluate.evaluate_model(m, "CartPole-v1", episodes=2, max_steps=700, seed=5, sample=sample)
        info = {}
        b = evaluate.evaluate_model(m, "CartPole-v1", episodes=2, max_steps=700, seed=5, sample=sample,
                                    backend="torch", info=info)
        assert a == b and all(math.isfinite(x) for x in a)
        assert info["backend"] == "torch" and info["compute_dtype"] == "fp32" and 10 < info["steps"] <= 700
    short = {}
    evaluate.evaluate_model(m, "CartPole-v1", episodes=2, max_steps=3, info=short)
    assert short["steps"] == 3          # no CartPole episode ends within 3 steps
    path = m.mask[0].numpy()
    a = evaluate.evaluate_path(net, m.store.flat, path, "CartPole-v1", episodes=6, seed=7, max_steps=600)
    b = evaluate.evaluate_path(net, m.store.flat, path, "CartPole-v1", episodes=6, seed=7, max_steps=600,
                               backend="torch", compute_dtype=None)
    assert a == b and a["finished"] == 6 and a["backend"] == "torch" and a["compute_dtype"] == "fp32"
    for k in ("mean", "min", "max", "finished", "episodes", "steps", "policy", "seed", "returns"):
        assert k in a, k


def test_unknown_backend_is_refused():
    net, m = cart_model()
    with pytest.raises(ValueError, match="backend"):
        evaluate.evaluate_model(m, "CartPole-v1", backend="cuda")
    with pytest.raises(ValueError, match="backend"):
        evaluate.evaluate_path(net, m.store.flat, m.mask[0].numpy(), "CartPole-v1", episodes=2, backend="triton")


def test_hip_needs_a_gpu_and_auto_falls_back_to_torch(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # also where one is visible
    net, m = cart_model()
    path = m.mask[0].numpy()
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate.evaluate_model(m, "CartPole-v1", backend="hip")
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate.evaluate_path(net, m.store.flat, path, "CartPole-v1", episodes=2, backend="hip")
    a = evaluate.evaluate_model(m, "CartPole-v1", episodes=2, max_steps=700, seed=5)
    assert evaluate.evaluate_model(m, "CartPole-v1", episodes=2, max_steps=700, seed=5, backend="auto") == a
    p = evaluate.evaluate_path(net, m.store.flat, path, "CartPole-v1", episodes=4, seed=7, max_steps=600)
    q = evaluate.evaluate_path(net, m.store.flat, path, "CartPole-v1", episodes=4, seed=7, max_steps=600,
                               backend="auto")
    assert p == q and q["backend"] == "torch"
    from pathnet_gym_amd.runtime.evaluator import HipEvaluator
    with pytest.raises(RuntimeError, match="GPU"):
        HipEvaluator(net, "CartPole-v1", 2, 2, device="cuda")
    with pytest.raises(RuntimeError, match="GPU"):
        HipEvaluator(net, "CartPole-v1", 2, 2, device="cpu")


def test_the_evaluators_envelope_is_host_arithmetic():
    """``auto`` asks unsupported_reason before it touches a GPU: the answers need none."""
    from pathnet_gym_amd.runtime.evaluator import env_shape, min_envs_per_path, unsupported_reason
    cart, pong, ref = preset("cartpole").net, preset("pong").net, preset("reference").net
    assert unsupported_reason(cart, "CartPole-v1", None, 1) is None
    assert unsupported_reason(pong, "Pong", "fp32x", 16) is None
    assert unsupported_reason(ref, "Alien", "bf16", 32) is None
    assert "host" in unsupported_reason(cart, "PyCartPole-v1", None, 1)
    assert "host" in unsupported_reason(pong, "Pong-v0", None, 16)
    assert "multiple of 16" in unsupported_reason(pong, "Pong", None, 4)
    assert "> 32" in unsupported_reason(pong, "Pong", None, 48)
    ref.lstm_size = 100
    assert "hybrid" in unsupported_reason(ref, "Alien", "fp32", 16)
    assert "compute_dtype" in unsupported_reason(cart, "CartPole-v1", "fp16", 1)
    assert (min_envs_per_path(cart), min_envs_per_path(pong)) == (1, 16)
    assert env_shape(pong, 64) == (2, 32) and env_shape(pong, 5) == (1, 16) and env_shape(cart, 5) == (1, 5)
    assert env_shape(cart, 256) == (8, 32) and env_shape(pong, 33) == (2, 32)


def _tiny_checkpoint(tmp_path):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.utils import checkpoint as ckpt
    cfg = preset("cartpole-cpu")
    cfg.gc_freeze = False
    tr = PathNetTrainer(cfg, device="cpu")
    p = str(tmp_path / "ck.safetensors")
    ckpt.save(tr, p)
    return cfg, p


def test_evaluate_checkpoint_keeps_its_keys_and_adds_the_backend(tmp_path):
    cfg, p = _tiny_checkpoint(tmp_path)
    a = evaluate.evaluate_checkpoint(cfg, p, episodes=1, max_steps=600)
    b = evaluate.evaluate_checkpoint(cfg, p, episodes=1, max_steps=600, backend="torch", sample=False, seed=12345)
    assert a == b
    for k in ("env", "task", "returns", "best_path", "best_return", "backend", "compute_dtype", "steps"):
        assert k in a, k
    assert a["backend"] == "torch" and len(a["returns"]) == cfg.paths and a["best_return"] == max(a["returns"])
    c = evaluate.evaluate_checkpoint(cfg, p, episodes=1, max_steps=600, sample=True, seed=3)
    assert c["returns"] != a["returns"]


def test_cli_eval_flags_reach_evaluate_checkpoint(tmp_path, monkeypatch, capsys):
    from pathnet_gym_amd import cli
    seen = {}

    def fake(cfg, path, **kw):
        seen.update(kw, path=path, tasks=list(cfg.tasks))
        return {"returns": []}

    monkeypatch.setattr(evaluate, "evaluate_checkpoint", fake)
    ap = cli.build_parser()
    cli.cmd_eval(ap.parse_args(["eval", "--preset", "cartpole-cpu", "--checkpoint", "x.safetensors"]))
    assert seen == dict(path="x.safetensors", tasks=["CartPole-v1"], episodes=1, max_steps=2000, device="cpu",
                        backend="torch", compute_dtype=None, sample=False, seed=12345)
    assert json.loads(capsys.readouterr().out) == {"returns": []}
    built = []
    from pathnet_gym_amd import _build
    monkeypatch.setattr(_build, "build", lambda *a, **k: built.append(1))
    cli.cmd_eval(ap.parse_args(["eval", "--preset", "cartpole-cpu", "--checkpoint", "y", "--backend", "auto",
                                "--device", "cuda:0", "--sample", "--seed", "9", "--compute_dtype", "fp32x",
                                "--episodes", "3", "--max_steps", "50"]))
    assert seen == dict(path="y", tasks=["CartPole-v1"], episodes=3, max_steps=50, device="cuda:0", backend="auto",
                        compute_dtype="fp32x", sample=True, seed=9)
    assert bool(built) == torch.cuda.is_available()          # the kernels are built before a hip run, as cmd_train does
    with pytest.raises(SystemExit):
        ap.parse_args(["eval", "--checkpoint", "y", "--backend", "triton"])


def test_solve_tracker_passes_confirm_backend_through(monkeypatch):
    from pathnet_gym_amd.algo.solve import SolveTracker
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset("cartpole-cpu")
    cfg.gc_freeze = False
    tr = PathNetTrainer(cfg, device="cpu")
    calls = []

    def fake(net_cfg, flat, expressed, env_id, **kw):
        calls.append(kw)
        return {"mean": 1.0}

    monkeypatch.setattr(evaluate, "evaluate_path", fake)
    SolveTracker(tr, confirm_episodes=4).confirm(0)
    assert "backend" not in calls[-1] and "compute_dtype" not in calls[-1]      # the default: the call it always was
    trk = SolveTracker(tr, confirm_episodes=4, confirm_backend="hip")
    trk.confirm(0)
    assert calls[-1]["backend"] == "hip" and calls[-1]["compute_dtype"] == tr.compute_dtype
    assert calls[-1]["episodes"] == 4 and calls[-1]["seed"] == trk.eval_seed
    assert "hip" in trk.record()["confirm_policy"]
    SolveTracker(tr, confirm_backend="auto", confirm_compute_dtype="fp32x").confirm(0)
    assert calls[-1]["backend"] == "auto" and calls[-1]["compute_dtype"] == "fp32x"
    assert SolveTracker(tr).record()["confirm_policy"] == "sampled, fp32 PyTorch forward"
