"""GAConfig.frozen_mode ("or" | "available") and the counter-hash ``down`` operator of the device GA's host mirror
(CPU, torch backend): expressed masks, the operator against its scalar oracle, its properties and rates, the
CounterPopulation dispatch, the trainer across a task boundary, checkpoints, the evaluator and the CLI."""
import json
import math

import numpy as np
import pytest
import torch

from pathnet_gym_amd.algo import ga
from pathnet_gym_amd.algo.ga import Population, express
from pathnet_gym_amd.algo.trainer import PathNetTrainer
from pathnet_gym_amd.config import TrainConfig, preset
from pathnet_gym_amd.utils import checkpoint as ckpt


# ---------------------------------------------------------------------------
# expressed masks
# ---------------------------------------------------------------------------
def test_expressed_follows_frozen_mode():
    pops = {m: Population(12, 3, 6, 2, 3, seed=4, frozen_mode=m) for m in ("or", "available")}
    assert Population(12, 3, 6, 2, 3, seed=4).frozen_mode == "or"                 # the default is the reference's rule
    for pop in pops.values():
        pop.frozen[0, 5] = 1
        pop.frozen[2, 1] = 1
    g = pops["or"].genotypes
    assert np.array_equal(g, pops["available"].genotypes)
    fr = pops["or"].frozen
    today = ((g > 0.5) | (fr[None] > 0.5)).astype(np.float32)                     # the rule as it was hard-coded
    assert not np.array_equal(today, g)                                            # some path does not select them
    assert np.array_equal(pops["or"].expressed(), today)
    assert pops["or"].expressed().dtype == np.float32
    assert np.array_equal(pops["available"].expressed(), g)
    assert pops["available"].expressed().dtype == np.float32
    assert np.array_equal(express(g[3], fr), today[3])
    assert np.array_equal(express(g[3], fr, "or"), today[3])
    assert np.array_equal(express(g[3], fr, "available"), g[3])
    with pytest.raises(ValueError):
        express(g[3], fr, "and")
    with pytest.raises(ValueError):
        Population(12, 3, 6, 2, 3, frozen_mode="always")
    pops["or"].frozen_mode = "nope"
    with pytest.raises(ValueError):
        pops["or"].expressed()


def test_trainer_rejects_unknown_frozen_mode():
    cfg = preset("cartpole-cpu")
    cfg.ga.frozen_mode = "union"
    with pytest.raises(ValueError):
        PathNetTrainer(cfg)


# ---------------------------------------------------------------------------
# counter_mutation_down
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L,M,N", [(5, 10, 4), (1, 2, 1)])
def test_counter_mutation_down_vectorised_draws_match_scalar(L, M, N):
    from pathnet_gym_amd.algo.ga_device import counter_mutation_down, counter_mutation_down_scalar
    rng = np.random.RandomState(0)
    changed = 0
    for _ in range(200):
        g = (rng.rand(L, M) < 0.5).astype(np.float32)
        seed, gen, path = int(rng.randint(0, 2 ** 32 - 1)), int(rng.randint(0, 10 ** 7)), int(rng.randint(0, 4096))
        a = counter_mutation_down(g.copy(), L, M, N, seed, gen, path)
        b = counter_mutation_down_scalar(g.copy(), L, M, N, seed, gen, path)
        assert np.array_equal(a, b)
        assert a is not g and set(np.unique(a)) <= {0.0, 1.0}
        changed += not np.array_equal(a, g)
    assert changed > 20                                        # the comparison saw moves, not 200 untouched rows


def test_counter_mutation_down_properties():
    """Inactive modules only light up under a move, a layer never grows, and a move from j lands on
    max(j-4,0)..max(j-1,0).  Rows with ONE active module make the move and its offset readable from the result."""
    from pathnet_gym_amd.algo.ga_device import counter_mutation_down
    L, M, N = 4, 10, 1                                          # L*N = 4: an active module moves half the time
    rng = np.random.RandomState(1)
    moves = 0
    landed = {j: set() for j in range(M)}
    for it in range(600):
        g = (rng.rand(L, M) < 0.4).astype(np.float32)
        g[it % L] = 0
        g[it % L, (M - 1) if it % 3 == 0 else it % M] = 1       # one layer with a single module, often module M-1
        out = counter_mutation_down(g.copy(), L, M, N, seed=77, gen=it, path=it % 13)
        for l in range(L):
            assert out[l].sum() <= g[l].sum()                   # never grows
            lit = np.nonzero((out[l] == 1) & (g[l] == 0))[0]
            gone = np.nonzero((out[l] == 0) & (g[l] == 1))[0]
            for t in lit:                                       # ... some active module above it moved onto it
                assert any(max(j - 4, 0) <= t <= max(j - 1, 0) for j in np.nonzero(g[l])[0])
            assert len(lit) <= len(gone)                        # every newly lit module cost a vacated one
            if g[l].sum() == 1:
                j = int(np.nonzero(g[l])[0][0])
                assert out[l].sum() == 1
                t = int(np.nonzero(out[l])[0][0])
                if t != j:
                    moves += 1
                    assert max(j - 4, 0) <= t <= max(j - 1, 0), (j, t)
                    landed[j].add(t)
    assert moves > 100
    assert landed[M - 1] == {M - 5, M - 4, M - 3, M - 2}        # all four offsets from the top module
    # an all-inactive genotype draws nothing and stays empty
    z = np.zeros((L, M), np.float32)
    assert not counter_mutation_down(z.copy(), L, M, N, 1, 2, 3).any()


def test_counter_mutation_down_smallest_shape_always_moves_to_module_zero():
    """(L,M,N) = (1,2,1): L*N = 1, so u24 * 1 < 2^25 always holds -- every active module moves on every call and every
    target clamps to 0: the result is module 0 alone, whatever was active."""
    from pathnet_gym_amd.algo.ga_device import counter_mutation_down, counter_mutation_down_scalar
    want = np.array([[1.0, 0.0]], np.float32)
    for fn in (counter_mutation_down, counter_mutation_down_scalar):
        for start in ([[1, 0]], [[0, 1]], [[1, 1]]):
            for gen in range(50):
                out = fn(np.array(start, np.float32), 1, 2, 1, seed=gen * 7919 + 1, gen=gen, path=gen % 3)
                assert np.array_equal(out, want), (start, gen)
        assert not fn(np.zeros((1, 2), np.float32), 1, 2, 1, 5, 6, 0).any()


def test_counter_mutation_down_rates_match_reference_operator():
    """Move frequency p = 2/(L*N) and the four offsets at 1/4 each, within 5 sigma of a binomial over n (active
    module, call) pairs -- for the counter-hash operator and, in the same test, for the host operator
    (ga.mutation_down on MT19937), so the bounds are ones the reference operator itself stays within.

    Every row holds one active module at j >= 4: no clamp applies and (moved, offset) is read off the result.
    n = 64000 pairs: the move bound 5*sqrt(p(1-p)/n) = 0.0065 is 5.2 % of p = 1/8."""
    from pathnet_gym_amd.algo.ga_device import counter_mutation_down
    L, M, N = 4, 10, 4
    p = 2.0 / (L * N)
    calls = 16000
    n = calls * L
    bound = 5.0 * math.sqrt(p * (1 - p) / n)
    assert bound < 0.1 * p
    rng = np.random.RandomState(99)

    def run(op):
        moved, offs = 0, {-4: 0, -3: 0, -2: 0, -1: 0}
        for c in range(calls):
            g = np.zeros((L, M), np.float32)
            js = [4 + (c + 5 * l) % (M - 4) for l in range(L)]
            for l, j in enumerate(js):
                g[l, j] = 1
            out = op(g, c)
            for l, j in enumerate(js):
                assert out[l].sum() == 1
                t = int(np.nonzero(out[l])[0][0])
                if t != j:
                    moved += 1
                    offs[t - j] += 1
        return moved, offs

    results = {
        "counter": run(lambda g, c: counter_mutation_down(g, L, M, N, seed=123, gen=c, path=c % 29)),
        "mt19937": run(lambda g, c: ga.mutation_down(g, L, M, N, rng)),
    }
    for name, (moved, offs) in results.items():
        assert sum(offs.values()) == moved
        assert abs(moved / n - p) < bound, (name, moved / n, p, bound)
        ob = 5.0 * math.sqrt(0.25 * 0.75 / moved)
        for o, k in offs.items():
            assert abs(k / moved - 0.25) < ob, (name, o, k / moved, ob)


# ---------------------------------------------------------------------------
# CounterPopulation dispatch
# ---------------------------------------------------------------------------
def _feed(pop, steps=80):
    """The random fitness feed of tests/test_hip_kernels.py::test_device_ga_matches_host_mirror."""
    rng = np.random.RandomState(0)
    fired = []
    for t in range(steps):
        f = pop.fitness.copy()
        fresh = rng.rand(pop.P) < 0.35
        f[fresh] = rng.randint(-21, 22, int(fresh.sum())).astype(np.float32)
        evs = pop.step(f, t)
        fired.append([(e.generation, tuple(e.candidates), e.winner) for e in evs])
        yield t
    pop._fired = fired


def test_counter_population_down_never_grows_and_fires_like_ref():
    from pathnet_gym_amd.algo.ga_device import CounterPopulation
    P, L, M, N, B, C = 40, 5, 10, 4, 3, 6
    down = CounterPopulation(P, L, M, N, B, seed=3, concurrent=C, mutation_kind="down")
    ref = CounterPopulation(P, L, M, N, B, seed=3, concurrent=C)
    assert np.array_equal(down.genotypes, ref.genotypes)
    for _ in _feed(down):
        assert down.genotypes.sum(2).max() <= N                 # down cannot grow a path
    for _ in _feed(ref):
        pass
    # tournaments, candidates and winners do not depend on the operator
    assert down._fired == ref._fired
    assert sum(len(x) for x in down._fired) > 30
    assert down.generation == ref.generation
    assert not np.array_equal(down.genotypes, ref.genotypes)
    assert ref.genotypes.sum(2).max() > N                       # the ref operator does grow paths under this feed
    with pytest.raises(ValueError):
        CounterPopulation(P, L, M, N, B, seed=3, concurrent=C, mutation_kind="up")
    down.mutation_kind = "sideways"
    with pytest.raises(ValueError):
        down.step(down.fitness.copy(), 0)


# ---------------------------------------------------------------------------
# trainer across the task boundary (torch backend)
# ---------------------------------------------------------------------------
def _two_task_cfg(mode):
    cfg = preset("cartpole-cpu")
    cfg.paths, cfg.envs_per_path = 4, 4
    cfg.tasks = ["CartPole-v1", "CartPole-v1"]
    cfg.ga.frozen_mode = mode
    return cfg


def _frozen_segments(tr, frozen):
    return [s for s in tr.model.store.layout.segments if s.layer >= 0 and frozen[s.layer, s.module] > 0.5]


def _run_two_tasks(mode, n1=6, n2=8):
    torch.manual_seed(0)
    tr = PathNetTrainer(_two_task_cfg(mode))
    assert tr.pop.frozen_mode == mode
    for _ in range(n1):
        tr.update()
    winner, frozen = tr.end_task()
    tr._start_task(1)                                           # as scripts/continual.py train_task does
    # one path selects a frozen module on purpose (fresh genotypes may or may not)
    l0, j0 = [int(x[0]) for x in np.nonzero(frozen > 0.5)]
    tr.pop.genotypes[0, l0, j0] = 1.0
    tr._push_genotypes()
    after_freeze = tr.model.store.flat.detach().clone()
    selected = 0
    for _ in range(n2):
        selected += int((tr.model.mask.cpu().numpy()[:, frozen > 0.5] > 0.5).any())
        tr.update()
    return tr, frozen, after_freeze, selected


def test_trainer_available_mode_keeps_frozen_modules_out_of_the_masks():
    tr, frozen, after_freeze, selected = _run_two_tasks("available")
    lo, hi = tr.path_offset, tr.path_offset + tr.P
    mask = tr.model.mask.cpu().numpy()
    assert np.array_equal(mask, tr.pop.genotypes[lo:hi])                      # nothing ORed in
    assert np.array_equal(tr.pop.expressed(), tr.pop.genotypes)
    assert frozen.sum() > 0 and selected > 0                                  # a frozen module was in use in task 2
    flat = tr.model.store.flat.detach()
    segs = _frozen_segments(tr, frozen)
    assert segs
    for s in segs:                                                            # selected or not: never trained
        sl = slice(s.offset, s.offset + s.numel)
        assert torch.equal(flat[sl], after_freeze[sl]), s.name
    frozen_ids = {id(s) for s in segs}
    assert any(not torch.equal(flat[s.offset:s.offset + s.numel], after_freeze[s.offset:s.offset + s.numel])
               for s in tr.model.store.layout.segments if id(s) not in frozen_ids)
    assert torch.isfinite(flat).all()


def test_trainer_or_mode_still_forces_frozen_modules():
    tr, frozen, after_freeze, _ = _run_two_tasks("or")
    lo, hi = tr.path_offset, tr.path_offset + tr.P
    want = ((tr.pop.genotypes[lo:hi] > 0.5) | (frozen[None] > 0.5)).astype(np.float32)
    assert np.array_equal(tr.model.mask.cpu().numpy(), want)
    assert (tr.model.mask.cpu().numpy()[:, frozen > 0.5] == 1).all()
    flat = tr.model.store.flat.detach()
    for s in _frozen_segments(tr, frozen):
        sl = slice(s.offset, s.offset + s.numel)
        assert torch.equal(flat[sl], after_freeze[sl]), s.name


# ---------------------------------------------------------------------------
# checkpoints, evaluator, CLI
# ---------------------------------------------------------------------------
def test_checkpoint_resume_in_available_mode_is_exact(tmp_path, monkeypatch):
    torch.manual_seed(0)
    a = PathNetTrainer(_two_task_cfg("available"))
    for _ in range(5):
        a.update()
    _, frozen = a.end_task()
    a._start_task(1)
    for _ in range(3):
        a.update()
    p = str(tmp_path / "ck.safetensors")
    ckpt.save(a, p)
    torch.manual_seed(123)
    for _ in range(4):
        a.update()
    stored = ckpt.read_config(p)
    assert stored.ga.frozen_mode == "available"
    assert json.loads(ckpt.read_metadata(p)["config"])["ga"]["frozen_mode"] == "available"
    b = PathNetTrainer(stored)
    ckpt.load(b, p)
    assert b.task_idx == 1 and b.pop.frozen_mode == "available"
    assert np.array_equal(b.pop.frozen, frozen)
    torch.manual_seed(123)
    for _ in range(4):
        b.update()
    assert torch.equal(a.model.store.flat, b.model.store.flat)
    assert np.array_equal(a.pop.genotypes, b.pop.genotypes)
    assert np.array_equal(a.pop.fitness, b.pop.fitness) and a.pop.candidates == b.pop.candidates
    assert a.pop.generation == b.pop.generation and a.global_step == b.global_step
    assert np.array_equal(b.model.mask.cpu().numpy(), b.pop.genotypes)

    # the evaluator follows cfg.ga.frozen_mode: masks of the stored genotypes, without / with the frozen modules
    from pathnet_gym_amd.algo import evaluate
    seen = {}

    def fake_eval(model, env_id, *args, **kw):
        seen["mask"] = model.mask.cpu().numpy().copy()
        return [0.0] * model.P

    monkeypatch.setattr(evaluate, "evaluate_model", fake_eval)
    from safetensors.torch import load_file
    d = load_file(p)
    g = d["ga.genotypes"].numpy().astype(np.float32)
    fr = d["ga.frozen"].numpy().astype(np.float32)
    assert fr.sum() > 0
    res = evaluate.evaluate_checkpoint(stored, p)
    assert res["task"] == 1 and np.array_equal(seen["mask"], g)
    stored.ga.frozen_mode = "or"
    evaluate.evaluate_checkpoint(stored, p)
    assert np.array_equal(seen["mask"], ((g > 0.5) | (fr[None] > 0.5)).astype(np.float32))


def test_config_json_without_frozen_mode_loads_as_or():
    cfg = preset("cartpole-cpu")
    cfg.ga.frozen_mode = "available"
    d = json.loads(cfg.to_json())
    assert d["ga"]["frozen_mode"] == "available"
    assert TrainConfig.from_json(json.dumps(d)).ga.frozen_mode == "available"
    del d["ga"]["frozen_mode"]                                 # a checkpoint written before the field existed
    old = TrainConfig.from_json(json.dumps(d))
    assert old.ga.frozen_mode == "or"
    assert preset("pong").ga.frozen_mode == "or" and preset("reference").ga.frozen_mode == "or"


def test_cli_train_takes_frozen_mode_and_mutation():
    from pathnet_gym_amd.cli import build_parser, config_from_args
    ap = build_parser()
    a = ap.parse_args(["train", "--preset", "cartpole-cpu", "--frozen_mode", "available", "--mutation", "down"])
    cfg = config_from_args(a)
    assert cfg.ga.frozen_mode == "available" and cfg.ga.mutation == "down"
    cfg = config_from_args(ap.parse_args(["train", "--preset", "cartpole-cpu"]))
    assert cfg.ga.frozen_mode == "or" and cfg.ga.mutation == "ref"
    with pytest.raises(SystemExit):
        ap.parse_args(["train", "--frozen_mode", "and"])
