"""Device GA with an operator / frozen-rule argument (csrc/ga.hip launch_ga_step_ex, launch_ga_compact_ex) against
the host mirror (algo/ga_device.CounterPopulation) and the unchanged entry points, and the HIP trainer with
frozen_mode="available" + mutation="down" across a task boundary (run on an MI355X)."""
import numpy as np
import pytest
import torch

from pathnet_gym_amd.algo.ga import compact_active
from pathnet_gym_amd.algo.ga_device import CounterPopulation
from pathnet_gym_amd.config import preset

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -22


class DevGA:
    """The device GA's buffers for one population (the layout of runtime/engine.py enable_device_ga)."""

    def __init__(self, pop):
        self.pop = pop
        self.geno = torch.from_numpy(pop.genotypes.astype(np.uint8)).to(DEV)
        self.slots = torch.from_numpy(pop.slots.astype(np.int32)).to(DEV)
        self.gen = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.events = torch.zeros(pop.concurrent, 3, dtype=torch.int32, device=DEV)
        self.fit = None
        self.reset = None

    def step(self, f, entry, mut_kind=None):
        from pathnet_gym_amd.ops import _lib
        p = self.pop
        self.fit = torch.from_numpy(f).to(DEV)
        self.reset = torch.full((p.P,), 7, dtype=torch.uint8, device=DEV)
        head = (self.geno.data_ptr(), self.fit.data_ptr(), self.slots.data_ptr(), self.gen.data_ptr(),
                self.events.data_ptr(), p.P, p.L, p.M, p.N, p.B, p.concurrent, p.seed32)
        mid = () if mut_kind is None else (mut_kind,)
        _lib.call(entry, *head, *mid, self.reset.data_ptr(), _lib.stream())

    def state(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("geno", "slots", "fit", "events", "gen", "reset")}


def feed(pop, steps=80):
    """The random fitness feed of test_hip_kernels.py::test_device_ga_matches_host_mirror: yields the vector fed to
    the device, then steps the host mirror with it."""
    rng = np.random.RandomState(0)
    for t in range(steps):
        f = pop.fitness.copy()
        fresh = rng.rand(pop.P) < 0.35
        f[fresh] = rng.randint(-21, 22, int(fresh.sum())).astype(np.float32)
        evs = pop.step(f.copy(), t)
        yield t, f, evs


def test_step_ex_ref_equals_old_entry_point(hip_lib):
    P, L, M, N, B, C = 40, 5, 10, 4, 3, 6
    pop = CounterPopulation(P, L, M, N, B, seed=3, concurrent=C)
    old, new = DevGA(pop), DevGA(pop)
    fired = 0
    for t, f, evs in feed(pop):
        fired += len(evs)
        old.step(f, "launch_ga_step")
        new.step(f, "launch_ga_step_ex", 0)
        a, b = old.state(), new.state()
        for k in a:
            assert np.array_equal(a[k], b[k]), (t, k)
        assert np.array_equal(b["geno"], pop.genotypes.astype(np.uint8)), t
    assert fired > 30


@pytest.mark.parametrize("shape,min_fired", [
    ((40, 5, 10, 4, 3, 6), 31),
    ((3, 1, 2, 1, 3, 1), 1),        # L*N = 1: every active module moves every time, clamp to 0, one slot
    ((20, 16, 16, 4, 2, 8), 1),     # GA_MAXL, GA_MAXM; C*B*L = 256 items = the block size
    ((150, 5, 10, 4, 3, 6), 1),     # more than 64 paths; C*B*L not a multiple of the block
])
def test_down_on_device_equals_mirror(hip_lib, shape, min_fired):
    P, L, M, N, B, C = shape
    pop = CounterPopulation(P, L, M, N, B, seed=3, concurrent=C, mutation_kind="down")
    dev = DevGA(pop)
    fired = 0
    for t, f, evs in feed(pop):
        fired += len(evs)
        dev.step(f, "launch_ga_step_ex", 1)
        s = dev.state()
        want = np.zeros(P, np.uint8)
        for e in evs:
            want[e.candidates] = 1
        assert np.array_equal(s["reset"], want), t
        assert np.array_equal(s["geno"], pop.genotypes.astype(np.uint8)), t
        assert np.array_equal(s["slots"], pop.slots.astype(np.int32)), t
        assert np.array_equal(s["fit"], pop.fitness), t
        assert int(s["gen"][0]) == pop.generation, t
        assert pop.genotypes.sum(2).max() <= N
    assert fired >= min_fired
    if (L, M, N) == (1, 2, 1):
        # every loser of every tournament is module 0 alone
        losers = {i for e in pop.history for i in e.candidates if i != e.winner}
        assert losers and all(np.array_equal(pop.genotypes[i], [[1.0, 0.0]]) for i in losers)


def _compact(entry, geno, frozen, off, Pl, L, M, mode=None, fill=0):
    from pathnet_gym_amd.ops import _lib
    out = dict(mask=torch.full((Pl, L, M), float(fill), device=DEV),
               ai=torch.full((Pl, L, M), fill, dtype=torch.int32, device=DEV),
               ac=torch.full((Pl, L), fill, dtype=torch.int32, device=DEV),
               ip=torch.full((L, M, Pl), fill, dtype=torch.int32, device=DEV),
               isl=torch.full((L, M, Pl), fill, dtype=torch.int32, device=DEV),
               ic=torch.full((L, M), fill, dtype=torch.int32, device=DEV))
    mid = () if mode is None else (mode,)
    rc = getattr(_lib.lib(), entry)(geno.data_ptr(), frozen.data_ptr(), off, Pl, L, M, *mid,
                                    *[out[k].data_ptr() for k in ("mask", "ai", "ac", "ip", "isl", "ic")],
                                    _lib.stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _check_compact(o, expr, tails):
    Pl, L, M = expr.shape
    idx, cnt = compact_active(expr)
    assert np.array_equal(o["mask"], expr)
    assert np.array_equal(o["ai"], idx) and np.array_equal(o["ac"], cnt)
    for l in range(L):
        for j in range(M):
            users = [p for p in range(Pl) if expr[p, l, j] > 0.5]
            assert int(o["ic"][l, j]) == len(users)
            assert o["ip"][l, j, :len(users)].tolist() == users
            assert o["isl"][l, j, :len(users)].tolist() == [int(expr[p, l, :j].sum()) for p in users]
            if tails:
                assert (o["ip"][l, j, len(users):] == 0).all() and (o["isl"][l, j, len(users):] == 0).all()


def _mode_population(P, seed):
    """A population with an empty and a full layer, module [2,7] frozen and a frozen module [4,3] no path selects."""
    L, M, N, B, C = 5, 10, 4, 3, 6
    pop = CounterPopulation(P, L, M, N, B, seed=seed, concurrent=C, frozen_mode="available")
    pop.genotypes[9, 1, :] = 0
    pop.genotypes[10, 3, :] = 1
    pop.genotypes[:, 4, 3] = 0
    pop.frozen[2, 7] = 1
    pop.frozen[4, 3] = 1
    return pop


def test_compact_ex_without_and_with_the_or(hip_lib):
    L, M = 5, 10
    for P, Pl, off, fill in ((40, 16, 8, 0), (150, 150, 0, -5)):
        pop = _mode_population(P, seed=3 if P == 40 else 5)
        geno = torch.from_numpy(pop.genotypes.astype(np.uint8)).to(DEV)
        frozen = torch.from_numpy(pop.frozen.astype(np.uint8)).to(DEV)
        local = pop.genotypes[off:off + Pl]
        assert not (local[:, 2, 7] > 0.5).all() and (local[:, 2, 7] > 0.5).any()    # the OR would change the masks
        rc, o = _compact("launch_ga_compact_ex", geno, frozen, off, Pl, L, M, mode=0, fill=fill)
        assert rc == 0
        assert np.array_equal(pop.expressed()[off:off + Pl], local)
        _check_compact(o, local, tails=True)
        assert o["ic"][4, 3] == 0 and o["ic"][2, 7] == int(local[:, 2, 7].sum())
        # frozen_or = 1: every output equals the unchanged entry point's (the reference's OR)
        rc1, o1 = _compact("launch_ga_compact_ex", geno, frozen, off, Pl, L, M, mode=1, fill=fill)
        rc2, o2 = _compact("launch_ga_compact", geno, frozen, off, Pl, L, M, fill=fill)
        assert rc1 == 0 and rc2 == 0
        for k in o1:
            assert np.array_equal(o1[k], o2[k]), k
        pop.frozen_mode = "or"
        _check_compact(o1, pop.expressed()[off:off + Pl], tails=True)
        assert o1["ic"][4, 3] == Pl and o1["ic"][2, 7] == Pl


def test_ex_launchers_reject_an_unknown_mode_and_write_nothing(hip_lib):
    from pathnet_gym_amd.ops import _lib
    P, L, M, N, B, C = 40, 5, 10, 4, 3, 6
    pop = _mode_population(P, seed=3)
    pop.fitness[:] = 1.0                                           # every slot is ready: a valid mode would fire
    geno = torch.from_numpy(pop.genotypes.astype(np.uint8)).to(DEV)
    frozen = torch.from_numpy(pop.frozen.astype(np.uint8)).to(DEV)
    for mode in (2, -1):
        rc, o = _compact("launch_ga_compact_ex", geno, frozen, 8, 16, L, M, mode=mode, fill=-9)
        assert rc == EINVAL
        assert all((v == -9).all() for v in o.values())
        dev = DevGA(pop)
        dev.events.fill_(-9)
        before = dev.geno.clone()
        dev.fit = torch.from_numpy(pop.fitness.copy()).to(DEV)
        dev.reset = torch.full((P,), 7, dtype=torch.uint8, device=DEV)
        rc = _lib.lib().launch_ga_step_ex(dev.geno.data_ptr(), dev.fit.data_ptr(), dev.slots.data_ptr(),
                                          dev.gen.data_ptr(), dev.events.data_ptr(), P, L, M, N, B, C, pop.seed32,
                                          mode, dev.reset.data_ptr(), _lib.stream())
        assert rc == EINVAL
        s = dev.state()
        assert np.array_equal(s["geno"], before.cpu().numpy())
        assert np.array_equal(s["slots"], pop.slots.astype(np.int32))
        assert np.array_equal(s["fit"], pop.fitness) and (s["events"] == -9).all()
        assert int(s["gen"][0]) == 0 and (s["reset"] == 7).all()


def test_active_union_is_the_same_under_both_rules(hip_lib):
    """launch_active_union computes (OR_p genotype) & ~frozen: "expressed minus frozen" under the OR and under
    "available" alike, so the device GA's all-reduce plan needs no mode."""
    from pathnet_gym_amd.ops import _lib
    from pathnet_gym_amd.parallel.comm import active_union
    P, L, M = 40, 5, 10
    pop = _mode_population(P, seed=3)
    pop.genotypes[:, 0, 6] = 0                                     # a non-frozen module nobody selects
    geno = torch.from_numpy(pop.genotypes.astype(np.uint8)).to(DEV)
    frozen = torch.from_numpy(pop.frozen.astype(np.uint8)).to(DEV)
    out = torch.full((L * M,), 9, dtype=torch.uint8, device=DEV)
    _lib.call("launch_active_union", geno.data_ptr(), frozen.data_ptr(), P, L, M, out.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    want = (pop.genotypes > 0.5).any(0) & ~(pop.frozen > 0.5)
    got = out.cpu().numpy().reshape(L, M)
    assert np.array_equal(got, want.astype(np.uint8))
    assert got[2, 7] == 0 and got[4, 3] == 0 and got[0, 6] == 0 and got.sum() == L * M - 3
    for mode in ("or", "available"):
        pop.frozen_mode = mode
        assert np.array_equal(active_union(pop.expressed(), pop.frozen), want)


def _two_task_trainer(mode, mutation):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset("cartpole")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 8, 16, 5
    cfg.tasks = ["CartPole-v1", "CartPole-v1"]
    cfg.ga.backend = "device"
    cfg.ga.concurrent_tournaments = 2
    cfg.ga.frozen_mode = mode
    cfg.ga.mutation = mutation
    return PathNetTrainer(cfg, device=DEV)


def _run_two_tasks(tr, n):
    N = tr.cfg.net.N
    for _ in range(n):
        tr.update()
    _, frozen = tr.end_task()                                      # flushes the pipelined update first
    gen1 = tr.pop.generation
    widest = int(tr.pop.genotypes.sum(2).max())
    tr._start_task(1)
    # one path selects a frozen module on purpose, keeping its layer at N modules
    l0, j0 = [int(x[0]) for x in np.nonzero(frozen > 0.5)]
    row = tr.pop.genotypes[0, l0]
    if row[j0] < 0.5:
        row[int(np.nonzero(row > 0.5)[0][0])] = 0.0
        row[j0] = 1.0
    tr._push_genotypes()
    tr.engine.ga_upload(tr.pop)
    torch.cuda.synchronize()
    after_freeze = tr.model.store.flat.detach().clone()
    for _ in range(n):
        tr.update()
    tr.flush()                                                     # the host mirror runs one update behind
    torch.cuda.synchronize()
    return frozen, after_freeze, gen1, max(widest, int(tr.pop.genotypes.sum(2).max())), N


def _frozen_params_unchanged(tr, frozen, after_freeze):
    flat = tr.model.store.flat.detach()
    n = 0
    for s in tr.model.store.layout.segments:
        if s.layer >= 0 and frozen[s.layer, s.module] > 0.5:
            sl = slice(s.offset, s.offset + s.numel)
            assert torch.equal(flat[sl], after_freeze[sl]), s.name
            n += 1
    assert n > 0
    assert not torch.equal(flat, after_freeze)                     # the rest did train
    assert torch.isfinite(flat).all()


def test_hip_trainer_available_down_across_a_task_boundary(hip_lib):
    tr = _two_task_trainer("available", "down")
    frozen, after_freeze, gen1, widest, N = _run_two_tasks(tr, 40)
    eng = tr.engine
    assert eng.use_graph and eng.g_opt is not None                 # the GA ran from the captured optimizer graph
    assert eng.ga_dev["mut_kind"] == 1 and eng.ga_dev["frozen_or"] == 0
    g = tr.pop.genotypes
    assert np.array_equal(eng.ga_dev["geno"].cpu().numpy(), g.astype(np.uint8))
    assert np.array_equal(eng.ga_dev["slots"].cpu().numpy(), tr.pop.slots.astype(np.int32))
    assert int(eng.ga_dev["gen"]) == tr.pop.generation
    assert np.array_equal(tr.model.mask.cpu().numpy(), g)          # no frozen OR
    assert np.array_equal(eng.ga_dev["frozen"].cpu().numpy(), frozen.astype(np.uint8))   # the real mask is uploaded
    _frozen_params_unchanged(tr, frozen, after_freeze)
    assert 0 < gen1 < tr.pop.generation                            # tournaments fired in both tasks
    assert widest <= N                                             # down cannot grow a path


def test_hip_trainer_or_mode_still_forces_frozen_modules(hip_lib):
    tr = _two_task_trainer("or", "down")
    frozen, after_freeze, gen1, widest, N = _run_two_tasks(tr, 12)
    eng = tr.engine
    assert eng.ga_dev["mut_kind"] == 1 and eng.ga_dev["frozen_or"] == 1
    g = tr.pop.genotypes
    assert np.array_equal(eng.ga_dev["geno"].cpu().numpy(), g.astype(np.uint8))
    want = ((g > 0.5) | (frozen[None] > 0.5)).astype(np.float32)
    assert np.array_equal(tr.model.mask.cpu().numpy(), want)
    assert (want[:, frozen > 0.5] == 1).all()
    _frozen_params_unchanged(tr, frozen, after_freeze)
    assert widest <= N
