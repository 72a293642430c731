"""The episode ledger of the forward-only evaluator: ``algo/evaluate.py ledger_ref`` on hand-written cases (CPU) and
``csrc/heads.hip eval_ledger_kernel`` against it, bit for bit (GPU; the kernel only moves data, so no tolerance).

Rule: entry (t, b) of a chunk counts iff b < nvalid, dones[t, b], cnt[b] < quota and clock + t < max_steps; counted
entries are taken in increasing t, each writes ret[b, cnt[b]] = epret[t, b] and endstep[b, cnt[b]] = clock + t + 1,
then cnt[b] += 1; after the chunk clock += T and pending = #{b < nvalid : cnt[b] < quota}.
"""
import numpy as np
import pytest
import torch

SENT_I = -7


def fresh(B, quota):
    return (np.zeros(B, np.int32), np.full((B, quota), np.nan, np.float32), np.full((B, quota), SENT_I, np.int32))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ----------------------------------------------------------------------------------------------------------- CPU oracle
def test_ledger_ref_quota_reached_mid_chunk_and_second_episode_in_one_chunk():
    from pathnet_gym_amd.algo.evaluate import ledger_ref
    # env 0: episodes end at t = 1, 2 and 4 (quota 2: the third is not counted); env 1: one episode at t = 3
    dones = np.zeros((5, 2), np.uint8)
    dones[[1, 2, 4], 0] = 1
    dones[3, 1] = 1
    epret = np.arange(10, dtype=np.float32).reshape(5, 2) + 0.5
    cnt, ret, end = fresh(2, 2)
    clock, pending = ledger_ref(dones, epret, 2, 2, 10 ** 6, cnt, ret, end, 100)
    assert (clock, pending) == (105, 1)
    assert cnt.tolist() == [2, 1]
    assert ret[0].tolist() == [2.5, 4.5] and end[0].tolist() == [102, 103]
    assert ret[1, 0] == 7.5 and end[1, 0] == 104
    assert np.isnan(ret[1, 1]) and end[1, 1] == SENT_I          # nothing written past cnt


def test_ledger_ref_env_that_never_finishes_stays_pending_and_state_carries():
    from pathnet_gym_amd.algo.evaluate import ledger_ref
    cnt, ret, end = fresh(3, 1)
    clock = 0
    d1 = np.zeros((4, 3), np.uint8)
    d1[2, 0] = 1
    clock, pending = ledger_ref(d1, np.full((4, 3), 3.0, np.float32), 3, 1, 10 ** 6, cnt, ret, end, clock)
    assert (clock, pending) == (4, 2)
    d2 = np.zeros((4, 3), np.uint8)
    d2[0, 0] = 1          # env 0 already holds its quota: ignored
    d2[3, 2] = 1
    clock, pending = ledger_ref(d2, np.full((4, 3), 9.0, np.float32), 3, 1, 10 ** 6, cnt, ret, end, clock)
    assert (clock, pending) == (8, 1)
    assert cnt.tolist() == [1, 0, 1]
    assert ret[0, 0] == 3.0 and end[0, 0] == 3 and ret[2, 0] == 9.0 and end[2, 0] == 8
    assert np.isnan(ret[1, 0]) and end[1, 0] == SENT_I


def test_ledger_ref_max_steps_cuts_inside_a_chunk():
    from pathnet_gym_amd.algo.evaluate import ledger_ref
    dones = np.ones((6, 1), np.uint8)
    epret = np.arange(6, dtype=np.float32).reshape(6, 1)
    cnt, ret, end = fresh(1, 8)
    # clock 10, max_steps 13: steps 10, 11 and 12 (t = 0..2) count, t = 3.. do not
    clock, pending = ledger_ref(dones, epret, 1, 8, 13, cnt, ret, end, 10)
    assert (clock, pending) == (16, 1)
    assert cnt[0] == 3 and ret[0, :3].tolist() == [0.0, 1.0, 2.0] and end[0, :3].tolist() == [11, 12, 13]
    assert np.isnan(ret[0, 3:]).all() and (end[0, 3:] == SENT_I).all()
    # a later chunk lies wholly past max_steps: only the clock moves
    clock, pending = ledger_ref(dones, epret, 1, 8, 13, cnt, ret, end, clock)
    assert (clock, pending, int(cnt[0])) == (22, 1, 3)


def test_ledger_ref_rows_at_and_beyond_nvalid_are_never_touched():
    from pathnet_gym_amd.algo.evaluate import ledger_ref
    dones = np.ones((3, 4), np.uint8)
    epret = np.ones((3, 4), np.float32)
    cnt, ret, end = fresh(4, 2)
    clock, pending = ledger_ref(dones, epret, 2, 2, 10 ** 6, cnt, ret, end, 0)
    assert (clock, pending) == (3, 0)
    assert cnt.tolist() == [2, 2, 0, 0]
    assert np.isnan(ret[2:]).all() and (end[2:] == SENT_I).all()
    clock, pending = ledger_ref(dones, epret, 0, 2, 10 ** 6, cnt, ret, end, clock)          # nvalid 0: nothing pending
    assert (clock, pending) == (6, 0)
    with pytest.raises(ValueError):
        ledger_ref(dones, epret, 5, 2, 10 ** 6, cnt, ret, end, 0)


# --------------------------------------------------------------------------------------------------------------- kernel
def make_case(B, T, quota, seed, shift=0):
    """Chunks of dones / epret in which env b is of kind (b + shift) % 3 over the whole run: 0 never finishes an
    episode, 1 finishes exactly ``quota``, 2 finishes more than ``quota`` (at random steps).  At least three chunks;
    more when three chunks of T steps cannot hold quota + 1 episodes (T = 1, quota = 3)."""
    rng = np.random.RandomState(seed)
    calls = max(3, -(-(quota + 1) // T))
    S = calls * T
    dones = np.zeros((S, B), np.uint8)
    for b in range(B):
        kind = (b + shift) % 3
        k = 0 if kind == 0 else quota if kind == 1 else rng.randint(quota + 1, S + 1)
        dones[rng.choice(S, k, replace=False), b] = 1
    epret = rng.standard_normal((S, B)).astype(np.float32)          # also where no episode ends: must not be copied
    return dones.reshape(calls, T, B), epret.reshape(calls, T, B)


class DeviceLedger:
    def __init__(self, B, T, quota, nvalid, max_steps):
        dev = "cuda"
        self.args = (T, B, nvalid, quota, max_steps)
        cnt, ret, end = fresh(B, quota)
        self.cnt, self.ret, self.end = (torch.from_numpy(x).to(dev) for x in (cnt, ret, end))
        self.clock = torch.zeros(1, dtype=torch.int64, device=dev)
        self.pending = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.dones = torch.zeros(T, B, dtype=torch.uint8, device=dev)
        self.epret = torch.zeros(T, B, dtype=torch.float32, device=dev)

    def feed(self, dones, epret):
        self.dones.copy_(torch.from_numpy(dones))
        self.epret.copy_(torch.from_numpy(epret))

    def launch(self):
        from pathnet_gym_amd.ops import _lib
        T, B, nvalid, quota, max_steps = self.args
        _lib.call("launch_eval_ledger", self.dones.data_ptr(), self.epret.data_ptr(), T, B, nvalid, quota, max_steps,
                  self.cnt.data_ptr(), self.ret.data_ptr(), self.end.data_ptr(), self.clock.data_ptr(),
                  self.pending.data_ptr(), _lib.stream())

    def state(self):
        return (self.cnt.cpu().numpy(), self.ret.cpu().numpy(), self.end.cpu().numpy(), int(self.clock.item()),
                int(self.pending.item()))


def run_against_ref(B, T, quota, seed, shift=0, max_steps=10 ** 6):
    """Every chunk through the kernel and through ledger_ref; all state compared after every call.  -> finished
    episodes per valid env over the whole run (from the inputs, not from the ledger)."""
    from pathnet_gym_amd.algo.evaluate import ledger_ref
    nvalid = B - B // 4
    dones, epret = make_case(B, T, quota, seed, shift)
    dl = DeviceLedger(B, T, quota, nvalid, max_steps)
    cnt, ret, end = fresh(B, quota)
    clock = 0
    for k in range(dones.shape[0]):
        dl.feed(dones[k], epret[k])
        dl.launch()
        clock, pending = ledger_ref(dones[k], epret[k], nvalid, quota, max_steps, cnt, ret, end, clock)
        gc, gr, ge, gclock, gpend = dl.state()
        assert (gclock, gpend) == (clock, pending), (k, gclock, gpend, clock, pending)
        assert np.array_equal(gc, cnt), k
        assert np.array_equal(bits(gr), bits(ret)), k          # NaN sentinels included, bit for bit
        assert np.array_equal(ge, end), k
    # untouched: everything past cnt[b] and every row >= nvalid still holds the sentinels
    for b in range(B):
        n = int(cnt[b]) if b < nvalid else 0
        assert np.isnan(gr[b, n:]).all() and (ge[b, n:] == SENT_I).all(), b
        assert b < nvalid or gc[b] == 0
    return dones.reshape(-1, B).sum(0)[:nvalid]


@pytest.mark.gpu
@pytest.mark.parametrize("quota", [1, 3])
@pytest.mark.parametrize("T", [1, 5, 20])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
def test_ledger_kernel_equals_ledger_ref_bit_for_bit(hip_lib, B, T, quota):
    """Three (or, where T * 3 < quota + 1, more) consecutive calls that carry state.  Each case holds envs that
    finish 0, exactly ``quota`` and more than ``quota`` episodes; with one env (B = 1) the case is run once per kind."""
    kinds = set()
    for shift in (range(3) if B < 4 else (0,)):
        fin = run_against_ref(B, T, quota, seed=1000 * B + 10 * T + quota, shift=shift)
        kinds |= {"none" if f == 0 else "quota" if f == quota else "more" if f > quota else "short" for f in fin}
    assert {"none", "quota", "more"} <= kinds, kinds


@pytest.mark.gpu
def test_ledger_kernel_max_steps_cut_inside_a_chunk(hip_lib):
    """max_steps = 2 T + 2 with every kind of env: the third chunk is cut after two steps."""
    run_against_ref(65, 5, 3, seed=5, max_steps=12)
    run_against_ref(300, 20, 1, seed=6, max_steps=47)


@pytest.mark.gpu
def test_ledger_kernel_captured_graph_replayed_three_times_equals_three_eager_calls(hip_lib):
    B, T, quota = 65, 5, 3
    dones, epret = make_case(B, T, quota, seed=77)
    eager = DeviceLedger(B, T, quota, B - 3, 10 ** 6)
    graph = DeviceLedger(B, T, quota, B - 3, 10 ** 6)
    for k in range(3):
        eager.feed(dones[k], epret[k])
        eager.launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        graph.launch()
    for k in range(3):
        graph.feed(dones[k], epret[k])
        g.replay()
    torch.cuda.synchronize()
    a, b = eager.state(), graph.state()
    assert a[3:] == b[3:] == (15, b[4])
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    assert a[0].max() == quota and a[0].min() == 0


@pytest.mark.gpu
def test_ledger_launcher_refuses_bad_sizes(hip_lib):
    dl = DeviceLedger(4, 2, 2, 4, 100)
    before = dl.state()

    def rc(T=2, B=4, nvalid=4, quota=2):
        from pathnet_gym_amd.ops import _lib
        return hip_lib.launch_eval_ledger(dl.dones.data_ptr(), dl.epret.data_ptr(), T, B, nvalid, quota, 100,
                                          dl.cnt.data_ptr(), dl.ret.data_ptr(), dl.end.data_ptr(),
                                          dl.clock.data_ptr(), dl.pending.data_ptr(), _lib.stream())

    for bad in (dict(T=0), dict(T=-1), dict(B=0), dict(quota=0), dict(quota=-1), dict(nvalid=-1), dict(nvalid=5)):
        assert rc(**bad) == -1, bad
    torch.cuda.synchronize()
    after = dl.state()
    assert after[3:] == before[3:] and np.array_equal(after[0], before[0])
    assert rc(nvalid=0) == 0          # no valid env: the clock moves, nothing is pending
    torch.cuda.synchronize()
    assert dl.state()[3:] == (2, 0)
