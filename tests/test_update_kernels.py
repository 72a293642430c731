"""The last stage of every update, launcher by launcher, against plain float64 with buffers of the test's own:
``launch_rmsprop`` (csrc/optim.hip: clip-by-norm + TF-RMSProp on the fp32 master weights), ``launch_pack_ranges``
(csrc/comm.hip: the gather / scatter around the all-reduce) and the operand copies rebuilt after the step,
``launch_refresh_weights_f16`` and ``launch_refresh_weights_cmajor`` (csrc/optim.hip).

The kernels are called through ``ops/_lib`` on synthetic buffers (no model; the two tests that build a trainer or the
``RMSPropTF`` wrapper say so).  The float64 references are fed the fp32 operands as the kernels read them, and the
hyper-parameters as the kernel receives them through its ``float`` arguments: float32(decay), float32(1) -
float32(decay), float32(lr), ... widened to double.

RMSProp bound (derived, asserted elementwise on w, ms and mom)
--------------------------------------------------------------
u = 2^-23 per arithmetic operation (twice the unit roundoff, so the bound holds with or without fused multiply-adds
and for any summation order); ``sqrtf`` and ``/`` are correctly rounded (``_build.py`` passes no fast-math flag) and
cost u each.  Every bound is first order in u and multiplied by 1.001 for the higher-order terms (the largest relative
term below is ~70 u ~ 1e-5).  For a segment of nb blocks (<= 8192 elements each):

    S  = sum g^2          every term is >= 0, so the error is relative to S and counts the roundings on the longest
                          path of one term: 1 square, <= 32 adds in its thread (8192 / 256), 6 shuffle levels of the
                          wave sum, 2 adds of (r0 + r1) + (r2 + r3) and nb sequential adds over the partials:
                              E_S = (41 + nb) u
    norm = sqrt(S)            E_n = E_S / 2 + u
    scale = clip / max(norm, clip)
                          log-1-Lipschitz in norm on both sides of the threshold, plus the division:
                              E_s = E_n + u         but E_s = 0 where norm (1 + E_n) < clip: the kernel's max() then
                          returns clip itself and clip / clip == 1 exactly (``far below clip``), and E_s = 0 with
                          scale = 0 where S (1 - E_S) exceeds the largest float (the fp32 sum is +inf, clip / inf = 0)
    gi = g scale              E_g = E_s + u         (0 where E_s = 0: g * 1 and g * 0 are exact)
    m  = decay ms + (1 - decay) gi gi = t1 + t2,  both >= 0:
                              B_m = u t1 + (2 E_g + 2 u) t2 + u m                        (absolute)
    r  = sqrt(m + eps)        E_r = (B_m / (m + eps) + u) / 2 + u                        (relative)
    q  = lr gi / r            E_q = E_g + u + E_r + u                                    (relative)
    mo = momentum mom + q     B_mo = u |momentum mom| + E_q |q| + u |mo|                 (absolute)
    w' = w - mo               B_w = B_mo + u |w - mo|                                    (absolute)

At a realistic lr the step is far below ulp(w), so ``mom`` (which IS the step at momentum 0) is the sharp check and
``w`` mostly checks its final rounding; with w0 = 0 the test ties them together exactly (w' == -mom').  Elements the
launch must not touch (frozen segments, the gaps between segments, everything on a skipped step) have bound 0 and are
also compared as int32.  The largest |hip - ref| / bound per output and hyper-parameter triple is recorded under
``update_kernels_f64`` in tests/data/numerics_measured.json (``PATHNET_RECORD_NUMERICS``); the assertion is the bound.

The CPU tests check the bound against a numpy fp32 evaluation in the kernel's own order and show that six wrong
float64 references (a dropped block partial, the global norm, epsilon outside the root, decay off by 2 %, no momentum
term, clip / norm without the max) each exceed it at least eightfold.

Pack / unpack and the 16-bit operand copies are exact and compared as integers; ``hcorr`` (the column sums of the
rounded halves) is within (ceil(KP / 256) + 8) 2^-24 sum |h| of float64.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import numerics_budget as budget
from pathnet_gym_amd.config import preset
from pathnet_gym_amd.models.pathnet import ParamLayout
from pathnet_gym_amd.parallel.comm import active_union, union_ranges

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -23
SLACK = 1.001
BLK = 8192
PAD = 64
SENT = -3.0
NAN = float("nan")
CLIP = 40.0
LR = 7e-4
FLT_MAX = float(np.finfo(np.float32).max)
HYPERS = [(0.0, 0.99, 0.1), (0.9, 0.99, 0.1), (0.9, 0.9, 1e-10)]          # (momentum, decay, eps)
HYPER_IDS = ["shipped", "mom0.9", "mom0.9-decay0.9-eps1e-10"]
OUTS = ("w", "ms", "mom")

# segment lengths and what the gradient of each is scaled to (norm relative to clip)
SEGMENTS = [
    (1, "frozen"),                   # a one-element frozen segment
    (255, "small"),                  # far below clip: scale == 1 exactly
    (256, "below"),                  # 0.995 clip
    (257, "above"),                  # 1.005 clip
    (BLK - 1, "x10"),
    (BLK, "below"),                  # ends exactly at the block edge
    (BLK + 1, "above"),              # a one-element tail block that holds 15 % of the square sum
    (2 * BLK, "frozen"),             # multi-block and frozen
    (3 * BLK + 5, "x20"),            # 4 blocks
    (20 * BLK + 17, "x10"),          # 21 blocks: the sequential sum over the partials
    (1, "clip1"),                    # one element of 40.0: norm == clip
    (5, "clip4"),                    # four elements of 20.0 and a zero: norm == clip
    (300, "zero"),                   # trainable, all-zero gradient: ms decays, w moves by momentum * mom only
    (BLK + 3, "small"),              # two blocks, far below clip
]
FACTOR = {"below": 0.995, "above": 1.005, "x10": 10.0, "x20": 20.0}
I_X20, I_SMALL2, I_FROZEN1, I_FROZEN2 = 8, 13, 0, 7


# ---------------------------------------------------------------------------------------------------------------
# layouts, block tables, inputs (numpy; shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------------------------------------------
def make_layout(lens=tuple(n for n, _ in SEGMENTS), first=37):
    """Segments at irregular offsets with gaps of 3 .. 25 elements that no block covers, and PAD elements after."""
    off, segs = first, []
    for i, n in enumerate(lens):
        segs.append((off, n))
        off += n + 3 + (7 * i) % 23
    return dict(segs=segs, numel=off + PAD)


def block_tables(segs):
    seg, beg, end, blk0 = [], [], [], []
    for i, (o, n) in enumerate(segs):
        blk0.append(len(seg))
        for b in range(o, o + n, BLK):
            seg.append(i)
            beg.append(b)
            end.append(min(b + BLK, o + n))
    blk0.append(len(seg))
    return dict(seg=np.array(seg, np.int32), beg=np.array(beg, np.int64), end=np.array(end, np.int64),
                blk0=np.array(blk0, np.int32))


def check_partition(segs, tab):
    """The blocks partition every segment, in order, in pieces <= 8192, and nothing lies outside a segment."""
    seg, beg, end, blk0 = (np.asarray(tab[k]).astype(np.int64) for k in ("seg", "beg", "end", "blk0"))
    assert len(blk0) == len(segs) + 1 and blk0[0] == 0 and blk0[-1] == len(seg) == len(beg) == len(end)
    assert bool((np.diff(blk0) >= 1).all()) and bool((np.diff(seg) >= 0).all())
    for i, (o, n) in enumerate(segs):
        b0, b1 = blk0[i], blk0[i + 1]
        assert b1 - b0 == -(-n // BLK) and bool((seg[b0:b1] == i).all())
        assert beg[b0] == o and end[b1 - 1] == o + n
        assert bool((beg[b0 + 1:b1] == end[b0:b1 - 1]).all())
        ln = end[b0:b1] - beg[b0:b1]
        assert bool((ln >= 1).all()) and bool((ln <= BLK).all()) and bool((ln[:-1] == BLK).all())


def seg_mask(lay, which=None):
    m = np.zeros(lay["numel"], bool)
    for i, (o, n) in enumerate(lay["segs"]):
        if which is None or which[i]:
            m[o:o + n] = True
    return m


def make_grad(role, n, rng):
    if role == "zero":
        return np.zeros(n, np.float32)
    if role == "clip1":
        return np.full(1, 40.0, np.float32)
    if role == "clip4":
        return np.array([20.0, 20.0, 0.0, 20.0, 20.0], np.float32)
    x = rng.standard_normal(n)
    if role == "small":
        return (0.01 * x).astype(np.float32)
    if role == "frozen":
        return (3.0 * x).astype(np.float32)
    tail = n % BLK if n > BLK else 0
    if tail:                                     # 15 % of the square sum in the last, short block
        x[:-tail] *= math.sqrt(0.85) / np.linalg.norm(x[:-tail])
        x[-tail:] *= math.sqrt(0.15) / np.linalg.norm(x[-tail:])
    else:
        x /= np.linalg.norm(x)
    return (x * FACTOR[role] * CLIP).astype(np.float32)


def make_state(lay, seed, roles=tuple(r for _, r in SEGMENTS), w_zero=False):
    """fp32 w / ms / mom with a sentinel in the gaps, g with NaN in the gaps; -> (state, trainable)."""
    rng = np.random.default_rng(seed)
    N = lay["numel"]
    st = dict(w=np.full(N, SENT, np.float32), ms=np.full(N, SENT, np.float32), mom=np.full(N, SENT, np.float32),
              g=np.full(N, NAN, np.float32))
    for (o, n), role in zip(lay["segs"], roles):
        st["w"][o:o + n] = 0.0 if w_zero else (0.1 * rng.standard_normal(n)).astype(np.float32)
        ms = 10.0 ** rng.uniform(-6.0, 2.0, n)
        ms[rng.random(n) < 0.05] = 0.0
        st["ms"][o:o + n] = ms.astype(np.float32)
        mom = (1e-3 * rng.standard_normal(n)).astype(np.float32)
        mom[mom == 0] = 1e-3
        st["mom"][o:o + n] = mom
        st["g"][o:o + n] = make_grad(role, n, rng)
    return st, np.array([r != "frozen" for r in roles], bool)


def f32(x):
    return np.float64(np.float32(x))


def ref_rmsprop(lay, st, trainable, lr, hyper, clip=CLIP, skip=False, mutate=None):
    """float64 reference of one launch and the elementwise bounds of the module docstring.
    -> dict(w, ms, mom, w_bound, ms_bound, mom_bound, flag).  ``mutate`` names one of the wrong references of the
    negative controls."""
    mu, d, eps = (f32(x) for x in hyper)
    omd = np.float64(np.float32(1) - np.float32(hyper[1]))
    lr, clip = f32(lr), f32(clip)
    out = {k: st[k].astype(np.float64) for k in OUTS}
    out.update({k + "_bound": np.zeros(lay["numel"]) for k in OUTS})
    g = st["g"]
    out["flag"] = float(any(not np.isfinite(g[o:o + n]).all() for (o, n), t in zip(lay["segs"], trainable) if t))
    if out["flag"] or skip:
        return out
    if mutate == "decay_off":
        d = d * 1.02
    S_all = sum(float((g[o:o + n].astype(np.float64) ** 2).sum()) for (o, n), t in zip(lay["segs"], trainable) if t)
    for (o, n), t in zip(lay["segs"], trainable):
        if not t:
            continue
        sl = slice(o, o + n)
        g64, w, ms, mom = g[sl].astype(np.float64), out["w"][sl], out["ms"][sl], out["mom"][sl]
        nb = -(-n // BLK)
        S = float((g64 ** 2).sum())
        if mutate == "drop_last_block" and nb > 1:
            S -= float((g64[(nb - 1) * BLK:] ** 2).sum())
        if mutate == "global_norm":
            S = S_all
        E_S = (41 + nb) * U
        norm = math.sqrt(S)
        E_n = E_S / 2 + U
        if S * (1 - E_S) > FLT_MAX:
            scale, E_s = 0.0, 0.0
        elif norm * (1 + E_n) < clip:
            scale, E_s = 1.0, 0.0
        else:
            assert S * (1 + E_S) < FLT_MAX, "square sum too close to the fp32 overflow threshold to call"
            scale, E_s = clip / max(norm, clip), E_n + U
        if mutate == "no_max" and norm > 0:
            scale = clip / norm
        E_g = E_s + U if E_s else 0.0
        gi = g64 * scale
        t1, t2 = d * ms, omd * gi * gi
        m = t1 + t2
        B_m = U * t1 + (2 * E_g + 2 * U) * t2 + U * m
        r = np.sqrt(m) + eps if mutate == "eps_outside" else np.sqrt(m + eps)
        E_r = (B_m / (m + eps) + U) / 2 + U
        q = lr * gi / r
        E_q = E_g + U + E_r + U
        mm = 0.0 * mom if mutate == "no_momentum" else mu * mom
        mo = mm + q
        B_mo = U * np.abs(mm) + E_q * np.abs(q) + U * np.abs(mo)
        wn = w - mo
        out["ms"][sl], out["mom"][sl], out["w"][sl] = m, mo, wn
        out["ms_bound"][sl], out["mom_bound"][sl] = SLACK * B_m, SLACK * B_mo
        out["w_bound"][sl] = SLACK * (B_mo + U * np.abs(wn))
    return out


def emulate_fp32(lay, st, trainable, lr, hyper, clip=CLIP):
    """numpy fp32, one rounding per operation, in the kernels' order: 256 strided per-thread sums, the xor-shuffle
    tree over 64 lanes, (r0 + r1) + (r2 + r3), the sequential sum over a segment's partials, then the apply."""
    F = np.float32
    mu, d, eps, lr, clip = F(hyper[0]), F(hyper[1]), F(hyper[2]), F(lr), F(clip)
    omd = F(1) - d
    tab = block_tables(lay["segs"])
    nblk = len(tab["seg"])
    X = np.zeros((nblk, BLK), F)
    for b in range(nblk):
        X[b, :tab["end"][b] - tab["beg"][b]] = st["g"][tab["beg"][b]:tab["end"][b]]
    X = X.reshape(nblk, BLK // 256, 256)
    s = np.zeros((nblk, 256), F)
    for k in range(BLK // 256):
        s = s + X[:, k] * X[:, k]
    s = s.reshape(nblk, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ o]
    red = s[:, :, 0]
    partial = (red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3])
    out = {k: st[k].copy() for k in OUTS}
    for i, (o, n) in enumerate(lay["segs"]):
        if not trainable[i]:
            continue
        S = F(0)
        for b in range(tab["blk0"][i], tab["blk0"][i + 1]):
            S = S + partial[b]
        scale = clip / np.maximum(np.sqrt(S), clip)
        sl = slice(o, o + n)
        gi = st["g"][sl] * scale
        m = d * st["ms"][sl] + (omd * gi) * gi
        mo = mu * st["mom"][sl] + (lr * gi) / np.sqrt(m + eps)
        out["ms"][sl], out["mom"][sl], out["w"][sl] = m, mo, st["w"][sl] - mo
        assert m.dtype == mo.dtype == out["w"].dtype == F
    return out


def ratios(got, ref):
    """max |got - ref| / bound per output (inf where a bound of 0 is missed)."""
    out = {}
    for k in OUTS:
        err, bound = np.abs(got[k].astype(np.float64) - ref[k]), ref[k + "_bound"]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        out[k] = float(np.nanmax(r)) if np.isfinite(got[k]).all() else float("inf")
    return out


def record_measured(vals):
    """PATHNET_RECORD_NUMERICS=<file>: keep the max per key under update_kernels_f64."""
    rec = os.environ.get("PATHNET_RECORD_NUMERICS")
    if not rec:
        return
    d = budget._load(rec)
    t = d.setdefault("update_kernels_f64", {})
    for k, v in vals.items():
        t[k] = max(float(v), float(t.get(k, 0.0)))
    os.makedirs(os.path.dirname(rec) or ".", exist_ok=True)
    with open(rec, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def within(tag, got, ref, key=None):
    r = ratios(got, ref)
    print(f"{tag}: worst err / bound: " + ", ".join(f"{k} = {v:.4f}" for k, v in r.items()))
    if key:
        record_measured({f"rmsprop.{key}.{k}": v for k, v in r.items() if np.isfinite(v)})
    assert all(v <= 1.0 for v in r.values()), (tag, r)
    return r


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in OUTS)


# ---------------------------------------------------------------------------------------------------------------
# CPU: the layout, the bound against the ordered fp32 emulation, the negative controls
# ---------------------------------------------------------------------------------------------------------------
def test_layout_and_inputs_cover_the_intended_cases_cpu():
    lay = make_layout()
    st, tr = make_state(lay, seed=1)
    tab = block_tables(lay["segs"])
    check_partition(lay["segs"], tab)
    assert [n for _, n in lay["segs"]] == [1, 255, 256, 257, 8191, 8192, 8193, 16384, 3 * 8192 + 5, 20 * 8192 + 17,
                                           1, 5, 300, 8195]
    assert len(tab["seg"]) == 40 and lay["numel"] < 2_200_000
    inside = seg_mask(lay)
    assert bool(np.isnan(st["g"][~inside]).all()) and bool(np.isfinite(st["g"][inside]).all())
    assert all(bool((st[k][~inside] == SENT).all()) for k in OUTS)
    prev = 0
    for o, n in lay["segs"]:
        assert o - prev >= 3                                 # a gap before every segment
        prev = o + n
    assert bool((st["ms"][inside] >= 0).all()) and bool((st["ms"][inside] == 0).any())
    pos = st["ms"][inside][st["ms"][inside] > 0]
    assert pos.min() < 1e-5 and pos.max() > 10 and bool((st["mom"][inside] != 0).all())
    assert not tr[I_FROZEN1] and not tr[I_FROZEN2] and lay["segs"][I_FROZEN1][1] == 1 \
        and lay["segs"][I_FROZEN2][1] > BLK and tr.sum() == len(tr) - 2
    seen = set()
    for (o, n), (_, role) in zip(lay["segs"], SEGMENTS):
        g64 = st["g"][o:o + n].astype(np.float64)
        norm = math.sqrt((g64 ** 2).sum())
        seen.add(role)
        if role == "small":
            assert norm < 0.05 * CLIP
        elif role == "below":
            assert 0.99 * CLIP < norm < CLIP * (1 - 1e-4)
        elif role == "above":
            assert CLIP * (1 + 1e-4) < norm < 1.01 * CLIP
        elif role in ("x10", "x20"):
            assert abs(norm / (FACTOR[role] * CLIP) - 1) < 1e-6
        elif role in ("clip1", "clip4"):
            assert norm == CLIP and np.float32((st["g"][o:o + n] ** 2).sum()) == 1600.0
        elif role == "zero":
            assert norm == 0
        if role in FACTOR and n > BLK:                       # a sum that drops the last block is visible
            assert (g64[n - n % BLK:] ** 2).sum() >= 0.10 * (g64 ** 2).sum()
    assert seen == {"frozen", "small", "below", "above", "x10", "x20", "clip1", "clip4", "zero"}


@pytest.mark.parametrize("hyper", HYPERS, ids=HYPER_IDS)
def test_bound_holds_for_the_ordered_fp32_emulation_cpu(hyper):
    lay = make_layout()
    for seed, kw in ((1, {}), (2, dict(w_zero=True))):
        st, tr = make_state(lay, seed=seed, **kw)
        ref = ref_rmsprop(lay, st, tr, LR, hyper)
        emu = emulate_fp32(lay, st, tr, LR, hyper)
        r = ratios(emu, ref)
        print(f"fp32 emulation {hyper} seed {seed}: {r}")
        assert all(v <= 1.0 for v in r.values()), r
        untouched = ~seg_mask(lay, tr)
        assert all(np.array_equal(bits(emu[k])[untouched], bits(st[k])[untouched]) for k in OUTS)
        assert float(ref["flag"]) == 0.0
        # a bound is 0 only where the value is exact: untouched elements, and exact zeros
        moved = seg_mask(lay, tr)
        assert all(bool((ref[k + "_bound"][moved] > 0)[ref[k][moved] != 0].all()) for k in OUTS)
        assert all(bool((ref[k + "_bound"][untouched] == 0).all()) for k in OUTS)
        if kw:
            assert np.array_equal(emu["w"][moved], -emu["mom"][moved])


NEGATIVE_CONTROLS = [("drop_last_block", HYPERS[0]), ("global_norm", HYPERS[0]), ("eps_outside", HYPERS[0]),
                     ("decay_off", HYPERS[0]), ("no_momentum", HYPERS[1]), ("no_max", HYPERS[0])]


@pytest.mark.parametrize("mutation,hyper", NEGATIVE_CONTROLS, ids=[m for m, _ in NEGATIVE_CONTROLS])
def test_wrong_references_exceed_the_bound_eightfold_cpu(mutation, hyper):
    lay = make_layout()
    st, tr = make_state(lay, seed=1)
    ref = ref_rmsprop(lay, st, tr, LR, hyper)
    bad = ref_rmsprop(lay, st, tr, LR, hyper, mutate=mutation)
    r = ratios({k: bad[k] for k in OUTS}, ref)
    print(f"{mutation}: err / bound = {r}")
    assert max(r.values()) >= 8.0, (mutation, r)


# ---------------------------------------------------------------------------------------------------------------
# GPU plumbing for launch_rmsprop
# ---------------------------------------------------------------------------------------------------------------
class DevState:
    """Device copies of a state, its block tables and the launch scratch (partial and status carry sentinels)."""

    def __init__(self, lay, st, trainable):
        tab = block_tables(lay["segs"])
        self.lay, self.nblk = lay, len(tab["seg"])
        self.t = {k: torch.from_numpy(st[k].copy()).to(DEV) for k in ("w", "g", "ms", "mom")}
        self.seg, self.beg, self.end, self.blk0 = (torch.from_numpy(tab[k]).to(DEV)
                                                   for k in ("seg", "beg", "end", "blk0"))
        self.trainable = torch.from_numpy(np.asarray(trainable, np.uint8)).to(DEV)
        self.partial = torch.full((self.nblk + 1 + PAD,), SENT, device=DEV)
        self.status = torch.full((1 + PAD,), SENT, device=DEV)
        self.lr = torch.zeros(2, device=DEV)

    def load(self, st):
        for k in ("w", "g", "ms", "mom"):
            if k in st:
                self.t[k].copy_(torch.from_numpy(st[k]))

    def args(self, hyper, clip=CLIP, status=True, nblk=None):
        from pathnet_gym_amd.ops import _lib
        mu, d, eps = hyper
        return (self.t["w"].data_ptr(), self.t["g"].data_ptr(), self.t["ms"].data_ptr(), self.t["mom"].data_ptr(),
                self.seg.data_ptr(), self.beg.data_ptr(), self.end.data_ptr(), self.nblk if nblk is None else nblk,
                self.partial.data_ptr(), self.blk0.data_ptr(), self.trainable.data_ptr(), self.lr.data_ptr(),
                self.status.data_ptr() if status else None, d, mu, eps, clip, _lib.stream())

    def launch(self, lr, hyper, skip=0.0, **kw):
        from pathnet_gym_amd.ops import _lib
        self.lr.copy_(torch.tensor([lr, skip]))
        _lib.call("launch_rmsprop", *self.args(hyper, **kw))
        torch.cuda.synchronize()
        return self.fetch()

    def fetch(self):
        out = {k: self.t[k].cpu().numpy() for k in OUTS}
        partial, status = self.partial.cpu().numpy(), self.status.cpu().numpy()
        assert bool((partial[self.nblk + 1:] == SENT).all()) and bool((status[1:] == SENT).all())
        out["status"], out["flag"], out["partial"] = float(status[0]), float(partial[self.nblk]), partial[:self.nblk]
        return out


def check_launch(lay, st, tr, lr, hyper, tag, key=None, dev=None):
    """One launch from ``st``: status clear, every output within its bound, everything else bit-intact."""
    dev = dev or DevState(lay, st, tr)
    dev.load(st)
    got = dev.launch(lr, hyper)
    ref = ref_rmsprop(lay, st, tr, lr, hyper)
    assert got["status"] == 0.0 and got["flag"] == 0.0, tag
    within(tag, got, ref, key)
    untouched = ~seg_mask(lay, tr)
    assert all(np.array_equal(bits(got[k])[untouched], bits(st[k])[untouched]) for k in OUTS), tag
    return got, ref, dev


# ---------------------------------------------------------------------------------------------------------------
# 1. launch_rmsprop
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hyper", HYPERS, ids=HYPER_IDS)
def test_rmsprop_matches_float64(hip_lib, hyper):
    """Every segment role of SEGMENTS at once; the same launch from the same state again gives the same bits."""
    lay = make_layout()
    st, tr = make_state(lay, seed=1)
    got, _, dev = check_launch(lay, st, tr, LR, hyper, f"rmsprop {hyper}", key=HYPER_IDS[HYPERS.index(hyper)])
    assert same_bits(check_launch(lay, st, tr, LR, hyper, "again", dev=dev)[0], got)
    for i, (o, n) in enumerate(lay["segs"]):
        sl = slice(o, o + n)
        if tr[i] and n > 1:                                  # the step is not vacuous
            assert float((got["ms"][sl] != st["ms"][sl])[st["ms"][sl] > 0].mean()) > 0.99
        if SEGMENTS[i][1] == "zero":                         # exact: ms decays, w moves by momentum * mom alone
            d32, mu32 = np.float32(hyper[1]), np.float32(hyper[0])
            assert np.array_equal(got["ms"][sl], d32 * st["ms"][sl])
            assert np.array_equal(got["mom"][sl], mu32 * st["mom"][sl])
            assert np.array_equal(got["w"][sl], st["w"][sl] - got["mom"][sl])


@gpu
@pytest.mark.parametrize("hyper", HYPERS, ids=HYPER_IDS)
def test_rmsprop_zero_lr_and_zero_weights(hip_lib, hyper):
    lay = make_layout()
    st, tr = make_state(lay, seed=3)
    moved = seg_mask(lay, tr)
    got, _, dev = check_launch(lay, st, tr, 0.0, hyper, f"lr=0 {hyper}")
    assert np.array_equal(got["mom"][moved], np.float32(hyper[0]) * st["mom"][moved])      # the step term is +-0
    st0, _ = make_state(lay, seed=4, w_zero=True)
    got, _, _ = check_launch(lay, st0, tr, LR, hyper, f"w0=0 {hyper}", key=HYPER_IDS[HYPERS.index(hyper)], dev=dev)
    assert np.array_equal(got["w"][moved], -got["mom"][moved]) and bool((got["mom"][moved] != 0).any())


def plant_sites(lay, i):
    """(first element, last element of the tail block, an element only a lane of waves 1..3 reads) of segment i."""
    o, n = lay["segs"][i]
    site = o + BLK + 3 * 256 + 130
    assert n > 2 * BLK and n % BLK and (site - (o + BLK)) % 256 >= 64
    return dict(first=o, tail_last=o + n - 1, wave2=site)


@gpu
@pytest.mark.parametrize("where", ["first", "tail_last", "wave2"])
@pytest.mark.parametrize("value", [NAN, float("inf"), float("-inf")], ids=["nan", "+inf", "-inf"])
def test_rmsprop_nonfinite_gradient_skips_the_step_and_flags_it(hip_lib, value, where):
    lay = make_layout()
    st, tr = make_state(lay, seed=5)
    hyper = HYPERS[1]
    dev = DevState(lay, st, tr)
    bad = dict(st, g=st["g"].copy())
    bad["g"][plant_sites(lay, I_X20)[where]] = value
    dev.load(bad)
    got = dev.launch(LR, hyper)
    assert got["status"] == 1.0 and got["flag"] == 1.0
    assert same_bits(got, st)
    blk = int(np.searchsorted(block_tables(lay["segs"])["beg"], plant_sites(lay, I_X20)[where], side="right")) - 1
    assert np.isnan(got["partial"][blk]) and int(np.isnan(got["partial"]).sum()) == 1
    # not sticky: a clean launch right after steps normally
    check_launch(lay, st, tr, LR, hyper, f"after {value} at {where}", dev=dev)


@gpu
def test_rmsprop_nonfinite_gradient_in_frozen_segments_only(hip_lib):
    lay = make_layout()
    st, tr = make_state(lay, seed=6)
    o1, _ = lay["segs"][I_FROZEN1]
    o2, n2 = lay["segs"][I_FROZEN2]
    st["g"][o1] = NAN
    st["g"][o2], st["g"][o2 + BLK + 200], st["g"][o2 + n2 - 1] = float("inf"), NAN, float("-inf")
    for hyper in (HYPERS[0], HYPERS[1]):
        got, _, _ = check_launch(lay, st, tr, LR, hyper, f"frozen non-finite {hyper}")     # status 0, bounds, frozen
        assert int(np.isnan(got["partial"]).sum()) == 3                                   # bits: all in check_launch


@gpu
def test_rmsprop_finite_gradient_whose_square_sum_overflows(hip_lib):
    """64 entries of 1e30 in a trainable two-block segment: not flagged; that segment gets exactly what scale = 0
    gives (tf.clip_by_norm's t * clip / max(inf, clip)), every other segment steps within its bound."""
    lay = make_layout()
    st, tr = make_state(lay, seed=7)
    o, n = lay["segs"][I_SMALL2]
    st["g"][o + 100:o + 164] = 1e30
    for hyper in HYPERS:
        got, _, _ = check_launch(lay, st, tr, LR, hyper, f"overflow {hyper}")
        sl = slice(o, o + n)
        assert np.isinf(got["partial"][block_tables(lay["segs"])["blk0"][I_SMALL2]])
        assert all(np.isfinite(got[k][sl]).all() for k in OUTS)
        assert np.array_equal(got["ms"][sl], np.float32(hyper[1]) * st["ms"][sl])
        assert np.array_equal(got["mom"][sl], np.float32(hyper[0]) * st["mom"][sl])
        assert np.array_equal(got["w"][sl], st["w"][sl] - got["mom"][sl])


@gpu
def test_rmsprop_host_skip_and_null_status(hip_lib):
    lay = make_layout()
    st, tr = make_state(lay, seed=8)
    hyper = HYPERS[1]
    dev = DevState(lay, st, tr)
    got = dev.launch(LR, hyper, skip=1.0)                    # lr_ptr[1] = 1: nothing changes, status says "finite"
    assert same_bits(got, st) and got["status"] == 0.0 and got["flag"] == 0.0
    bad = dict(st, g=st["g"].copy())
    bad["g"][lay["segs"][1][0] + 7] = NAN
    dev.load(bad)
    got = dev.launch(LR, hyper, skip=1.0)                    # ... and still reports the gradient
    assert same_bits(got, st) and got["status"] == 1.0 and got["flag"] == 1.0
    dev.load(st)
    want = dev.launch(LR, hyper)
    assert want["status"] == 0.0 and not same_bits(want, st)
    dev.load(st)
    dev.status.fill_(SENT)
    got = dev.launch(LR, hyper, status=False)                # status == NULL is accepted
    assert same_bits(got, want) and got["status"] == SENT and got["flag"] == 0.0


@gpu
def test_rmsprop_three_steps_carry_the_state(hip_lib):
    """Three launches with different gradients on the same device buffers; the float64 reference is re-seeded from
    the kernel's own fp32 state before each, so the bound stays a one-step bound."""
    lay = make_layout()
    st, tr = make_state(lay, seed=9)
    hyper = HYPERS[1]
    dev = DevState(lay, st, tr)
    for step in range(3):
        st["g"] = make_state(lay, seed=20 + step)[0]["g"]
        dev.load(dict(g=st["g"]))
        got = dev.launch(LR, hyper)
        within(f"step {step}", got, ref_rmsprop(lay, st, tr, LR, hyper))
        assert got["status"] == 0.0 and not same_bits(got, st)
        for k in OUTS:
            st[k] = got[k]


@gpu
def test_rmsprop_graph_replay_equals_eager(hip_lib):
    """The three-kernel chain captured once and replayed twice == two eager launches (the path the engine ships)."""
    from pathnet_gym_amd.ops import _lib
    lay = make_layout()
    st, tr = make_state(lay, seed=10)
    hyper = HYPERS[1]
    dev = DevState(lay, st, tr)
    first = dev.launch(LR, hyper)
    eager = dev.launch(LR, hyper)
    assert eager["status"] == 0.0
    dev.load(st)
    dev.partial.fill_(SENT)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _lib.call("launch_rmsprop", *dev.args(hyper))
    torch.cuda.synchronize()
    dev.load(st)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    got = dev.fetch()
    assert same_bits(got, eager) and got["status"] == 0.0
    assert np.array_equal(bits(got["partial"]), bits(eager["partial"]))
    within("second replay", got, ref_rmsprop(lay, dict(g=st["g"], **{k: first[k] for k in OUTS}), tr, LR, hyper))


@gpu
def test_rmsprop_launcher_contract(hip_lib):
    lay = make_layout()
    st, tr = make_state(lay, seed=11)
    dev = DevState(lay, st, tr)
    dev.lr.copy_(torch.tensor([LR, 0.0]))
    assert hip_lib.launch_rmsprop(*dev.args(HYPERS[0], nblk=-1)) == -22
    assert hip_lib.launch_rmsprop(*dev.args(HYPERS[0], nblk=-40)) == -22
    assert hip_lib.launch_rmsprop(*dev.args(HYPERS[0], nblk=0)) == -1
    torch.cuda.synchronize()
    got = dev.fetch()
    assert same_bits(got, st) and got["status"] == SENT and bool((dev.partial == SENT).all())


@gpu
@pytest.mark.parametrize("name", ["pong", "cartpole", "reference"])
def test_engine_block_tables(hip_lib, name):
    """The tables the engine and the standalone wrapper build for a real layout (the one test here with a trainer;
    4 paths x 16 envs is the smallest population the suite builds)."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.ops.optim import _tables
    cfg = preset(name)
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 4, 16, 2
    cfg.ga.B = min(cfg.ga.B, 3)
    tr = PathNetTrainer(cfg, device=DEV)
    eng, segs = tr.engine, [(s.offset, s.numel) for s in tr.model.store.layout.segments]
    own, wrap = block_tables(segs), _tables(tr.opt)
    mine = dict(seg=eng.blk_seg, beg=eng.blk_beg, end=eng.blk_end, blk0=eng.seg_blk0)
    for k, dt in (("seg", torch.int32), ("beg", torch.int64), ("end", torch.int64), ("blk0", torch.int32)):
        assert mine[k].dtype == wrap[k].dtype == dt and mine[k].is_contiguous()
        assert np.array_equal(mine[k].cpu().numpy(), own[k]) and torch.equal(mine[k], wrap[k]), (name, k)
    assert eng.nblk == len(own["seg"]) and eng.partial.numel() == wrap["partial"].numel() == eng.nblk + 1
    check_partition(segs, {k: v.cpu().numpy() for k, v in mine.items()})
    covered = np.zeros(tr.model.store.layout.numel, np.int32)
    for b, e in zip(own["beg"], own["end"]):
        covered[b:e] += 1
    assert bool((covered == 1).all())                        # the layout has no gaps: every parameter in one block
    assert eng.trainable_u8.numel() == len(segs)


@gpu
def test_rmsprop_wrapper_on_the_cartpole_layout(hip_lib):
    """``RMSPropTF(backend='hip').step`` with two frozen modules and momentum 0.9, three steps."""
    from pathnet_gym_amd.algo.optim import RMSPropTF
    net = preset("cartpole").net
    layout = ParamLayout(net)
    lay = dict(segs=[(s.offset, s.numel) for s in layout.segments], numel=layout.numel)
    rng = np.random.default_rng(12)
    flat = torch.from_numpy((0.1 * rng.standard_normal(layout.numel)).astype(np.float32)).to(DEV)
    hyper = (0.9, 0.99, 0.1)
    opt = RMSPropTF(layout, flat, decay=hyper[1], momentum=hyper[0], epsilon=hyper[2], clip_norm=CLIP, backend="hip")
    frozen = np.zeros((net.L, net.M), np.float32)
    frozen[0, 1] = frozen[1, 2] = 1
    opt.set_frozen(frozen)
    tr = opt.seg_trainable.cpu().numpy()
    assert (~tr).sum() == 4
    opt.ms.copy_(torch.from_numpy((10.0 ** rng.uniform(-4, 1, layout.numel)).astype(np.float32)))
    opt.mom.copy_(torch.from_numpy((1e-3 * rng.standard_normal(layout.numel)).astype(np.float32)))
    clipped = 0
    for step in range(3):
        g = (3.0 * rng.standard_normal(layout.numel)).astype(np.float32)
        st = dict(w=flat.cpu().numpy(), ms=opt.ms.cpu().numpy(), mom=opt.mom.cpu().numpy(), g=g)
        ref = ref_rmsprop(lay, st, tr, LR, hyper)
        clipped += sum(np.linalg.norm(g[o:o + n].astype(np.float64)) > CLIP for o, n in lay["segs"])
        opt.step(torch.from_numpy(g).to(DEV), LR)
        torch.cuda.synchronize()
        got = dict(w=flat.cpu().numpy(), ms=opt.ms.cpu().numpy(), mom=opt.mom.cpu().numpy())
        within(f"wrapper step {step}", got, ref, key="wrapper")
        frozen_el = ~seg_mask(lay, tr)
        assert frozen_el.any() and all(np.array_equal(bits(got[k])[frozen_el], bits(st[k])[frozen_el]) for k in OUTS)
        assert not np.array_equal(got["w"], st["w"]) and float(opt._hip_tables["status"]) == 0.0
    assert clipped >= 3                                      # segments on both sides of the threshold


# ---------------------------------------------------------------------------------------------------------------
# 2. launch_pack_ranges
# ---------------------------------------------------------------------------------------------------------------
def make_table(lens, gaps, order=None):
    """Source ranges laid out with ``gaps[i]`` elements before range i; table rows (src_off, len, dst_off) in
    ``order`` (default: source order) with contiguous ascending dst offsets.  -> table [nr, 3], index [n], flat size."""
    src, o = [], 0
    for ln, gp in zip(lens, gaps):
        o += gp
        src.append(o)
        o += ln
    order = list(range(len(lens))) if order is None else list(order)
    tab, d = np.zeros((len(lens), 3), np.int64), 0
    for r, i in enumerate(order):
        tab[r] = (src[i], lens[i], d)
        d += lens[i]
    index = np.concatenate([np.arange(s, s + ln, dtype=np.int64) for s, ln, _ in tab])
    return tab, index, o + 9


def random_table(nr, seed, permute=False):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 40, nr)
    gaps = rng.integers(0, 6, nr)
    lens[nr // 2] = lens[nr // 2 + 1] = lens[-1] = 1         # adjacent length-1 ranges, and a last range of length 1
    gaps[0], gaps[nr // 2], gaps[nr // 2 + 1] = 2, 1, 0
    lens[3] = 777                                            # several workgroups inside one range
    return make_table(lens.tolist(), gaps.tolist(), rng.permutation(nr) if permute else None)


# union_ranges sorts its ranges and numbers the packed offsets in that order, so source order == destination
# order in every table the project builds; the kernel searches dst_off alone, and "permuted" holds it to that.
PACK_CASES = {
    "nr1": lambda: make_table([1], [5]),
    "nr2": lambda: make_table([1, 1], [4, 0]),
    "nr3": lambda: make_table([7, 1, 300], [3, 2, 1]),
    "nr50": lambda: random_table(50, seed=50),
    "nr51": lambda: random_table(51, seed=51),
    "permuted": lambda: random_table(50, seed=52, permute=True),
    "grid_stride": lambda: make_table([1_000_000, 300, 1_097_152], [11, 1, 7]),      # n = 8192 * 256 + 300
    "zero_length": lambda: make_table([5, 0, 9, 1, 0], [2, 3, 4, 0, 6]),             # one inside, one as the last row
}
NAN_BITS, SENT_BITS = 0x7FC00001, int(np.float32(SENT).view(np.int32))


def test_pack_tables_cpu():
    for name, mk in PACK_CASES.items():
        tab, index, size = mk()
        n = int(tab[:, 1].sum())
        assert len(index) == n == len(np.unique(index)) and index.max() < size - 8, name
        assert tab[0, 2] == 0 and np.array_equal(tab[1:, 2], np.cumsum(tab[:-1, 1])), name
        srt = tab[np.argsort(tab[:, 0], kind="stable")]
        assert bool((srt[:-1, 0] + srt[:-1, 1] <= srt[1:, 0]).all()), name                  # disjoint sources
        assert (name == "permuted") == (not bool((np.diff(tab[:, 0]) >= 0).all())), name
        # the kernel's search, ``last row whose dst_off <= i``, written out: it lands in the row that holds i
        rows = np.searchsorted(tab[:, 2], np.arange(n), side="right") - 1
        assert np.array_equal(tab[rows, 0] + np.arange(n) - tab[rows, 2], index), name
    assert sorted(len(mk()[0]) for mk in PACK_CASES.values()) == [1, 2, 3, 3, 5, 50, 50, 51]
    assert PACK_CASES["grid_stride"]()[1].size == 2_097_152 + 300
    t = PACK_CASES["nr50"]()[0]
    assert bool(((t[:-1, 1] == 1) & (t[1:, 1] == 1) & (t[:-1, 0] + 1 == t[1:, 0])).any())


def rand_bits(n, seed):
    """n random 32-bit patterns (1 in 256 is a NaN or an infinity), a quiet and a signalling NaN up front."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    b[:2] = torch.tensor([NAN_BITS, 0x7F800001], dtype=torch.int32)[:n]
    return b


def pack_call(flat, packed, off, tab_d, nr, n, unpack):
    from pathnet_gym_amd.ops import _lib
    _lib.call("launch_pack_ranges", flat.data_ptr(), packed.data_ptr() + 4 * off, tab_d.data_ptr(), nr, n, unpack,
              _lib.stream())
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("case", list(PACK_CASES))
def test_pack_ranges_both_directions_are_exact(hip_lib, case):
    tab, index, size = PACK_CASES[case]()
    nr, n = len(tab), len(index)
    tab_d, idx = torch.from_numpy(tab).to(DEV), torch.from_numpy(index)
    outside = torch.ones(size, dtype=torch.bool)
    outside[idx] = False
    flat0 = rand_bits(size, seed=1)
    flat0[idx[:2]] = flat0[:2][:n].clone()                 # the NaN payloads inside the packed part
    for off in (0, 3):                                       # _pack_tab's destination: buf + packed_off * 4
        # pack: packed[off : off + n] = flat[index]; nothing else written
        flat = flat0.to(DEV).view(torch.float32)
        packed = torch.full((off + n + PAD,), SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
        pack_call(flat, packed, off, tab_d, nr, n, 0)
        pk = packed.view(torch.int32).cpu()
        assert torch.equal(pk[off:off + n], flat0[idx]), (case, off)
        assert bool((pk[:off] == SENT_BITS).all()) and bool((pk[off + n:] == SENT_BITS).all()), (case, off)
        assert torch.equal(flat.view(torch.int32).cpu(), flat0), (case, off)
        # pack then unpack is the identity on flat
        pack_call(flat, packed, off, tab_d, nr, n, 1)
        assert torch.equal(flat.view(torch.int32).cpu(), flat0), (case, off)
        # unpack: flat[index] = packed; every other element (a NaN or the sentinel, alternating) bit-intact
        tgt0 = rand_bits(size, seed=2)
        pos = torch.arange(size)
        tgt0[outside] = torch.where(pos % 2 == 0, NAN_BITS, SENT_BITS).to(torch.int32)[outside]
        src0 = rand_bits(n, seed=3)
        tgt = tgt0.to(DEV).view(torch.float32)
        src = torch.full((off + n + PAD,), SENT_BITS, dtype=torch.int32, device=DEV)
        src[off:off + n] = src0.to(DEV)
        pack_call(tgt, src.view(torch.float32), off, tab_d, nr, n, 1)
        out = tgt.view(torch.int32).cpu()
        assert torch.equal(out[idx], src0), (case, off)
        assert torch.equal(out[outside], tgt0[outside]), (case, off)
        assert torch.equal(src[off:off + n].cpu(), src0) and bool((src[off + n:] == SENT_BITS).all()), (case, off)


@gpu
def test_pack_ranges_launcher_contract(hip_lib):
    from pathnet_gym_amd.ops import _lib
    tab, index, size = PACK_CASES["nr3"]()
    tab_d = torch.from_numpy(tab).to(DEV)
    flat0 = rand_bits(size, seed=4)
    flat = flat0.to(DEV).view(torch.float32)
    packed = torch.full((len(index) + PAD,), SENT, device=DEV)

    def call(nr=3, n=len(index), unpack=0):
        return hip_lib.launch_pack_ranges(flat.data_ptr(), packed.data_ptr(), tab_d.data_ptr(), nr, n, unpack,
                                          _lib.stream())
    assert call(nr=-1) == -22 and call(n=-1) == -22 and call(unpack=-1) == -22
    assert call(nr=0) == -1 and call(n=0) == 0 and call(n=0, unpack=1) == 0
    torch.cuda.synchronize()
    assert bool((packed == SENT).all()) and torch.equal(flat.view(torch.int32).cpu(), flat0)


def random_unions(layout, count, seed):
    """[L, M] unions the way the engine gets them: OR over a population's expressed modules, minus a frozen mask;
    plus the empty one, one without any first-layer module and the full one."""
    L, M = layout.cfg.L, layout.cfg.M
    rng = np.random.default_rng(seed)
    out = [np.zeros((L, M), bool), np.ones((L, M), bool)]
    for i in range(count):
        expressed = rng.random((4, L, M)) < 0.15 + 0.1 * i
        frozen = rng.random((L, M)) < 0.2
        out.append(active_union(expressed, frozen))
    no_first = out[-1].copy()
    no_first[0] = False
    return out + [no_first]


def test_union_ranges_are_sorted_disjoint_merged_and_cover_the_union_cpu():
    layout = ParamLayout(preset("pong").net)
    L, M = layout.cfg.L, layout.cfg.M
    unions = random_unions(layout, 6, seed=1)
    for union in unions:
        rng = union_ranges(layout, union)
        assert all(0 <= s < e <= layout.numel for s, e in rng)
        assert all(e0 < s1 for (_, e0), (s1, _) in zip(rng, rng[1:]))        # sorted, disjoint, merged where they touch
        want = np.zeros(layout.numel, bool)
        for l in range(L):
            for j in range(M):
                if union[l, j]:
                    s, e = layout.module_range(l, j)
                    want[s:e] = True
        want[layout.trunk_numel:] = True
        got = np.zeros(layout.numel, bool)
        for s, e in rng:
            got[s:e] = True
        assert np.array_equal(got, want) and sum(e - s for s, e in rng) == int(want.sum())
        assert len(rng) <= L * M + 1
    assert union_ranges(layout, unions[0]) == [(layout.trunk_numel, layout.numel)]
    assert union_ranges(layout, unions[1]) == [(0, layout.numel)]
    assert max(len(union_ranges(layout, u)) for u in unions) >= 8
    # the module chunks tile the trunk, weights then bias, in layer-major order
    assert layout.module_range(0, 0)[0] == 0 and layout.module_range(L - 1, M - 1)[1] == layout.trunk_numel


@gpu
def test_plan_tables_pack_like_the_host_index(hip_lib):
    """The device table of ``plan_union`` and the two of ``_plan_split`` (split at the first layer's end) pack to
    exactly ``grad.index_select(0, index)``, the host-index fallback of the same class."""
    from pathnet_gym_amd.parallel.comm import FusedUpdateComm
    from pathnet_gym_amd.parallel.dist import DistContext
    layout = ParamLayout(preset("pong").net)
    P = 4
    mk = lambda: FusedUpdateComm(DistContext(), layout, P_total=P, P_local=P, device=DEV)      # noqa: E731
    comm, host, split = mk(), mk(), mk()
    host._gpu_pack = False
    so = layout.layer_info[1]["offset"]
    assert so == layout.module_range(0, layout.cfg.M - 1)[1]
    split.enable_overlap(so)
    grad = rand_bits(layout.numel, seed=5).to(DEV).view(torch.float32)
    sparse = 0
    for union in random_unions(layout, 4, seed=2):
        for c in (comm, host, split):
            c.plan_union(union)
        torch.cuda.synchronize()
        if host.index is None:                               # >= 95 % of the network: the dense plan, no table
            assert comm.rtab is None and comm.dense
            index = torch.arange(layout.numel, device=DEV)
        else:
            sparse += 1
            index, n = host.index, comm.ngrad
            assert comm.rtab is not None and n == index.numel() and comm.nranges == len(comm.ranges)
            comm.buf.fill_(SENT)
            comm._pack(grad, n)
            torch.cuda.synchronize()
            assert torch.equal(comm.buf[:n].view(torch.int32), grad.index_select(0, index).view(torch.int32))
            assert bool((comm.buf[n:n + PAD] == SENT).all())
        i1, i2 = index[index >= so], index[index < so]
        n1, n2 = split.n1, split.n2
        assert (n1, n2) == (i1.numel(), i2.numel()) and (n2 == 0) == (not union[0].any())
        m = n1 + P + split.NCOUNTERS
        split.buf.fill_(SENT)
        split._pack_tab(grad, 0, split.tab1, split.nr1, n1, 0)
        split._pack_tab(grad, m, split.tab2, split.nr2, n2, 0)
        torch.cuda.synchronize()
        assert torch.equal(split.buf[:n1].view(torch.int32), grad.index_select(0, i1).view(torch.int32))
        assert torch.equal(split.buf[m:m + n2].view(torch.int32), grad.index_select(0, i2).view(torch.int32))
        assert bool((split.buf[n1:m] == SENT).all()) and bool((split.buf[m + n2:m + n2 + PAD] == SENT).all())
    assert sparse >= 4


# ---------------------------------------------------------------------------------------------------------------
# 3. launch_refresh_weights_f16 / launch_refresh_weights_cmajor
# ---------------------------------------------------------------------------------------------------------------
F16_GEOMS = [(256, 256, 8), (27, 32, 5), (300, 320, 16)]               # (K, KP, Cout)
CMAJOR_GEOMS = [(8, 8, 4, 8), (4, 2, 4, 3), (2, 2, 8, 5), (4, 2, 8, 6)]        # (KH, KW, CIN, Cout); last: all differ
MODULES = [1, 3, 10]
W_OFF = 37
# beyond fp16's normal range: subnormal results, a flush to zero, the largest half, and two overflows
EXTREMES = [1e-6, -1e-6, 6e-8, 2e-8, 65519.0, -3e-5]
OVERFLOW = [65520.0, 7e4]


def make_weight_flat(K, Cout, M, seed, extremes=True):
    """``flat`` with M chunks of [K, Cout] weights at an odd offset, chunk > K * Cout, NaN everywhere else (the
    biases too).  -> flat, W [M, K, Cout], chunk, (j, c) of the one column that overflows fp16 (or None)."""
    g = torch.Generator().manual_seed(seed)
    chunk = K * Cout + Cout + 3
    W = torch.randn(M, K, Cout, generator=g) * 0.1
    inf_col = None
    if extremes:
        ks = torch.randperm(K, generator=g)[:len(EXTREMES) + len(OVERFLOW)].tolist()
        for i, v in enumerate(EXTREMES):
            W[i % M, ks[i], i % Cout] = v
        W[0, K - 1, 0] = 1e-6                                # the last real k of the first map
        inf_col = (M - 1, Cout - 1)
        for k, v in zip(ks[len(EXTREMES):], OVERFLOW):
            W[inf_col[0], k, inf_col[1]] = v
    flat = torch.full((W_OFF + M * chunk + 29,), NAN)
    for j in range(M):
        flat[W_OFF + j * chunk:W_OFF + j * chunk + K * Cout] = W[j].reshape(-1)
    return flat, W, chunk, inf_col


def ref_f16(W, KP):
    """Wh [M, Cout, KP] (torch's round-to-nearest-even ``.half()``, +0 padding), float64 hcorr and its bound."""
    M, K, Cout = W.shape
    Wh = torch.zeros(M, Cout, KP, dtype=torch.float16)
    Wh[:, :, :K] = W.permute(0, 2, 1).half()
    h64 = Wh.double()
    return Wh, h64.sum(-1), (-(-KP // 256) + 8) * 2.0 ** -24 * h64.abs().sum(-1)


def ref_cmajor(flat, chunk, KH, KW, CIN, Cout, M, f16):
    """Wc[j][c][(ci KH + kh) KW + kw] = cast(flat[w_off + j chunk + ((kh KW + kw) CIN + ci) Cout + c]), by index."""
    K = KH * KW * CIN
    j, c, ci, kh, kw = np.meshgrid(np.arange(M), np.arange(Cout), np.arange(CIN), np.arange(KH), np.arange(KW),
                                   indexing="ij")
    src = W_OFF + j * chunk + ((kh * KW + kw) * CIN + ci) * Cout + c
    v = flat[torch.from_numpy(src.reshape(M, Cout, K))]
    return (v.half() if f16 else v.bfloat16()).view(torch.int16)


def test_operand_copy_references_cpu():
    for K, KP, Cout in F16_GEOMS:
        flat, W, chunk, inf_col = make_weight_flat(K, Cout, 3, seed=K)
        assert W_OFF % 2 == 1 and chunk > K * Cout and int(torch.isfinite(flat).sum()) == 3 * K * Cout
        Wh, hc, bound = ref_f16(W, KP)
        assert bool((Wh[:, :, K:].view(torch.int16) == 0).all())
        inf = torch.isinf(hc)
        assert int(inf.sum()) == 1 and bool(inf[inf_col]) and int(torch.isinf(Wh).sum()) == 2
        sub = (Wh != 0) & (Wh.abs().float() < 2.0 ** -14)
        assert int(sub.sum()) >= 4 and bool((bound[~inf] > 0).all())
        assert float(torch.tensor(2e-8).half()) == 0 and float(torch.tensor(65519.0).half()) == 65504
        assert float(torch.tensor(6e-8).half()) == 2.0 ** -24 and Wh[0, 0, K - 1] == torch.tensor(1e-6).half()
    for KH, KW, CIN, Cout in CMAJOR_GEOMS:
        K = KH * KW * CIN
        assert K % 32 == 0
        flat, W, chunk, _ = make_weight_flat(K, Cout, 3, seed=K + Cout)
        want = W.view(3, KH, KW, CIN, Cout).permute(0, 4, 3, 1, 2).reshape(3, Cout, K)
        for f16 in (0, 1):
            got = ref_cmajor(flat, chunk, KH, KW, CIN, Cout, 3, f16)
            assert torch.equal(got, (want.half() if f16 else want.bfloat16()).view(torch.int16))
            # no other order of the three source axes gives the same copy (only guaranteed when all three differ)
            if len({KH, KW, CIN}) == 3:
                for perm in ((0, 4, 3, 2, 1), (0, 4, 1, 2, 3), (0, 4, 2, 1, 3), (0, 4, 1, 3, 2), (0, 4, 2, 3, 1)):
                    other = W.view(3, KH, KW, CIN, Cout).permute(*perm).reshape(3, Cout, K)
                    assert not torch.equal(got, (other.half() if f16 else other.bfloat16()).view(torch.int16))
    assert any(len({KH, KW, CIN}) == 3 for KH, KW, CIN, _ in CMAJOR_GEOMS)


@gpu
@pytest.mark.parametrize("M", MODULES)
@pytest.mark.parametrize("K,KP,Cout", F16_GEOMS)
def test_refresh_f16_copy_is_exact_and_hcorr_matches_float64(hip_lib, K, KP, Cout, M):
    from pathnet_gym_amd.ops import _lib
    flat, W, chunk, inf_col = make_weight_flat(K, Cout, M, seed=100 * K + M)
    Wh_ref, hc_ref, bound = ref_f16(W, KP)
    n = M * Cout * KP
    Wh = torch.full((n + PAD,), int(SENT), dtype=torch.int16, device=DEV)
    hcorr = torch.full((M * Cout + PAD,), SENT, device=DEV)
    _lib.call("launch_refresh_weights_f16", flat.to(DEV).data_ptr(), W_OFF, chunk, K, KP, Cout, M, Wh.data_ptr(),
              hcorr.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert bool((Wh[n:] == int(SENT)).all()) and bool((hcorr[M * Cout:] == SENT).all())
    assert torch.equal(Wh[:n].cpu().view(M, Cout, KP), Wh_ref.view(torch.int16))
    hc = hcorr[:M * Cout].cpu().double().view(M, Cout)
    inf = torch.isinf(hc_ref)
    assert torch.equal(hc[inf], hc_ref[inf]) and bool(inf[inf_col]) and bool(torch.isfinite(hc[~inf]).all())
    ratio = float(((hc - hc_ref).abs()[~inf] / bound[~inf]).max())
    print(f"hcorr K={K} KP={KP} Cout={Cout} M={M}: worst err / bound = {ratio:.4f}")
    record_measured({"refresh_f16.hcorr": ratio})
    assert ratio <= 1.0


@gpu
def test_refresh_f16_launcher_contract(hip_lib):
    from pathnet_gym_amd.ops import _lib
    K, KP, Cout, M = 27, 32, 5, 3
    flat, _, chunk, _ = make_weight_flat(K, Cout, M, seed=1)
    flat_d = flat.to(DEV)
    Wh = torch.full((M * Cout * KP + PAD,), int(SENT), dtype=torch.int16, device=DEV)
    hcorr = torch.full((M * Cout + PAD,), SENT, device=DEV)

    def call(w_off=W_OFF, chunk=chunk, K=K, KP=KP, Cout=Cout, M=M):
        return hip_lib.launch_refresh_weights_f16(flat_d.data_ptr(), w_off, chunk, K, KP, Cout, M, Wh.data_ptr(),
                                                  hcorr.data_ptr(), _lib.stream())
    assert call(KP=K - 1) == -1 and call(KP=1) == -1
    for kw in (dict(chunk=0), dict(K=0), dict(KP=0), dict(Cout=0), dict(M=0), dict(w_off=-1), dict(chunk=-5),
               dict(K=-27), dict(KP=-32), dict(Cout=-5), dict(M=-3)):
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert bool((Wh == int(SENT)).all()) and bool((hcorr == SENT).all())


@gpu
@pytest.mark.parametrize("M", MODULES)
@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("KH,KW,CIN,Cout", CMAJOR_GEOMS)
def test_refresh_cmajor_copy_is_the_exact_permutation(hip_lib, KH, KW, CIN, Cout, f16, M):
    from pathnet_gym_amd.ops import _lib
    K = KH * KW * CIN
    flat, _, chunk, _ = make_weight_flat(K, Cout, M, seed=1000 * K + 10 * Cout + M)
    want = ref_cmajor(flat, chunk, KH, KW, CIN, Cout, M, f16)
    n = M * Cout * K
    Wc = torch.full((n + PAD,), int(SENT), dtype=torch.int16, device=DEV)
    _lib.call("launch_refresh_weights_cmajor", flat.to(DEV).data_ptr(), W_OFF, chunk, KH, KW, CIN, Cout, M,
              Wc.data_ptr(), f16, _lib.stream())
    torch.cuda.synchronize()
    assert bool((Wc[n:] == int(SENT)).all())
    assert torch.equal(Wc[:n].cpu().view(M, Cout, K), want)


@gpu
def test_refresh_cmajor_launcher_contract(hip_lib):
    from pathnet_gym_amd.ops import _lib
    flat, _, chunk, _ = make_weight_flat(36, 4, 2, seed=2)
    flat_d = flat.to(DEV)
    Wc = torch.full((2 * 4 * 36 + PAD,), int(SENT), dtype=torch.int16, device=DEV)

    def call(KH=3, KW=3, CIN=4, Cout=4, M=2, f16=0, w_off=W_OFF, chunk=chunk):
        return hip_lib.launch_refresh_weights_cmajor(flat_d.data_ptr(), w_off, chunk, KH, KW, CIN, Cout, M,
                                                     Wc.data_ptr(), f16, _lib.stream())
    assert call() == -22 and call(KH=1, KW=1, CIN=31) == -22 and call(KH=2, KW=2, CIN=4) == -22     # K % 32 != 0
    for kw in (dict(KH=0), dict(KW=0), dict(CIN=0), dict(Cout=0), dict(M=0), dict(chunk=0), dict(w_off=-1),
               dict(f16=-1)):
        assert call(**dict(dict(KH=4, KW=2, CIN=4), **kw)) == -22, kw
    torch.cuda.synchronize()
    assert bool((Wc == int(SENT)).all())
