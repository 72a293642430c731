"""HIP kernel numerics vs the fp32 PyTorch oracle (run on an MI355X).

Every test compares a hand-written gfx950 kernel against a plain PyTorch
fp32 implementation of the same op (``models/pathnet.py``,
``algo/a2c_math.py``, ``algo/optim.py``, ``envs/*.py``).  bf16 MFMA operands
give ~1e-3 .. 1e-2 relative error: every budget is 3x the measured error of that layer / segment / path
(tests/numerics_budget.py, tests/data/numerics_measured.json); envs are integer/bit exact.
"""
import os

import numpy as np
import pytest
import torch

import numerics_budget as budget
from pathnet_gym_amd.algo.a2c_math import a2c_loss, nstep_returns
from pathnet_gym_amd.algo.ga import Population, get_geopath
from pathnet_gym_amd.config import LayerSpec, PathNetConfig, preset
from pathnet_gym_amd.models.acnet import ACPathNet
from pathnet_gym_amd.models.pathnet import heads_ref, trunk_forward_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a, b):
    a = a.float().flatten()
    b = b.float().flatten()
    return float((a - b).norm() / (b.norm() + 1e-12))


def random_masks(P, L, M, N, seed=0, with_edge=True):
    rng = np.random.RandomState(seed)
    m = np.stack([get_geopath(L, M, N, rng) for _ in range(P)])
    if with_edge and P >= 3:
        m[0, 1, :] = 0          # empty layer -> zero output
        m[1, :, :] = 1          # all modules active
        m[2, 0, :] = 0
        m[2, 0, M - 1] = 1      # single (odd) module
    return m


def small_pixel_cfg(M=10, N=4):
    return PathNetConfig(L=5, M=M, N=N, input_shape=(160, 120, 4),
                         layers=[LayerSpec("conv", 8, 8, 4), LayerSpec("conv", 8, 4, 2), LayerSpec("conv", 8, 3, 1),
                                 LayerSpec("fc", 256), LayerSpec("fc", 256)],
                         trunk_scale="M", num_actions=6)


def make_model(cfg, P, masks, seed=3):
    m = ACPathNet(cfg, P, DEV, "hip", seed=seed)
    m.set_paths(masks)
    return m


# ---------------------------------------------------------------------------
def test_trunk_forward_matches_oracle(hip_lib):
    cfg = small_pixel_cfg()
    P, E = 4, 16
    masks = random_masks(P, cfg.L, cfg.M, cfg.N)
    m = make_model(cfg, P, masks)
    g = torch.Generator(device="cpu").manual_seed(0)
    obs = torch.randint(0, 256, (P * E, 160, 120, 4), generator=g, dtype=torch.uint8).to(DEV)
    feat = m.hip.trunk(obs, E)
    with torch.no_grad():
        ref = trunk_forward_ref(m.store, obs.float() / 255.0, m.mask.repeat_interleave(E, 0))
    assert feat.shape == ref.shape
    # path 0 has an empty layer 1 -> every later layer sees zeros
    errs = {}
    for p in range(P):
        sl = slice(p * E, (p + 1) * E)
        if ref[sl].norm() == 0:
            assert feat[sl].norm() == 0, p
            continue
        errs[f"path{p}"] = rel(feat[sl], ref[sl])
    print("bf16 trunk forward vs fp32 oracle:", errs)
    budget.check("trunk_forward_bf16", errs, 3e-2)


def test_conv1_fp16_offset_forward_is_tight(hip_lib):
    """First conv layer (uint8 pixels): fp16 MFMA on (1024 + pixel) with the offset removed through the bias
    (csrc/conv_fast.hip F16 path) vs an fp32 conv with the same fp16-rounded weights; only the bf16 output
    rounding separates them."""
    import torch.nn.functional as F
    cfg = small_pixel_cfg()
    P, E = 4, 16
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, seed=11)
    m = make_model(cfg, P, masks, seed=9)
    hp = m.hip
    g0 = hp.geoms[0]
    obs = torch.randint(0, 256, (P * E, 160, 120, 4), generator=torch.Generator().manual_seed(3),
                        dtype=torch.uint8).to(DEV)
    Y = torch.zeros(P * E, g0.out_feat, dtype=torch.bfloat16, device=DEV)
    bits, rows = hp.alloc_bits(0, 1, P * E)
    hp.layer_fwd(0, obs, Y, bits, P, E, 1, 0, rows)
    torch.cuda.synchronize()
    W = m.store.W(0).detach().to(torch.float16).float()          # [M, K, 8]
    b = m.store.b(0).detach()
    Wc = W.reshape(cfg.M, 8, 8, 4, 8).permute(0, 4, 3, 1, 2).reshape(cfg.M * 8, 4, 8, 8)
    y = F.conv2d(obs.permute(0, 3, 1, 2).float() / 255.0, Wc, b.reshape(-1), stride=4)
    y = F.relu(y).view(P * E, cfg.M, 8, g0.Ho, g0.Wo) * m.mask[:, 0].repeat_interleave(E, 0)[:, :, None, None, None]
    ref = y.sum(1).permute(0, 2, 3, 1).reshape(P * E, -1)
    assert rel(Y.float(), ref) < 4e-3, rel(Y.float(), ref)


def test_conv_forward_multi_step_launch_matches_per_step(hip_lib):
    """A T=2 forward launch (row iterators across the step boundary) writes exactly what two T=1 launches write
    (the one-step fast path computes global rows linearly, csrc/conv_fast.hip conv_fwd_fast `lin`)."""
    cfg = small_pixel_cfg()
    P, E, T = 4, 16, 2
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, seed=5)
    m = make_model(cfg, P, masks, seed=4)
    hp = m.hip
    B = P * E
    g = torch.Generator().manual_seed(8)
    x = torch.randint(0, 256, (T, B, 160 * 120 * 4), generator=g, dtype=torch.uint8).to(DEV)
    for l in range(3):                         # conv1 (uint8, affine path), conv2, conv3 (bf16 inputs)
        gl = hp.geoms[l]
        outs = []
        for mode in ("multi", "single"):
            Y = torch.zeros(T + 1, B, gl.out_feat, dtype=torch.bfloat16, device=DEV)
            bits, rows = hp.alloc_bits(l, T + 1, B)
            if mode == "multi":
                hp.layer_fwd(l, x, Y, bits, P, E, T, 0, rows)
            else:
                for t in range(T):
                    hp.layer_fwd(l, x, Y, bits, P, E, 1, t, rows)
            torch.cuda.synchronize()
            outs.append((Y, bits))
        assert torch.equal(outs[0][0], outs[1][0]), l
        assert torch.equal(outs[0][1], outs[1][1]), l
        x = outs[0][0]


def test_fc_trunk_forward_vector_input(hip_lib):
    cfg = preset("cartpole").net
    P, E = 6, 16
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, with_edge=False)
    m = make_model(cfg, P, masks)
    x = torch.randn(P * E, 4, device=DEV)
    feat = m.hip.trunk(x, E)
    with torch.no_grad():
        ref = trunk_forward_ref(m.store, x.to(torch.bfloat16).float(), m.mask.repeat_interleave(E, 0))
    budget.check("fc_trunk_forward_bf16", {"all": rel(feat, ref)}, 3e-2)


def _hip_trunk_fwd_bwd(m, obs_steps, dfeat, P, E):
    """Run T forward steps into engine-style buffers, then the trunk backward."""
    hp = m.hip
    T = len(obs_steps)
    B = P * E
    obs = torch.stack(obs_steps).reshape(T, B, -1).contiguous()
    acts, bits, rows, grads = [], [], [], []
    for l, g in enumerate(hp.geoms):
        acts.append(torch.zeros(T, B, g.out_feat, dtype=torch.bfloat16, device=DEV))
        b, r = hp.alloc_bits(l, T, B)
        bits.append(b)
        rows.append(r)
        grads.append(torch.zeros(T * B, g.out_feat, dtype=torch.float32, device=DEV))
    for t in range(T):
        x = obs
        for l in range(len(hp.geoms)):
            hp.layer_fwd(l, x, acts[l], bits[l], P, E, 1, t, rows[l])
            x = acts[l]
    grad_flat = torch.zeros_like(m.store.flat, requires_grad=False)
    grads[-1].copy_(dfeat)
    L = len(hp.geoms)
    for l in range(L - 1, -1, -1):
        X = obs if l == 0 else acts[l - 1]
        dX = grads[l - 1] if l > 0 else None
        hp.layer_bwd(l, X, grads[l], bits[l], grad_flat, dX, P, E, T, rows[l])
    torch.cuda.synchronize()
    return acts[-1].reshape(T * B, -1).float(), grad_flat


@pytest.mark.parametrize("wgrad_gm", [True, False], ids=["fc_wgrad_gm", "fc_wgrad_tiles"])
def test_trunk_backward_matches_autograd(hip_lib, wgrad_gm):
    cfg = small_pixel_cfg()
    P, E, T = 4, 16, 2
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, seed=5)
    m = make_model(cfg, P, masks, seed=7)
    m.hip.fc_wgrad_gm = wgrad_gm     # fc1 (K=1408): wgrad from the dgrad's masked-bf16 side output, or not
    g = torch.Generator(device="cpu").manual_seed(1)
    obs_steps = [torch.randint(0, 256, (P * E, 160, 120, 4), generator=g, dtype=torch.uint8).to(DEV)
                 for _ in range(T)]
    dfeat = torch.randn(T * P * E, 256, generator=g).to(DEV)
    feat_hip, grad_hip = _hip_trunk_fwd_bwd(m, obs_steps, dfeat, P, E)
    # oracle: rows ordered [t][p][e]
    flat = m.store.flat.detach().clone().requires_grad_(True)
    from pathnet_gym_amd.models.pathnet import ParamStore
    st = ParamStore(cfg, DEV, flat=flat)
    x = torch.cat(obs_steps).float() / 255.0
    mask = m.mask.repeat_interleave(E, 0).repeat(T, 1, 1)
    feat_ref = trunk_forward_ref(st, x, mask, emulate_bf16=True)
    (feat_ref * dfeat).sum().backward()
    gref = flat.grad
    test = f"trunk_backward_bf16_{'gm' if wgrad_gm else 'tiles'}"
    budget.check(test + "_fwd", {"feat": rel(feat_hip, feat_ref.detach())}, 1e-2)
    lay = m.store.layout
    errs = {}
    for s in lay.segments:
        if s.layer < 0:
            continue
        a = grad_hip[s.offset:s.offset + s.numel]
        b = gref[s.offset:s.offset + s.numel]
        if b.norm() < 1e-6:
            assert a.norm() < 1e-4, s.name
            continue
        errs[s.name] = rel(a, b)
    print({k: round(v, 4) for k, v in errs.items()})
    assert len(errs) > 20
    # every layer's WHOLE gradient (all modules) and every segment, each within 3x its measured error
    layer = {}
    for l in range(cfg.L):
        segs = [x for x in lay.segments if x.layer == l]
        a = torch.cat([grad_hip[x.offset:x.offset + x.numel] for x in segs])
        b = torch.cat([gref[x.offset:x.offset + x.numel] for x in segs])
        layer[f"layer{l}"] = rel(a, b)
    budget.check(test + "_layers", layer, 3e-2)
    budget.check(test + "_segments", errs, 6e-2)


def test_fc_backward_vector(hip_lib):
    cfg = preset("cartpole").net
    P, E, T = 4, 16, 3
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, seed=2, with_edge=False)
    m = make_model(cfg, P, masks)
    from pathnet_gym_amd.ops.envs import obs_to_bf16_padded
    xs = [torch.randn(P * E, 4, device=DEV) for _ in range(T)]
    obs_steps = [obs_to_bf16_padded(x) for x in xs]
    dfeat = torch.randn(T * P * E, 32, device=DEV)
    feat_hip, grad_hip = _hip_trunk_fwd_bwd(m, obs_steps, dfeat, P, E)
    flat = m.store.flat.detach().clone().requires_grad_(True)
    from pathnet_gym_amd.models.pathnet import ParamStore
    st = ParamStore(cfg, DEV, flat=flat)
    x = torch.cat(xs).to(torch.bfloat16).float()
    feat_ref = trunk_forward_ref(st, x, m.mask.repeat_interleave(E, 0).repeat(T, 1, 1), emulate_bf16=True)
    (feat_ref * dfeat).sum().backward()
    for s in m.store.layout.segments:
        if s.layer < 0:
            continue
        a, b = grad_hip[s.offset:s.offset + s.numel], flat.grad[s.offset:s.offset + s.numel]
        if b.norm() < 1e-6:
            continue
        assert rel(a, b) < 3e-2, (s.name, rel(a, b))


def test_heads_and_a2c_grad(hip_lib):
    from pathnet_gym_amd.ops import _lib
    cfg = small_pixel_cfg()
    P, E, T = 2, 16, 5
    B = P * E
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, with_edge=False)
    m = make_model(cfg, P, masks)
    hp = m.hip
    A = cfg.num_actions
    feat = (torch.randn(T + 1, B, 256, device=DEV) * 0.5).to(torch.bfloat16)
    logits = torch.zeros(T + 1, B, A, device=DEV)
    values = torch.zeros(T + 1, B, device=DEV)
    actions = torch.zeros(T + 1, B, dtype=torch.int32, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    for t in range(T + 1):
        hp.heads_fwd(feat[t], logits[t], values[t], actions[t], 123, ctr, t, T + 1, greedy=(t == T))
    lr_, vr_ = heads_ref(m.store, feat.float().reshape(-1, 256))
    assert rel(logits.reshape(-1, A), lr_.detach()) < 1e-4
    assert rel(values.reshape(-1), vr_.detach()) < 1e-4
    assert int(actions.min()) >= 0 and int(actions.max()) < A
    # sampling frequency sanity: greedy step picks the argmax
    assert torch.equal(actions[T].long(), logits[T].argmax(-1))
    rewards = torch.randint(-1, 2, (T, B), device=DEV).float() * 2
    dones = (torch.rand(T, B, device=DEV) < 0.2).to(torch.uint8)
    dlog = torch.zeros(T, B, A, device=DEV)
    dval = torch.zeros(T, B, device=DEV)
    stats = torch.zeros(4, device=DEV)
    beta, w = 0.01, 1.0 / E
    _lib.call("launch_a2c_grad", logits.data_ptr(), values.data_ptr(), actions.data_ptr(), rewards.data_ptr(),
              dones.data_ptr(), values[T].data_ptr(), T, B, A, 0.99, 1.0, 1.0, beta, 0.5, w, dlog.data_ptr(),
              dval.data_ptr(), stats.data_ptr(), _lib.stream())
    R, adv = nstep_returns(rewards, values[:T], dones.bool(), values[T], 0.99, 1.0, 1.0)
    lg = logits[:T].reshape(-1, A).clone().requires_grad_(True)
    vv = values[:T].reshape(-1).clone().requires_grad_(True)
    loss, lp, lv, ent = a2c_loss(lg, vv, actions[:T].reshape(-1), R.reshape(-1), adv.reshape(-1), beta, 0.5,
                                 torch.full((T * B,), w, device=DEV))
    loss.backward()
    assert rel(dlog.reshape(-1, A), lg.grad) < 1e-4
    assert rel(dval.reshape(-1), vv.grad) < 1e-4
    assert abs(float(stats[0]) - float(lp)) < 1e-3 * max(1.0, abs(float(lp)))
    # heads backward
    gflat = torch.zeros_like(m.store.flat, requires_grad=False)
    dfeat = torch.zeros(T * B, 256, device=DEV)
    hp.heads_bwd(feat[:T].reshape(T * B, 256), dlog.reshape(T * B, A), dval.reshape(-1), gflat, dfeat)
    flat = m.store.flat.detach().clone().requires_grad_(True)
    from pathnet_gym_amd.models.pathnet import ParamStore
    st = ParamStore(cfg, DEV, flat=flat)
    fx = feat[:T].reshape(T * B, 256).float().requires_grad_(True)
    l2, v2 = heads_ref(st, fx)
    ((l2 * dlog.reshape(T * B, A)).sum() + (v2 * dval.reshape(-1)).sum()).backward()
    assert rel(dfeat, fx.grad) < 1e-4
    for name in ("policy.weight", "policy.bias", "value.weight", "value.bias"):
        s = m.store.layout.by_name[name]
        assert rel(gflat[s.offset:s.offset + s.numel], flat.grad[s.offset:s.offset + s.numel]) < 1e-4, name


# ---------------------------------------------------------------------------
# a2c_grad_kernel (csrc/heads.hip) over its whole switch space, against float64
# ---------------------------------------------------------------------------
A2C_GAMMA, A2C_BETA, A2C_VCOEF = 0.99, 0.01, 0.5
A2C_QUANTITIES = ("dlogits", "dvalue", "policy_loss", "value_loss", "entropy_sum")
A2C_EPS32 = 2.0 ** -24          # an fp32 result carries this much relative rounding whatever computed it
# the kernel's error against float64 may be this many times the plain fp32 torch evaluation's (see
# test_a2c_grad_kernel_vs_float64 for the measured errors behind it)
A2C_ERR_MULT = 4.0
A2C_REL_CEILING = 1e-4          # the project's bound for this kernel (test_heads_and_a2c_grad)


def _a2c_launch(logits, values, actions, rewards, dones, vboot, lam, rclip, weight):
    from pathnet_gym_amd.ops import _lib
    T, B, A = logits.shape
    dlog = torch.zeros(T, B, A, device=DEV)
    dval = torch.zeros(T, B, device=DEV)
    stats = torch.zeros(4, device=DEV)
    _lib.call("launch_a2c_grad", logits.data_ptr(), values.data_ptr(), actions.data_ptr(), rewards.data_ptr(),
              dones.data_ptr(), vboot.data_ptr(), T, B, A, A2C_GAMMA, lam, rclip, A2C_BETA, A2C_VCOEF, weight,
              dlog.data_ptr(), dval.data_ptr(), stats.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return {"dlogits": dlog, "dvalue": dval, "policy_loss": stats[0], "value_loss": stats[1], "entropy_sum": stats[2]}


def _a2c_torch(dtype, logits, values, actions, rewards, dones, vboot, lam, rclip, weight):
    """algo/a2c_math.py nstep_returns + a2c_loss with autograd, evaluated in ``dtype`` on the same inputs."""
    T, B, A = logits.shape
    R, adv = nstep_returns(rewards.to(dtype), values.to(dtype), dones.bool(), vboot.to(dtype), A2C_GAMMA, lam, rclip)
    lg = logits.to(dtype).reshape(-1, A).clone().requires_grad_(True)
    vv = values.to(dtype).reshape(-1).clone().requires_grad_(True)
    wt = torch.full((T * B,), weight, dtype=dtype, device=DEV)
    loss, lp, lv, ent = a2c_loss(lg, vv, actions.reshape(-1), R.reshape(-1), adv.reshape(-1), A2C_BETA, A2C_VCOEF, wt)
    loss.backward()
    out = {"dlogits": lg.grad.reshape(T, B, A), "dvalue": vv.grad.reshape(T, B), "policy_loss": lp, "value_loss": lv,
           "entropy_sum": ent * (T * B)}
    # the policy loss is a sum of terms of both signs: its error is measured against the sum of their magnitudes
    # (the value loss and the entropy are sums of non-negative terms: their own value is that scale)
    with torch.no_grad():
        pi = torch.softmax(lg, -1)
        log_pi = torch.log(pi.clamp(1e-20, 1.0))
        lp_a = log_pi.gather(1, actions.reshape(-1).long()[:, None]).squeeze(1)
        entropy = -(pi * log_pi).sum(-1)
        out["policy_scale"] = (((lp_a * adv.reshape(-1)).abs() + A2C_BETA * entropy) * wt).sum()
    return out


def _a2c_errors(out, ref64):
    """Relative error of every compared quantity against the float64 reference, computed in float64."""
    err = {}
    for k in ("dlogits", "dvalue"):
        a, b = out[k].double().flatten(), ref64[k].flatten()
        err[k] = float((a - b).norm() / b.norm())
    for k, scale in (("policy_loss", "policy_scale"), ("value_loss", "value_loss"), ("entropy_sum", "entropy_sum")):
        err[k] = abs(float(out[k].double()) - float(ref64[k])) / float(ref64[scale])
    return err


def _a2c_check(label, inputs, lam, rclip, weight):
    """Launch twice, compare with float64 under a bound tied to the fp32 torch evaluation's own error."""
    out = _a2c_launch(*inputs, lam, rclip, weight)
    again = _a2c_launch(*inputs, lam, rclip, weight)
    ref64 = _a2c_torch(torch.float64, *inputs, lam, rclip, weight)
    e32 = _a2c_errors(_a2c_torch(torch.float32, *inputs, lam, rclip, weight), ref64)
    ek = _a2c_errors(out, ref64)
    for k in A2C_QUANTITIES:
        print(f"a2c_grad {label} {k}: fp32-torch {e32[k]:.3e} kernel {ek[k]:.3e}")
    for k in A2C_QUANTITIES:
        assert bool(torch.isfinite(out[k]).all()), (label, k)
    # one thread per (t, b) with a fixed arithmetic order: a second launch repeats every per-sample output bit for bit
    # (the three sums meet in atomics across workgroups and are compared by value only)
    assert torch.equal(out["dvalue"], again["dvalue"]) and torch.equal(out["dlogits"], again["dlogits"]), label
    for k in A2C_QUANTITIES:
        assert ek[k] <= A2C_ERR_MULT * max(e32[k], A2C_EPS32), (label, k, ek[k], e32[k])
        assert ek[k] < A2C_REL_CEILING, (label, k, ek[k])
    return out, ref64


def _a2c_inputs(T, B, A, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, B, A, generator=g) * 2.0
    values = torch.randn(T, B, generator=g)
    vboot = torch.randn(B, generator=g)
    actions = torch.randint(0, A, (T, B), generator=g, dtype=torch.int32)
    # non-integer rewards of both signs, magnitudes from 0.05 to 2.5: below and above both clips (0.5 and 1.0)
    mag = 0.05 + 2.45 * torch.rand(T, B, generator=g)
    rewards = mag * (torch.randint(0, 2, (T, B), generator=g).float() * 2 - 1)
    assert float(mag.min()) < 0.5 and ((mag > 0.5) & (mag < 1.0)).any() and float(mag.max()) > 1.0
    dones = (torch.rand(T, B, generator=g) < 0.2).to(torch.uint8)
    dones[:, 0] = 0                       # never done: bootstraps from vboot through every step
    dones[:, 1] = 1                       # done at every step: nothing carries
    dones[:, 2] = 0
    dones[0, 2] = 1                       # done only at t = 0
    dones[:, 3] = 0
    dones[T - 1, 3] = 1                   # done only at t = T - 1: vboot must not leak into any step
    return tuple(x.to(DEV).contiguous() for x in (logits, values, actions, rewards, dones, vboot))


@pytest.mark.parametrize("T,B,A", [(1, 16, 2), (5, 48, 6), (20, 33, 18)])
@pytest.mark.parametrize("rclip", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("lam", [1.0, 0.95, 0.0])
def test_a2c_grad_kernel_vs_float64(hip_lib, lam, rclip, T, B, A):
    """launch_a2c_grad over its switches -- the n-step (lam == 1) and GAE (lam != 1) recurrences, the reward clip off
    / 1.0 / 0.5, A at both ends of AMAX, one partial workgroup / one nearly full / three with a partial last one --
    against nstep_returns + a2c_loss + autograd in float64.  Columns 0..3 of ``dones`` are never / always / only at
    t = 0 / only at t = T - 1, the rest random at p = 0.2.

    Bound: the kernel (fast exp / log intrinsics, its own summation order) may be A2C_ERR_MULT times as far from
    float64 as the same torch code evaluated in fp32 is (with 2^-24 as the floor of that yardstick), and never
    beyond the project's 1e-4.

    Measured on an MI355X, relative error against float64 (fp32 torch / kernel), per shape the largest over the
    nine (lam, rclip) settings, and the largest kernel / max(fp32 torch, 2^-24) ratio of any single case:
        (T, B, A)      dlogits          dvalue           policy loss      value loss       entropy sum
        (1, 16, 2)     1.2e-7 / 1.0e-7  5.5e-8 / 5.5e-8  3.7e-8 / 9.6e-8  1.4e-7 / 1.4e-7  9.9e-8 / 6.1e-8
        (5, 48, 6)     9.9e-8 / 7.7e-8  6.6e-8 / 5.5e-8  2.8e-8 / 1.9e-8  8.8e-8 / 1.4e-7  6.8e-8 / 6.8e-8
        (20, 33, 18)   1.1e-7 / 1.0e-7  8.0e-8 / 8.4e-8  9.0e-9 / 8.9e-9  5.7e-8 / 8.8e-8  1.2e-7 / 1.3e-8
        worst ratio    1.03             1.05             1.61             2.34             1.00
    The kernel is as close to float64 as fp32 torch is; the per-sample outputs never exceed its error by more than
    5 %.  The three sums are single numbers, so a ratio of two roundings of a few 2^-24 each moves by chance (2.34
    at worst, both errors below 1.5e-7).  A2C_ERR_MULT = 4 leaves that room and no more: a wrong nd factor, carry or
    clip changes a result by 1e-2 or more."""
    inputs = _a2c_inputs(T, B, A, seed=1000 * T + A)
    _a2c_check(f"T{T} B{B} A{A} lam{lam} rclip{rclip}", inputs, lam, rclip, 1.0 / 16)


def test_a2c_grad_kernel_extreme_logits(hip_lib):
    """Softmax edges of a2c_grad_kernel: rows whose logits spread over ~60 (three of six pi_j below the 1e-20 clip of
    log(clip(pi)), taken actions on both sides of it), rows of equal logits, and the same rows offset by +80 and -80.
    The logits are multiples of 2^-10, so the offset rows hold exactly logit + 80: after the max subtraction they are
    the same numbers, and every per-sample output must repeat the un-offset rows bit for bit.  Same float64
    reference and bound as test_a2c_grad_kernel_vs_float64 (a2c_loss clamps, and autograd gives the clamp's zero
    gradient).

    Measured on an MI355X (fp32 torch / kernel, lam = 1.0 and 0.95): dlogits 5.9e-8 / 6.3e-8 and 8.4e-8 / 7.8e-8,
    dvalue 3.2e-8 / 3.2e-8 and 5.1e-8 / 5.9e-8, policy loss 1.7e-8 / 9.9e-9 and 4.9e-8 / 3.4e-8, value loss 8.7e-8 /
    5.9e-8 and 3.6e-8 / 3.6e-8, entropy sum 1.1e-7 / 1.1e-7 in both; worst ratio 1.06.  Before the kernel dropped the
    advantage term of a taken action whose pi_a is under the clip (where log(clip(pi_a)) is constant), its dlogits
    were off by a relative 1.06 here."""
    T, A, nb = 3, 6, 16
    g = torch.Generator().manual_seed(7)
    spread = torch.tensor([0.0, -10.0, -30.0, -50.0, -55.0, -60.0])
    base = torch.zeros(T, nb, A)
    for b in range(12):
        base[:, b] = torch.roll(spread, b % A)
    base[:, :12] += torch.randint(-256, 257, (T, 12, A), generator=g).float() / 1024     # +-0.25: far from the clip
    base[:, 12:] = torch.tensor([0.0, 0.703125, -3.5, 17.25])[None, :, None]             # rows of equal logits
    logits = torch.cat([base, base + 80.0, base - 80.0], 1)
    assert torch.equal(logits[:, nb:2 * nb] - 80.0, base) and torch.equal(logits[:, 2 * nb:] + 80.0, base)
    B = 3 * nb
    rep = lambda x: torch.cat([x, x, x], -1)
    values = rep(torch.randn(T, nb, generator=g))
    vboot = rep(torch.randn(nb, generator=g))
    rewards = rep(torch.randn(T, nb, generator=g) * 1.5)
    dones = rep((torch.rand(T, nb, generator=g) < 0.2).to(torch.uint8))
    # column b (spread rolled by b), step t takes action (2b + t) % A, the spread's entry (b + t) % A: all six of
    # them over the columns, clipped ones included
    actions = rep(((2 * torch.arange(nb)[None, :] + torch.arange(T)[:, None]) % A).to(torch.int32))
    pi = torch.softmax(logits.double(), -1)
    taken = pi.gather(-1, actions.long()[..., None])
    assert int((pi[:, :12] < 1e-21).sum(-1).min()) == 3 and not ((pi > 1e-21) & (pi < 1e-19)).any()
    assert (taken < 1e-21).any() and (taken > 1e-19).any()
    inputs = tuple(x.to(DEV).contiguous() for x in (logits, values, actions, rewards, dones, vboot))
    for lam in (1.0, 0.95):
        out, _ = _a2c_check(f"extreme lam{lam}", inputs, lam, 1.0, 1.0 / 16)
        for k in ("dlogits", "dvalue"):
            for off in (1, 2):
                assert torch.equal(out[k][:, off * nb:(off + 1) * nb], out[k][:, :nb]), (lam, k, off)


@pytest.mark.parametrize("A,F", [(18, 256), (6, 96), (3, 64), (6, 256), (8, 128)])
def test_heads_fwd_action_and_feature_widths(hip_lib, A, F):
    """Lane-per-sample heads forward for A <= 8 and A <= 18 (and the 16-samples-per-workgroup form for A <= 8,
    F % 128 == 0), a partial last workgroup, several F."""
    cfg = PathNetConfig(L=2, M=4, N=2, input_shape=(4,), layers=[LayerSpec("fc", 64), LayerSpec("fc", F)],
                        trunk_scale="none", num_actions=A)
    P, E = 3, 16
    m = make_model(cfg, P, random_masks(P, cfg.L, cfg.M, cfg.N, with_edge=False))
    B = P * E + 5
    feat = torch.randn(B, F, device=DEV).to(torch.bfloat16)
    logits = torch.zeros(B, A, device=DEV)
    values = torch.zeros(B, device=DEV)
    actions = torch.zeros(B, dtype=torch.int32, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    m.hip.heads_fwd(feat, logits, values, actions, 7, ctr, 0, 1, greedy=True)
    lr_, vr_ = heads_ref(m.store, feat.float())
    assert rel(logits, lr_.detach()) < 1e-4 and rel(values, vr_.detach()) < 1e-4
    assert torch.equal(actions.long(), logits.argmax(-1))


def test_heads_sampling_row_base_and_torch_keyed_sampler(hip_lib):
    """Sampling is keyed by the GLOBAL sample index (row_base + b): a launch over rows [k, B) with row_base = k draws
    what the full launch drew for those rows (strong scaling: a rank's envs sample like one GPU's), and the torch
    sampler of the CPU backend (a2c_math.sample_actions_keyed) reproduces the kernel's draws."""
    from pathnet_gym_amd.algo.a2c_math import sample_actions_keyed
    cfg = PathNetConfig(L=2, M=4, N=2, input_shape=(4,), layers=[LayerSpec("fc", 64), LayerSpec("fc", 128)],
                        trunk_scale="none", num_actions=6)
    P, E = 4, 16
    m = make_model(cfg, P, random_masks(P, cfg.L, cfg.M, cfg.N, with_edge=False))
    B = P * E
    feat = torch.randn(B, 128, generator=torch.Generator().manual_seed(5)).to(DEV).to(torch.bfloat16)
    ctr = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    outs = []
    for k in (0, 16):
        logits = torch.zeros(B - k, 6, device=DEV)
        values = torch.zeros(B - k, device=DEV)
        actions = torch.zeros(B - k, dtype=torch.int32, device=DEV)
        m.hip.heads_fwd(feat[k:].contiguous(), logits, values, actions, 99, ctr, 2, 5, row_base=k)
        outs.append((logits, actions))
    torch.cuda.synchronize()
    assert torch.equal(outs[1][1], outs[0][1][16:])
    # __logf vs torch.log: only near-ties may differ.  The rule of test_heads_kernels.py: the kernel's action is the
    # float64 Gumbel argmax on every row whose top-two gap is at least 8 e32, and the torch sampler obeys it too
    import test_heads_kernels as thk
    ta = sample_actions_keyed(outs[0][0], 99, 3 * 5 + 2, 0)
    for tag, a in (("hip", outs[0][1]), ("torch", ta)):
        thk.check_sampler_agreement(outs[0][0], a, 99, 3 * 5 + 2, 0, f"row_base test, {tag}", record=False)


@pytest.mark.parametrize("rows", [32, 128])
def test_heads_bwd_row_chunks_match_oracle(hip_lib, rows):
    """The default 32-row chunks with partials + wide chunk reduction (1 280 workgroups at the bench shape) and the
    128-row atomic kernel (heads_set_bwd_rows(128)) against the fp32 oracle at an N that is not a multiple of 32."""
    from pathnet_gym_amd.models.pathnet import ParamStore
    from pathnet_gym_amd.ops import _lib
    cfg = small_pixel_cfg()
    P = 2
    m = make_model(cfg, P, random_masks(P, cfg.L, cfg.M, cfg.N, with_edge=False))
    A = cfg.num_actions
    N = 3 * 64 + 21
    feat = (torch.randn(N, 256, device=DEV) * 0.5).to(torch.bfloat16)
    dlog = torch.randn(N, A, device=DEV) * 0.1
    dval = torch.randn(N, device=DEV) * 0.1
    gflat = torch.zeros_like(m.store.flat, requires_grad=False)
    dfeat = torch.zeros(N, 256, device=DEV)
    _lib.lib().heads_set_bwd_rows(rows)
    try:
        m.hip.heads_bwd(feat, dlog, dval, gflat, dfeat)
        torch.cuda.synchronize()
    finally:
        _lib.lib().heads_set_bwd_rows(32)            # the default
    flat = m.store.flat.detach().clone().requires_grad_(True)
    st = ParamStore(cfg, DEV, flat=flat)
    fx = feat.float().requires_grad_(True)
    l2, v2 = heads_ref(st, fx)
    ((l2 * dlog).sum() + (v2 * dval).sum()).backward()
    assert rel(dfeat, fx.grad) < 1e-4
    for name in ("policy.weight", "policy.bias", "value.weight", "value.bias"):
        s = m.store.layout.by_name[name]
        assert rel(gflat[s.offset:s.offset + s.numel], flat.grad[s.offset:s.offset + s.numel]) < 1e-4, (rows, name)


def test_rmsprop_kernel_matches_torch(hip_lib):
    from pathnet_gym_amd.algo.optim import RMSPropTF
    from pathnet_gym_amd.runtime.engine import HipEngine
    cfg = preset("pong")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 4, 16, 2
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    tr = PathNetTrainer(cfg, device=DEV)
    eng = tr.engine
    frozen = np.zeros((cfg.net.L, cfg.net.M), np.float32)
    frozen[0, 3] = 1
    tr.opt.set_frozen(frozen)
    eng.refresh_trainable()
    flat0 = tr.model.store.flat.detach().clone()
    g = torch.randn_like(flat0) * 3.0
    ref = RMSPropTF(tr.model.store.layout, flat0.clone(), clip_norm=40.0)
    ref.set_frozen(frozen)
    ref.ms.copy_(tr.opt.ms)
    ref.step(g, 7e-4)
    eng.grad_flat.copy_(g)
    eng.lr[0:1].fill_(7e-4)
    eng.lr[1:2].fill_(1.0)                 # skip flag (non-finite update): nothing may change
    ms0 = tr.opt.ms.clone()
    eng._optimizer_body()
    torch.cuda.synchronize()
    assert torch.equal(tr.model.store.flat.detach(), flat0) and torch.equal(tr.opt.ms, ms0)
    eng.lr[1:2].zero_()
    # a non-finite entry in a trainable segment: the kernel skips the whole step by itself and flags it
    gbad = g.clone()
    gbad[5] = float("nan")
    eng.grad_flat.copy_(gbad)
    eng._optimizer_body()
    torch.cuda.synchronize()
    assert torch.equal(tr.model.store.flat.detach(), flat0) and float(eng.opt_status) == 1.0
    eng.grad_flat.copy_(g)
    ms_before = tr.opt.ms.clone()
    eng._optimizer_body()
    torch.cuda.synchronize()
    assert float(eng.opt_status) == 0.0
    assert rel(tr.model.store.flat.detach() - flat0, ref.flat - flat0) < 1e-4
    s = tr.model.store.layout.by_name["layer0.module3.weight"]
    assert torch.equal(tr.model.store.flat[s.offset:s.offset + s.numel], flat0[s.offset:s.offset + s.numel])
    # deterministic: the same step from the same state is bit-identical (no atomics in the norm reduction)
    w1, m1 = tr.model.store.flat.detach().clone(), tr.opt.ms.clone()
    with torch.no_grad():
        tr.model.store.flat.copy_(flat0)
    tr.opt.ms.copy_(ms_before)
    eng._optimizer_body()
    torch.cuda.synchronize()
    assert torch.equal(tr.model.store.flat.detach(), w1) and torch.equal(tr.opt.ms, m1)
    # finite entries whose sum of squares overflows fp32: NOT skipped -- clip_by_norm scales that segment to 0
    # (tf.clip_by_norm's t * clip / max(inf, clip)) and every other segment steps normally
    s1 = tr.model.store.layout.by_name["layer1.module0.weight"]
    gbig = g.clone()
    gbig[s1.offset:s1.offset + 64] = 1e30
    with torch.no_grad():
        tr.model.store.flat.copy_(flat0)
    tr.opt.ms.copy_(ms_before)
    eng.grad_flat.copy_(gbig)
    eng._optimizer_body()
    torch.cuda.synchronize()
    assert float(eng.opt_status) == 0.0 and torch.isfinite(tr.model.store.flat).all()
    seg1 = slice(s1.offset, s1.offset + s1.numel)
    assert torch.equal(tr.model.store.flat[seg1], flat0[seg1])          # zero gradient, zero momentum
    assert torch.equal(tr.model.store.flat[:s1.offset], w1[:s1.offset])


def test_pong_env_hip_bit_exact_vs_torch(hip_lib):
    from pathnet_gym_amd.envs.pong import PongVec
    N = 24
    et = PongVec(N, device=DEV, seed=11, backend="torch")
    eh = PongVec(N, device=DEV, seed=11, backend="hip")
    ot = et.reset()
    oh = eh.reset()
    assert torch.equal(ot, oh)
    g = torch.Generator(device="cpu").manual_seed(0)
    ndone = 0
    for i in range(700):
        a = torch.randint(0, 6, (N,), generator=g).to(DEV)
        ot, rt, dt, it = et.step(a)
        oh, rh, dh, ih = eh.step(a)
        assert torch.equal(rt, rh), i
        assert torch.equal(dt, dh), i
        assert torch.equal(ot, oh), i
        assert torch.equal(it["episode_return"], ih["episode_return"]), i
        ndone += int(dt.sum())
    assert ndone > 0     # at least one auto-reset exercised


def test_pong_score_digits_every_score_bit_exact(hip_lib):
    """The score boxes come from per-score tables built once per env (csrc/envs.hip launch_pong_digit_tables): every
    score 0..20 on both sides renders as the torch game does, and the frame-ring kernel's batched quad walk writes
    the packed kernel's newest frame."""
    from pathnet_gym_amd.envs.pong import CS, PS, PongVec
    from pathnet_gym_amd.ops import envs as henv
    N = 42
    et = PongVec(N, device=DEV, seed=5, backend="torch")
    eh = PongVec(N, device=DEV, seed=5, backend="hip")
    er = PongVec(N, device=DEV, seed=5, backend="hip")
    idx = torch.arange(N, device=DEV)
    for e in (et, eh, er):
        e.reset()
        e.state[:, CS] = idx % 21
        e.state[:, PS] = (idx * 8 + 3) % 21
    for e in (eh, er):
        henv.pong_sync_to_device(e)
    g = torch.Generator(device="cpu").manual_seed(1)
    frames = torch.zeros(N, 2, 160 * 120, dtype=torch.uint8, device=DEV)
    fc_in = torch.zeros(N, dtype=torch.uint8, device=DEV)
    fc_out = torch.zeros_like(fc_in)
    for i in range(6):
        a = torch.randint(0, 6, (N,), generator=g).to(DEV)
        ot, rt, dt, _ = et.step(a)
        oh, rh, dh, _ = eh.step(a)
        r = torch.empty(N, device=DEV)
        d = torch.empty(N, dtype=torch.uint8, device=DEV)
        ep = torch.empty(N, device=DEV)
        er.step_ring_into(a.to(torch.int32).contiguous(), frames, 1, fc_in, fc_out, r, d, ep)
        torch.cuda.synchronize()
        assert torch.equal(ot, oh), i
        assert torch.equal(frames[:, 1], oh[..., 3].reshape(N, -1)), i
        assert torch.equal(r, rh) and torch.equal(d, dh.to(torch.uint8)), i
    assert len(set(er._st32[:, CS].tolist())) >= 20 and len(set(er._st32[:, PS].tolist())) >= 20


def test_cartpole_env_hip_vs_torch(hip_lib):
    from pathnet_gym_amd.envs.cartpole import CartPoleVec
    N = 64
    et = CartPoleVec(N, device=DEV, seed=3, backend="torch")
    eh = CartPoleVec(N, device=DEV, seed=3, backend="hip")
    ot, oh = et.reset(), eh.reset()
    assert torch.allclose(ot, oh)
    for i in range(8):
        a = (torch.arange(N, device=DEV) + i) % 2
        ot, rt, dt, _ = et.step(a)
        oh, rh, dh, _ = eh.step(a)
        assert torch.equal(dt, dh)
        assert torch.allclose(ot, oh, atol=1e-5)


@pytest.mark.parametrize("preset_name", ["pong", "cartpole"])
def test_engine_update_and_graph_replay(hip_lib, preset_name):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset(preset_name)
    cfg.paths = 4
    cfg.envs_per_path = 16
    cfg.a2c.t_max = 5
    cfg.use_graph = True
    tr = PathNetTrainer(cfg, device=DEV)
    w0 = tr.model.store.flat.detach().clone()
    for _ in range(4):          # eager, then capture, then replays
        st = tr.update()
        assert np.isfinite(st.loss_pi) and np.isfinite(st.loss_v)
    assert tr.engine.g_rollout is not None
    assert torch.isfinite(tr.model.store.flat).all()
    assert not torch.equal(w0, tr.model.store.flat.detach())
    assert tr.global_step == 4 * 4 * 16 * 5


def test_fast_conv_kernels_match_generic(hip_lib):
    """Compile-time-geometry conv kernels == generic runtime-geometry kernels."""
    from pathnet_gym_amd.ops import _lib
    cfg = small_pixel_cfg()
    P, E, T = 4, 16, 2
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, seed=9)
    m = make_model(cfg, P, masks, seed=11)
    g = torch.Generator(device="cpu").manual_seed(4)
    obs_steps = [torch.randint(0, 256, (P * E, 160, 120, 4), generator=g, dtype=torch.uint8).to(DEV)
                 for _ in range(T)]
    dfeat = torch.randn(T * P * E, 256, generator=g).to(DEV)
    lib = _lib.lib()
    lib.fast_conv_set_f16_fwd(0)        # the generic kernels use bf16 operands: compare like with like
    try:
        _lib.USE_FAST = False
        f0, g0 = _hip_trunk_fwd_bwd(m, obs_steps, dfeat, P, E)
        _lib.USE_FAST = True
        f1, g1 = _hip_trunk_fwd_bwd(m, obs_steps, dfeat, P, E)
    finally:
        _lib.USE_FAST = True
        lib.fast_conv_set_f16_fwd(1)
    assert torch.equal(f0, f1)          # same math, same rounding in the forward
    for s in m.store.layout.segments:
        if s.layer < 0 or s.layer > 2:
            continue
        a, b = g1[s.offset:s.offset + s.numel], g0[s.offset:s.offset + s.numel]
        if b.norm() < 1e-6:
            continue
        # layers 0-1 see dX from the MFMA (bf16-operand) dgrad instead of the fp32 VALU one
        assert rel(a, b) < (1e-3 if s.layer == 2 else 1e-2), (s.name, rel(a, b))


def test_engine_hybrid_lstm_reference_net(hip_lib):
    """Reference default net (L=4, M=10, N=4, LSTM 256): HIP trunk + fused HIP LSTM, graph-captured."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset("reference")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 4, 16, 4
    cfg.ga.B = 3
    tr = PathNetTrainer(cfg, device=DEV)
    assert tr.engine.lstm_hip and not tr.engine.hybrid and tr.engine.use_graph
    w0 = tr.model.store.flat.detach().clone()
    for _ in range(3):
        st = tr.update()
        assert np.isfinite(st.loss_pi)
    lay = tr.model.store.layout
    s = lay.by_name["lstm.kernel"]
    assert not torch.equal(w0[s.offset:s.offset + s.numel], tr.model.store.flat.detach()[s.offset:s.offset + s.numel])
    assert torch.isfinite(tr.model.store.flat).all()


def test_engine_torch_implemented_game(hip_lib):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset("atari4")
    cfg.tasks = ["Breakout", "SpaceInvaders"]
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 4, 16, 3
    tr = PathNetTrainer(cfg, device=DEV)
    assert tr.engine.use_graph                     # torch-logic games are capturable (in-place state, no syncs)
    for _ in range(3):
        st = tr.update()
        assert np.isfinite(st.loss_v)
    tr.end_task()
    tr._start_task(1)
    st = tr.update()
    assert np.isfinite(st.loss_v)


@pytest.mark.parametrize("graph,ring", [(False, True), (True, True), (False, False)])
def test_engine_gradient_matches_oracle(hip_lib, graph, ring):
    """Whole engine update == autograd of the A2C loss over the SAME stored rollout.

    Recomputes logits/values with the fp32 oracle from the engine's stored
    observations, rebuilds the n-step targets from the stored rewards/dones,
    and compares the full flat gradient (trunk modules + heads) with the
    engine's.  Catches wiring errors (step/slot/sample indexing) that the
    per-kernel tests cannot see.
    """
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.models.pathnet import ParamStore
    cfg = preset("pong")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 3, 16, 4
    cfg.use_graph = graph
    cfg.frame_ring = ring
    tr = PathNetTrainer(cfg, device=DEV)
    eng = tr.engine
    assert eng.ring == ring
    tr.env.max_episode_steps = 5           # episode resets inside the rollouts (frame-ring first-channel path)
    for _ in range(3 if graph else 1):     # with graphs: eager, capture, then a replayed update
        tr.update()
    T, P, E, B, A = eng.T, eng.P, eng.E, eng.B, eng.A
    obs0 = eng.obs_stack(0).clone()
    if graph:
        eng.rollout_backward()
    else:
        eng._rollout_backward_body()
    torch.cuda.synchronize()
    assert torch.equal(eng.obs_stack(0), obs0)
    assert eng.dones.any()
    a2c = cfg.a2c
    flat = tr.model.store.flat.detach().clone().requires_grad_(True)
    st = ParamStore(cfg.net, DEV, flat=flat)
    x = eng.obs_stacks().reshape((T + 1) * B, 160, 120, 4).float() / 255.0
    mask = tr.model.mask.repeat_interleave(E, 0).repeat(T + 1, 1, 1)
    feat = trunk_forward_ref(st, x, mask, emulate_bf16=True)
    logits, values = heads_ref(st, feat)
    test = f"engine_bf16_vs_emulated_{'graph' if graph else 'eager'}_{'ring' if ring else 'packed'}"
    budget.check(test + "_fwd", {"logits": rel(logits[:T * B], eng.logits[:T].reshape(-1, A)),
                                 "values": rel(values, eng.values[:T + 1].reshape(-1))}, 3e-2)
    R, adv = nstep_returns(eng.rewards, eng.values[:T], eng.dones.bool(), eng.values[T], a2c.gamma,
                           a2c.gae_lambda, a2c.reward_clip)
    loss, lp, lv, ent = a2c_loss(logits[:T * B], values[:T * B], eng.actions[:T].reshape(-1).long(), R.reshape(-1),
                                 adv.reshape(-1), a2c.entropy_beta, a2c.value_coef,
                                 torch.full((T * B,), eng.weight, device=DEV))
    loss.backward()
    g_ref, g_hip = flat.grad, eng.grad_flat
    errs = grad_errors(tr, g_hip, g_ref)
    print({k: round(v, 4) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])[:8]})
    budget.check(test, errs, 6e-2)
    if not graph and not ring and not os.environ.get("PATHNET_RECORD_NUMERICS") \
            and budget._load(budget.MEASURED).get(test):
        # negative control: a 2 % error in any layer's largest module breaks the budget
        neg = scaled_module_violations(tr, g_hip, g_ref, test, 6e-2)
        print("1.02-scaled module -> violations:", {k: len(v) for k, v in neg.items()})
        assert all(len(v) > 0 for v in neg.values()), neg


def grad_errors(tr, g_hip, g_ref, big=0.2):
    """{"layer<l>" / "policy" / "value": error of the group's whole gradient} + {segment: error} for segments
    carrying >= ``big`` x the largest segment gradient of their group (a module few rows reach is dominated by
    bf16 noise: its share of the layer error is what the layer key bounds)."""
    segs = tr.model.store.layout.segments
    key_of = lambda s: f"layer{s.layer}" if s.layer >= 0 else s.name.split(".")[0]      # noqa: E731
    top, parts, errs = {}, {}, {}
    for s in segs:
        top[key_of(s)] = max(top.get(key_of(s), 0.0), float(g_ref[s.offset:s.offset + s.numel].norm()))
    for s in segs:
        a, b = g_hip[s.offset:s.offset + s.numel], g_ref[s.offset:s.offset + s.numel]
        parts.setdefault(key_of(s), []).append((a, b))
        if b.norm() < 1e-7:
            assert a.norm() < 1e-4 * max(1.0, float(g_ref.norm())), s.name
            continue
        if float(b.norm()) >= big * top[key_of(s)]:
            errs[s.name] = rel(a, b)
    for k, v in parts.items():
        errs[k] = rel(torch.cat([a for a, _ in v]), torch.cat([b for _, b in v]))
    return errs


def scaled_module_violations(tr, g_hip, g_ref, test, fallback, factor=1.02):
    """Negative control: per layer, the largest active module's weight gradient x ``factor`` -> the budget
    violations it causes (must be non-empty for every layer)."""
    out = {}
    lay = tr.model.store.layout
    for l in range(tr.cfg.net.L):
        ws = [s for s in lay.segments if s.layer == l and s.name.endswith(".weight")]
        s = max(ws, key=lambda x: float(g_ref[x.offset:x.offset + x.numel].norm()))
        bad = g_hip.clone()
        bad[s.offset:s.offset + s.numel] *= factor
        out[s.name] = budget.violations(test, grad_errors(tr, bad, g_ref), fallback)
    return out


def test_engine_gradient_vs_plain_fp32_oracle(hip_lib):
    """Whole-update gradient of the bf16 HIP engine vs the fp32 autograd oracle WITHOUT bf16 emulation, at a
    small shape: every layer and every major segment within 3x its measured error (tests/numerics_budget.py)."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.models.pathnet import ParamStore
    cfg = preset("pong")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 3, 16, 4
    cfg.use_graph = False
    tr = PathNetTrainer(cfg, device=DEV)
    eng = tr.engine
    tr.env.max_episode_steps = 5
    tr.update()
    T, P, E, B, A = eng.T, eng.P, eng.E, eng.B, eng.A
    eng._rollout_backward_body()
    torch.cuda.synchronize()
    a2c = cfg.a2c
    flat = tr.model.store.flat.detach().clone().requires_grad_(True)
    st = ParamStore(cfg.net, DEV, flat=flat)
    x = eng.obs_stacks().reshape((T + 1) * B, 160, 120, 4).float() / 255.0
    mask = tr.model.mask.repeat_interleave(E, 0).repeat(T + 1, 1, 1)
    feat = trunk_forward_ref(st, x, mask)                 # plain fp32
    logits, values = heads_ref(st, feat)
    R, adv = nstep_returns(eng.rewards, eng.values[:T], eng.dones.bool(), eng.values[T], a2c.gamma,
                           a2c.gae_lambda, a2c.reward_clip)
    loss, lp, lv, ent = a2c_loss(logits[:T * B], values[:T * B], eng.actions[:T].reshape(-1).long(), R.reshape(-1),
                                 adv.reshape(-1), a2c.entropy_beta, a2c.value_coef,
                                 torch.full((T * B,), eng.weight, device=DEV))
    loss.backward()
    g_ref, g_hip = flat.grad, eng.grad_flat
    errs = grad_errors(tr, g_hip, g_ref)
    print("bf16 engine vs plain fp32 oracle:", {k: round(v, 5) for k, v in errs.items()})
    # bf16 rounding amplified through R - V makes some modules 5-20 % off the PLAIN fp32 gradient (measured,
    # tests/data/numerics_measured.json): this budget bounds that drift; the wiring check with a 2 % negative
    # control runs against the bf16-emulating oracle (test_engine_gradient_matches_oracle) and, for fp32-accurate
    # numbers, in tests/test_x3_engine.py / tests/test_f32_engine.py
    budget.check("engine_bf16_vs_plain_fp32", errs, 2.5e-1)


def test_bf16_conv_gradients_match_fp32(hip_lib):
    """engine.grads[0] / grads[1] in bf16 (the MFMA dgrads write them, the slab wgrads and the conv2 dgrad read
    them) vs fp32 buffers on the same rollout: only the bf16 rounding of dL/d(conv1 out), dL/d(conv2 out)
    separates them (every consumer rounds the masked gradient to bf16 for its MFMAs anyway)."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset("pong")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 3, 16, 4
    cfg.use_graph = False
    tr = PathNetTrainer(cfg, device=DEV)
    eng = tr.engine
    assert [g.dtype for g in eng.grads[:3]] == [torch.bfloat16, torch.bfloat16, torch.float32] and not eng.ring
    tr.update()
    eng._rollout_backward_body()
    torch.cuda.synchronize()
    g_bf = eng.grad_flat.clone()
    acts_bf = [g.float().clone() for g in eng.grads[:2]]
    eng.grads = [torch.zeros(g.shape, dtype=torch.float32, device=DEV) for g in eng.grads]
    eng.grad_flat.zero_()
    T, B, L = eng.T, eng.B, len(tr.model.hip.geoms)
    tr.model.hip.heads_bwd(eng.acts[L - 1][:T].reshape(T * B, -1), eng.dlogits.reshape(T * B, -1),
                           eng.dvalue.reshape(-1), eng.grad_flat, eng.grads[L - 1], task=tr.model.task)
    eng._layer_bwd_all(T)
    torch.cuda.synchronize()
    budget.check("bf16_conv_act_grads", {"grads1": rel(acts_bf[1], eng.grads[1]),
                                         "grads0": rel(acts_bf[0], eng.grads[0])}, 1e-2)
    errs = {}
    for s in tr.model.store.layout.segments:
        a, b = g_bf[s.offset:s.offset + s.numel], eng.grad_flat[s.offset:s.offset + s.numel]
        if b.norm() < 1e-7:
            assert a.norm() < 1e-5, s.name
            continue
        errs[s.name] = rel(a, b)
    budget.check("bf16_conv_act_grads_wgrad", errs, 2e-2)


@pytest.mark.parametrize("split", ["1", "2", "4"])
def test_frame_ring_stacks_match_packed_env(hip_lib, monkeypatch, split):
    """Frame-ring rollout (single-frame writes + first-valid-channel bytes) reproduces, bit for bit,
    the packed 4-frame stacks the packed Pong kernel produces for the same actions, resets included -- with the fused
    ring kernel (split 1) and the physics + split-render launches (csrc/envs.hip launch_pong_step_ring_split)."""
    monkeypatch.setenv("PATHNET_PONG_SPLIT", split)
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.ops import envs as henv
    cfg = preset("pong")
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 3, 16, 7
    cfg.use_graph = False
    cfg.frame_ring = True
    tr = PathNetTrainer(cfg, device=DEV)
    eng, env = tr.engine, tr.env
    assert eng.ring
    env.max_episode_steps = 3
    tr.update()
    torch.cuda.synchronize()
    st0, ctr0 = env._st32.clone(), env._ctr32.clone()
    cur = eng.obs_stack(0).clone()
    eng._rollout_backward_body()
    torch.cuda.synchronize()
    st_eng, ctr_eng = env._st32, env._ctr32
    env._st32, env._ctr32 = st0, ctr0
    B = eng.B
    try:
        for t in range(eng.T):
            nxt = torch.empty_like(cur)
            r = torch.empty(B, device=DEV)
            d = torch.empty(B, dtype=torch.uint8, device=DEV)
            e = torch.empty(B, device=DEV)
            henv.pong_step_into(env, eng.actions[t].contiguous(), cur, nxt, r, d, e)
            torch.cuda.synchronize()
            assert torch.equal(d, eng.dones[t]), t
            assert torch.equal(r, eng.rewards[t]), t
            assert torch.equal(nxt, eng.obs_stack(t + 1)), t
            cur = nxt
        assert eng.dones.any()
        assert torch.equal(env._st32, st_eng)
    finally:
        env._st32, env._ctr32 = st_eng, ctr_eng


def test_lstm_cell_kernels_match_autograd(hip_lib):
    """Fused LSTM fwd / bwd-step / wgrad kernels vs TF BasicLSTMCell semantics in fp32 autograd."""
    from pathnet_gym_amd.models.pathnet import ParamStore, bf16_ste, lstm_cell_ref
    cfg = preset("reference").net
    P, B = 3, 96                                   # B not a multiple of the 64-row tile
    m = make_model(cfg, P, random_masks(P, cfg.L, cfg.M, cfg.N, with_edge=False))
    hp = m.hip
    F, H = hp.lstm["F"], hp.lstm["H"]
    g = torch.Generator(device="cpu").manual_seed(3)
    x = (torch.randn(B, F, generator=g) * 0.5).to(DEV).to(torch.bfloat16)
    h = (torch.randn(B, H, generator=g) * 0.5).to(DEV).to(torch.bfloat16)
    c = torch.randn(B, H, generator=g).to(DEV)
    done = (torch.rand(B, generator=g) < 0.3).to(torch.uint8).to(DEV)
    hout = torch.zeros(B, H, dtype=torch.bfloat16, device=DEV)
    cout = torch.zeros(B, H, device=DEV)
    gates = torch.zeros(B, 4 * H, device=DEV)
    xh = torch.zeros(B, F + H, dtype=torch.bfloat16, device=DEV)
    hp.lstm_fwd(x, h, c, done, hout, cout, gates, xh)
    torch.cuda.synchronize()
    flat = m.store.flat.detach().clone().requires_grad_(True)
    st = ParamStore(cfg, DEV, flat=flat)
    k, b = st.lstm()
    keep = (1.0 - done.float())[:, None]
    xr = x.float().requires_grad_(True)
    hin = (h.float() * keep).requires_grad_(True)
    h2, c2 = lstm_cell_ref(xr, hin, c * keep, bf16_ste(k), b)
    errs = {"h": rel(hout.float(), h2.detach()), "c": rel(cout, c2.detach())}
    assert torch.equal(xh[:, :F], x) and torch.equal(xh[:, F:].float(), hin.detach().to(torch.bfloat16).float())
    dh = torch.randn(B, H, generator=g).to(DEV)
    (h2 * dh).sum().backward()
    dz = torch.zeros(B, 4 * H, device=DEV)
    dc_out = torch.zeros(B, H, device=DEV)
    dx = torch.zeros(B, F, device=DEV)
    dh_prev = torch.zeros(B, H, device=DEV)
    gflat = torch.zeros_like(m.store.flat, requires_grad=False)
    hp.lstm_bwd_step(dh, None, None, None, gates, cout, c, done, dz, dc_out, dx, dh_prev)
    hp.lstm_wgrad(xh, dz, gflat, rows_per_chunk=32)
    torch.cuda.synchronize()
    errs["dx"] = rel(dx, xr.grad)
    errs["dh_prev"] = rel(dh_prev, hin.grad)
    lay = m.store.layout
    for name in ("lstm.kernel", "lstm.bias"):
        s_ = lay.by_name[name]
        errs[name] = rel(gflat[s_.offset:s_.offset + s_.numel], flat.grad[s_.offset:s_.offset + s_.numel])
    print("lstm cell kernels:", errs)
    budget.check("lstm_cell_kernels", errs, 2e-2)


def test_engine_lstm_gradient_matches_oracle(hip_lib):
    """LSTM engine update (carried state, episode resets) == autograd over the stored rollout."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.models.pathnet import ParamStore, bf16_ste, lstm_cell_ref
    cfg = preset("reference")
    cfg.tasks = ["Pong"]
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 3, 16, 5
    tr = PathNetTrainer(cfg, device=DEV)
    eng = tr.engine
    assert eng.lstm_hip
    for _ in range(3):
        tr.update()
    T, P, E, B, A = eng.T, eng.P, eng.E, eng.B, eng.A
    h0, c0 = eng.hst[0].float().clone(), eng.cst[0].clone()
    eng.rollout_backward()
    torch.cuda.synchronize()
    a2c = cfg.a2c
    flat = tr.model.store.flat.detach().clone().requires_grad_(True)
    st = ParamStore(cfg.net, DEV, flat=flat)
    k, bb = st.lstm()
    kq = bf16_ste(k)
    x = eng.obs_stacks().reshape((T + 1) * B, 160, 120, 4).float() / 255.0
    mask = tr.model.mask.repeat_interleave(E, 0).repeat(T + 1, 1, 1)
    feat = trunk_forward_ref(st, x, mask, emulate_bf16=True).view(T + 1, B, -1)
    h, c = h0, c0
    hs = []
    for t in range(T + 1):
        if t > 0:
            keep = (1.0 - eng.dones[t - 1].float())[:, None]
            h, c = h * keep, c * keep
        h, c = lstm_cell_ref(bf16_ste(feat[t]), bf16_ste(h), c, kq, bb)
        hs.append(h)
    logits, values = heads_ref(st, bf16_ste(torch.stack(hs)).reshape((T + 1) * B, -1))
    budget.check("engine_lstm_fwd", {"logits": rel(logits[:T * B], eng.logits[:T].reshape(-1, A))}, 3e-2)
    R, adv = nstep_returns(eng.rewards, eng.values[:T], eng.dones.bool(), eng.values[T], a2c.gamma,
                           a2c.gae_lambda, a2c.reward_clip)
    loss, _, _, _ = a2c_loss(logits[:T * B], values[:T * B], eng.actions[:T].reshape(-1).long(), R.reshape(-1),
                             adv.reshape(-1), a2c.entropy_beta, a2c.value_coef,
                             torch.full((T * B,), 1.0 / E, device=DEV))
    loss.backward()
    errs = grad_errors(tr, eng.grad_flat, flat.grad)
    print({k_: round(v, 4) for k_, v in sorted(errs.items(), key=lambda kv: -kv[1])[:8]})
    budget.check("engine_lstm", errs, 8e-2)


@pytest.fixture(scope="module", params=["eager", "graph"])
def lstm_dones_rollout(hip_lib, request):
    """The `reference` preset in bf16 (Pong, 3 paths x 16 envs, t_max = 5) with episodes capped at 3 agent steps, a
    period coprime to t_max, so every rollout has episode ends at interior steps and at its last step.  The per-env
    step counters (column STEPS of the Pong state tensor) are offset by env % 3 before the first update, so the rows
    end their episodes at different steps.  "graph": hipGraph capture + replays, the last replay is the one compared.
    -> the engine's gradient, the oracle's (bf16-emulating trunk, lstm_cell_ref with keep from eng.dones, a2c_loss)
    and two wrong oracles: keep forced to 1, and dones[t] in place of dones[t-1]."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    from pathnet_gym_amd.envs.pong import STEPS
    from pathnet_gym_amd.models.pathnet import ParamStore, bf16_ste, lstm_cell_ref
    from pathnet_gym_amd.ops import envs as henv
    graph = request.param == "graph"
    cfg = preset("reference")
    cfg.tasks = ["Pong"]
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 3, 16, 5
    cfg.use_graph = graph
    tr = PathNetTrainer(cfg, device=DEV)
    eng, env = tr.engine, tr.env
    assert eng.lstm_hip and not eng.hybrid and eng.hst.dtype == torch.bfloat16 and eng.use_graph == graph
    env.max_episode_steps = 3
    if not hasattr(env, "_st32"):
        henv.pong_sync_to_device(env)
    env._st32[:, STEPS] += (torch.arange(eng.B, device=DEV) % 3).to(torch.int32)     # in place: the graphs keep it
    for _ in range(3 if graph else 2):
        tr.update()
    tr.flush()
    torch.cuda.synchronize()
    assert not graph or eng.g_rollout is not None
    T, P, E, B, A = eng.T, eng.P, eng.E, eng.B, eng.A
    ended = eng.dones[T - 1].bool().clone()              # the previous rollout's last step
    h0, c0 = eng.hst[0].float().clone(), eng.cst[0].clone()
    # the carry's job: the state entering the rollout is zero where the previous rollout ended an episode
    assert ended.any() and not ended.all()
    assert not h0[ended].any() and not c0[ended].any()
    assert bool((h0[~ended].abs().sum(1) > 0).all()) and bool((c0[~ended].abs().sum(1) > 0).all())
    eng.rollout_backward()
    torch.cuda.synchronize()
    dones = eng.dones.bool()
    assert dones[:T - 1].any() and dones[T - 1].any()
    assert len({tuple(r) for r in dones.t().tolist()}) >= 3            # the rows end at different steps
    a2c = cfg.a2c
    flat = tr.model.store.flat.detach().clone().requires_grad_(True)
    st = ParamStore(cfg.net, DEV, flat=flat)
    k, bb = st.lstm()
    kq = bf16_ste(k)
    x = eng.obs_stacks().reshape((T + 1) * B, 160, 120, 4).float() / 255.0
    mask = tr.model.mask.repeat_interleave(E, 0).repeat(T + 1, 1, 1)
    feat = trunk_forward_ref(st, x, mask, emulate_bf16=True).view(T + 1, B, -1)
    R, adv = nstep_returns(eng.rewards, eng.values[:T], eng.dones.bool(), eng.values[T], a2c.gamma,
                           a2c.gae_lambda, a2c.reward_clip)

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
        return logits.detach(), torch.autograd.grad(loss, flat, retain_graph=True)[0]

    kf = 1.0 - eng.dones.float()
    logits, g_ref = oracle(lambda t: kf[t - 1])
    _, g_keep1 = oracle(lambda t: torch.ones_like(kf[0]))
    _, g_shift = oracle(lambda t: kf[min(t, T - 1)])       # the bootstrap step (t = T) has no dones[T]: it keeps T-1's
    return dict(mode=request.param, tr=tr, eng=eng, logits=logits, g_ref=g_ref, g_hip=eng.grad_flat.clone(),
                g_keep1=g_keep1, g_shift=g_shift)


def test_engine_lstm_gradient_with_episode_ends(lstm_dones_rollout):
    """The bf16 reverse scan with episode ends inside the rollout and at its last step: the done mask on the
    recurrent gradients (kt), the dh_rec / dc_rec ping-pong, which dones[t] goes to which step, and the carry's
    reset == autograd over the stored rollout.  Negative controls from the oracle alone: a recurrence that ignores
    the episode ends, and one that uses dones[t] where dones[t-1] belongs, must both leave the budget this test
    applies to the LSTM gradient -- a budget that could not see the mask would be of no use."""
    r = lstm_dones_rollout
    tr, eng = r["tr"], r["eng"]
    T, B, A = eng.T, eng.B, eng.A
    budget.check("engine_lstm_dones_fwd", {"logits": rel(r["logits"][:T * B], eng.logits[:T].reshape(-1, A))}, 3e-2)
    errs = grad_errors(tr, r["g_hip"], r["g_ref"])
    print(r["mode"], {k_: round(v, 4) for k_, v in sorted(errs.items(), key=lambda kv: -kv[1])[:8]})
    assert "lstm" in errs
    ctrl = {name: grad_errors(tr, r[name], r["g_ref"])["lstm"] for name in ("g_keep1", "g_shift")}
    print("lstm error of the wrong oracles:", ctrl, "of the engine:", errs["lstm"])
    budget.check("engine_lstm_dones", errs, 8e-2)
    rec = budget._load(budget.MEASURED).get("engine_lstm_dones", {}).get("lstm")
    applied = 8e-2 if rec is None or os.environ.get("PATHNET_RECORD_NUMERICS") else budget.HEADROOM * max(rec, 1e-5)
    for name, v in ctrl.items():
        assert v > max(applied, 8e-2), (name, v, applied)


@pytest.mark.parametrize("E", [16, 32])
def test_slab_conv_kernels_match_fast(hip_lib, E):
    """LDS-slab implicit-im2col conv fwd/wgrad == the register-im2col fast kernels (all-active path included)."""
    from pathnet_gym_amd.ops import _lib
    cfg = small_pixel_cfg()
    P, T = 3, 2
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, seed=21)          # path 1: all 10 modules active
    m = make_model(cfg, P, masks, seed=5)
    g = torch.Generator(device="cpu").manual_seed(8)
    obs_steps = [torch.randint(0, 256, (P * E, 160, 120, 4), generator=g, dtype=torch.uint8).to(DEV)
                 for _ in range(T)]
    dfeat = torch.randn(T * P * E, 256, generator=g).to(DEV)
    lib = _lib.lib()
    try:
        lib.fast_conv_set_f16_fwd(0)      # the slab forward has bf16 operands: compare like with like
        lib.fast_conv_set_slab(0)
        lib.fast_conv_set_slab_fwd(0)
        f0, g0 = _hip_trunk_fwd_bwd(m, obs_steps, dfeat, P, E)
        lib.fast_conv_set_slab(1)
        lib.fast_conv_set_slab_fwd(1)
        f1, g1 = _hip_trunk_fwd_bwd(m, obs_steps, dfeat, P, E)
    finally:
        lib.fast_conv_set_slab(1)
        lib.fast_conv_set_slab_fwd(0)
        lib.fast_conv_set_f16_fwd(1)
    assert rel(f1, f0) < 1e-3
    for s in m.store.layout.segments:
        if s.layer < 0 or s.layer > 2:
            continue
        a, b = g1[s.offset:s.offset + s.numel], g0[s.offset:s.offset + s.numel]
        if b.norm() < 1e-6:
            assert a.norm() < 1e-6, s.name
            continue
        assert rel(a, b) < 2e-3, (s.name, rel(a, b))


@pytest.mark.parametrize("nt,pf", [(2, 2), (8, 1), (16, 2)])
def test_conv_pipeline_variants_match_default(hip_lib, nt, pf):
    """conv_fwd_fast with 2/8/16 row tiles per wave and the 1- / 2-deep-prefetch slab wgrad == the default kernels."""
    from pathnet_gym_amd.ops import _lib
    cfg = small_pixel_cfg()
    P, T, E = 3, 3, 16
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, seed=21)          # path 1: all 10 modules active
    m = make_model(cfg, P, masks, seed=5)
    g = torch.Generator(device="cpu").manual_seed(9)
    obs_steps = [torch.randint(0, 256, (P * E, 160, 120, 4), generator=g, dtype=torch.uint8).to(DEV)
                 for _ in range(T)]
    dfeat = torch.randn(T * P * E, 256, generator=g).to(DEV)
    lib = _lib.lib()
    f0, g0 = _hip_trunk_fwd_bwd(m, obs_steps, dfeat, P, E)
    try:
        lib.fast_conv_set_fwd_nt(nt)
        lib.fast_conv_set_wgrad_pf(pf)
        f1, g1 = _hip_trunk_fwd_bwd(m, obs_steps, dfeat, P, E)
    finally:
        lib.fast_conv_set_fwd_nt(4)
        lib.fast_conv_set_wgrad_pf(2)     # the default (csrc/conv_fast.hip WGRAD_PF)
    assert rel(f1, f0) < 1e-5
    for s in m.store.layout.segments:
        if s.layer < 0 or s.layer > 2:
            continue
        a, b = g1[s.offset:s.offset + s.numel], g0[s.offset:s.offset + s.numel]
        if b.norm() < 1e-6:
            assert a.norm() < 1e-6, s.name
            continue
        assert rel(a, b) < 1e-4, (s.name, rel(a, b))


def test_device_ga_matches_host_mirror(hip_lib):
    """csrc/ga.hip tournament + mutation + redraw == algo/ga_device.CounterPopulation, step by step;
    compaction == compact_active + the host inverse lists."""
    from pathnet_gym_amd.algo.ga import compact_active
    from pathnet_gym_amd.algo.ga_device import CounterPopulation
    from pathnet_gym_amd.ops import _lib
    P, L, M, N, B, C = 40, 5, 10, 4, 3, 6
    pop = CounterPopulation(P, L, M, N, B, seed=3, concurrent=C)
    pop.frozen[2, 7] = 1
    geno = torch.from_numpy(pop.genotypes.astype(np.uint8)).to(DEV)
    frozen = torch.from_numpy(pop.frozen.astype(np.uint8)).to(DEV)
    slots = torch.from_numpy(pop.slots.astype(np.int32)).to(DEV)
    gen = torch.zeros(1, dtype=torch.int64, device=DEV)
    events = torch.zeros(C, 3, dtype=torch.int32, device=DEV)
    rng = np.random.RandomState(0)
    fired = 0
    for t in range(80):
        f = pop.fitness.copy()
        fresh = rng.rand(P) < 0.35
        f[fresh] = rng.randint(-21, 22, int(fresh.sum())).astype(np.float32)
        fit = torch.from_numpy(f).to(DEV)
        evs = pop.step(f, t)
        fired += len(evs)
        reset = torch.full((P,), 7, dtype=torch.uint8, device=DEV)
        _lib.call("launch_ga_step", geno.data_ptr(), fit.data_ptr(), slots.data_ptr(), gen.data_ptr(),
                  events.data_ptr(), P, L, M, N, B, C, pop.seed32, reset.data_ptr(), _lib.stream())
        torch.cuda.synchronize()
        want = np.zeros(P, np.uint8)
        for e in evs:
            want[e.candidates] = 1
        assert np.array_equal(reset.cpu().numpy(), want), t          # exactly the fired candidates restart
        assert np.array_equal(geno.cpu().numpy(), pop.genotypes.astype(np.uint8)), t
        assert np.array_equal(slots.cpu().numpy(), pop.slots.astype(np.int32)), t
        assert np.array_equal(fit.cpu().numpy(), pop.fitness), t
        assert int(gen) == pop.generation
    assert fired > 30
    Pl, off = 16, 8
    mask = torch.zeros(Pl, L, M, device=DEV)
    ai = torch.zeros(Pl, L, M, dtype=torch.int32, device=DEV)
    ac = torch.zeros(Pl, L, dtype=torch.int32, device=DEV)
    ip = torch.zeros(L, M, Pl, dtype=torch.int32, device=DEV)
    isl = torch.zeros_like(ip)
    ic = torch.zeros(L, M, dtype=torch.int32, device=DEV)
    _lib.call("launch_ga_compact", geno.data_ptr(), frozen.data_ptr(), off, Pl, L, M, mask.data_ptr(), ai.data_ptr(),
              ac.data_ptr(), ip.data_ptr(), isl.data_ptr(), ic.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    expr = pop.expressed()[off:off + Pl]
    idx, cnt = compact_active(expr)
    assert np.array_equal(mask.cpu().numpy(), expr)
    assert np.array_equal(ai.cpu().numpy(), idx) and np.array_equal(ac.cpu().numpy(), cnt)
    for l in range(L):
        for j in range(M):
            users = [p for p in range(Pl) if expr[p, l, j] > 0.5]
            assert int(ic[l, j]) == len(users)
            assert ip[l, j, :len(users)].tolist() == users
            assert isl[l, j, :len(users)].tolist() == [int(expr[p, l, :j].sum()) for p in users]
    # more than one 64-path wave chunk per module (the inverse lists are built with ballots)
    big = CounterPopulation(150, L, M, N, B, seed=5, concurrent=C)
    gb = torch.from_numpy(big.genotypes.astype(np.uint8)).to(DEV)
    fb = torch.from_numpy(big.frozen.astype(np.uint8)).to(DEV)
    Pl = 150
    mask = torch.zeros(Pl, L, M, device=DEV)
    ai = torch.zeros(Pl, L, M, dtype=torch.int32, device=DEV)
    ac = torch.zeros(Pl, L, dtype=torch.int32, device=DEV)
    ip = torch.full((L, M, Pl), -5, dtype=torch.int32, device=DEV)
    isl = torch.full_like(ip, -5)
    ic = torch.zeros(L, M, dtype=torch.int32, device=DEV)
    _lib.call("launch_ga_compact", gb.data_ptr(), fb.data_ptr(), 0, Pl, L, M, mask.data_ptr(), ai.data_ptr(),
              ac.data_ptr(), ip.data_ptr(), isl.data_ptr(), ic.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    expr = big.expressed()
    for l in range(L):
        for j in range(M):
            users = [p for p in range(Pl) if expr[p, l, j] > 0.5]
            assert int(ic[l, j]) == len(users)
            assert ip[l, j, :len(users)].tolist() == users
            assert isl[l, j, :len(users)].tolist() == [int(expr[p, l, :j].sum()) for p in users]
            assert (ip[l, j, len(users):] == 0).all() and (isl[l, j, len(users):] == 0).all()


def test_trainer_device_ga_stays_in_sync(hip_lib):
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    cfg = preset("cartpole")                       # short episodes -> many tournaments
    cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 8, 16, 5
    cfg.ga.backend = "device"
    cfg.ga.concurrent_tournaments = 2
    tr = PathNetTrainer(cfg, device=DEV)
    for _ in range(60):
        tr.update()
    tr.flush()                                     # the host mirror runs one update behind when pipelined
    torch.cuda.synchronize()
    g = tr.engine.ga_dev
    assert tr.pop.generation > 0
    assert np.array_equal(g["geno"].cpu().numpy(), tr.pop.genotypes.astype(np.uint8))
    assert np.array_equal(tr.model.mask.cpu().numpy(), tr.pop.expressed())


@pytest.mark.parametrize("layer", [1, 2])
def test_dgrad_mfma_matches_valu(hip_lib, layer):
    """Superpixel MFMA conv dgrad == the fp32 VALU dgrad (bf16 operand rounding only)."""
    from pathnet_gym_amd.ops import _lib
    cfg = small_pixel_cfg()
    P, E, T = 3, 16, 2
    masks = random_masks(P, cfg.L, cfg.M, cfg.N, seed=4)          # includes an all-active and an empty layer
    m = make_model(cfg, P, masks, seed=6)
    hp = m.hip
    g = hp.geoms[layer]
    B = P * E
    G = torch.randn(T * B, g.out_feat, generator=torch.Generator().manual_seed(2)).to(DEV)
    bits, rows = hp.alloc_bits(layer, T, B)
    bits.copy_(torch.randint(0, 256, bits.shape, generator=torch.Generator().manual_seed(3)).to(torch.uint8).to(DEV))
    lib = _lib.lib()
    outs = []
    for on in (0, 1):
        dX = torch.zeros(T * B, g.Hin * g.Win * g.Cin, device=DEV)
        lib.fast_conv_set_dgrad_mfma(on)
        try:
            assert _lib.call_fast("fast_conv_dgrad", G.data_ptr(), bits.data_ptr(), m.store.flat.data_ptr(), g.w_off,
                                  g.chunk, m.act_idx.data_ptr(), m.act_cnt.data_ptr(), layer, hp.L, hp.M, g.Hin,
                                  g.Win, g.Cin, g.KH, g.KW, g.S, P, E, T, rows, 1.0, dX.data_ptr(), _lib.stream())
        finally:
            lib.fast_conv_set_dgrad_mfma(1)
        torch.cuda.synchronize()
        outs.append(dX)
    assert rel(outs[1], outs[0]) < 1e-2


def test_pipelined_update_matches_synchronous(hip_lib):
    """Pipelined host bookkeeping (device GA): the host mirror catches up exactly after flush(), step
    accounting matches the synchronous loop.  (Weights are not compared bit-for-bit: the split-R wgrad
    kernels accumulate with fp32 atomics, so two runs differ in the last bits and may diverge.)"""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer
    res = []
    for pipe in (False, True):
        cfg = preset("cartpole")
        cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 8, 16, 5
        cfg.ga.backend = "device"
        cfg.ga.concurrent_tournaments = 2
        cfg.pipeline = pipe
        tr = PathNetTrainer(cfg, device=DEV)
        assert tr.pipelined == pipe
        stats = [tr.update() for _ in range(30)]
        last = tr.flush()
        torch.cuda.synchronize()
        if pipe:
            assert np.isnan(stats[0].loss_pi) and last is not None and np.isfinite(last.loss_pi)
        g = tr.engine.ga_dev
        assert np.array_equal(g["geno"].cpu().numpy(), tr.pop.genotypes.astype(np.uint8))
        assert np.array_equal(g["slots"].cpu().numpy(), tr.pop.slots.astype(np.int32))
        assert int(g["gen"]) == tr.pop.generation > 0
        assert torch.isfinite(tr.model.store.flat).all()
        res.append(tr.global_step)
    assert res[0] == res[1] == 30 * 8 * 16 * 5


def test_image_staged_conv1_fwd_matches_fast(hip_lib):
    """Whole-image-staged first-layer forward == register-im2col forward (bit-exact outputs and ReLU bits)."""
    from pathnet_gym_amd.ops import _lib
    cfg = small_pixel_cfg()
    P, E = 3, 32
    m = make_model(cfg, P, random_masks(P, cfg.L, cfg.M, cfg.N, seed=12), seed=2)
    hp = m.hip
    g = hp.geoms[0]
    x = torch.randint(0, 256, (P * E, 160, 120, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(DEV)
    lib = _lib.lib()
    outs = []
    for on in (0, 1):
        Y = torch.zeros(P * E, g.out_feat, dtype=torch.bfloat16, device=DEV)
        bits, rows = hp.alloc_bits(0, 1, P * E)
        lib.fast_conv_set_img_fwd(on)
        lib.fast_conv_set_f16_fwd(0)      # the image-staged forward has bf16 operands
        try:
            hp.layer_fwd(0, x, Y, bits, P, E, 1, 0, rows)
        finally:
            lib.fast_conv_set_img_fwd(0)
            lib.fast_conv_set_f16_fwd(1)
        torch.cuda.synchronize()
        outs.append((Y, bits))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("game", ["Breakout", "SpaceInvaders", "Alien", "MsPacman", "Centipede"])
def test_rect_scene_render_kernel_bit_exact(hip_lib, game):
    """HIP rectangle rasteriser + gray + bilinear resize + stack push == the torch renderer/preprocess oracle."""
    from pathnet_gym_amd.envs.registry import make
    envs = [make(game, num_envs=24, device=DEV, seed=5, backend=b) for b in ("torch", "hip")]
    o0, o1 = envs[0].reset(), envs[1].reset()
    assert torch.equal(o0, o1)
    g = torch.Generator().manual_seed(0)
    for t in range(40):
        a = torch.randint(0, envs[0].num_actions, (24,), generator=g).to(DEV)
        r = [e.step(a) for e in envs]
        assert torch.equal(r[0][0], r[1][0]), t
        assert torch.equal(r[0][2], r[1][2]) and torch.equal(r[0][1], r[1][1])


def test_rgb_stack_push_matches_oracle(hip_lib):
    """Standalone RGB -> gray -> resize -> stack push kernel (external frames) == preprocess_frames + push."""
    from pathnet_gym_amd.envs.pong import preprocess_frames, resize_tables
    from pathnet_gym_amd.ops.envs import rgb_stack_push
    N = 10
    g = torch.Generator().manual_seed(0)
    rgb = torch.randint(0, 256, (N, 210, 160, 3), dtype=torch.uint8, generator=g).to(DEV)
    obs_in = torch.randint(0, 256, (N, 160, 120, 4), dtype=torch.uint8, generator=g).to(DEV)
    reset = torch.tensor([i % 3 == 0 for i in range(N)], device=DEV)
    out = torch.empty_like(obs_in)
    tabs = torch.from_numpy(resize_tables()).to(DEV)
    for gray in ("rgb", "bgr"):
        rgb_stack_push(rgb, obs_in, out, reset, tabs, gray)
        f = preprocess_frames(rgb, tabs, gray)
        ref = torch.where(reset[:, None, None, None], f[..., None].expand(-1, -1, -1, 4),
                          torch.cat([obs_in[..., 1:], f[..., None]], 3))
        assert torch.equal(out, ref), gray


@pytest.mark.parametrize("game", ["Breakout", "Centipede"])
def test_torch_game_step_replays_in_hipgraph(hip_lib, game):
    """A torch-logic game step captured once and replayed == the same game stepped eagerly."""
    from pathnet_gym_amd.envs.registry import make
    N = 32
    ea = make(game, num_envs=N, device=DEV, seed=9, backend="hip")
    eb = make(game, num_envs=N, device=DEV, seed=9, backend="hip")
    oa = ea.reset()
    eb.reset()
    A = eb.num_actions
    act = torch.zeros(N, dtype=torch.int32, device=DEV)
    obs_in = eb.obs.clone().reshape(N, -1)
    obs_out = torch.empty_like(obs_in)
    rew = torch.zeros(N, device=DEV)
    done = torch.zeros(N, dtype=torch.uint8, device=DEV)
    epr = torch.zeros(N, device=DEV)
    g = torch.Generator().manual_seed(3)
    seq = [torch.randint(0, A, (N,), generator=g).to(torch.int32).to(DEV) for _ in range(25)]
    # first step eager on both (warm-up, lazily built caches), then capture eb's step
    oa, ra, da, _ = ea.step(seq[0])
    act.copy_(seq[0])
    eb.step_into(act, obs_in, obs_out, rew, done, epr)
    assert torch.equal(obs_out.view_as(oa), oa)
    obs_in.copy_(obs_out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        eb.step_into(act, obs_in, obs_out, rew, done, epr)
    torch.cuda.synchronize()
    for t in range(1, 25):
        oa, ra, da, _ = ea.step(seq[t])
        act.copy_(seq[t])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(obs_out.view_as(oa), oa), t
        assert torch.equal(rew, ra) and torch.equal(done.bool(), da), t
        obs_in.copy_(obs_out)


def _typed_vs_oracle(cfg, P, rpp, din_shape, seed, tol):
    from pathnet_gym_amd.models.pathnet import ParamStore
    from pathnet_gym_amd.ops.typed_fc import typed_trunk_forward
    st = ParamStore(cfg, torch.device(DEV), seed=3)
    masks = torch.from_numpy(random_masks(P, cfg.L, cfg.M, cfg.N, seed=seed)).float().to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(1000 + seed)      # seeded: the same inputs every run
    x = torch.rand(P * rpp, *din_shape, device=DEV, generator=gen)
    flat_h = st.flat.detach().clone().requires_grad_(True)
    st.flat = flat_h
    yh = typed_trunk_forward(st, x, masks, rpp)
    w = torch.randn(yh.shape, device=DEV, generator=gen)
    (yh * w).sum().backward()
    # the oracle in float64 (the GPU's fp32 library GEMMs carry ~1e-5 of their own error on the 3072-wide layer,
    # which made this comparison fail now and then against an fp32 oracle)
    flat_r = flat_h.detach().double().requires_grad_(True)
    st.flat = flat_r
    yr = trunk_forward_ref(st, x.double(), masks.double().repeat_interleave(rpp, 0))
    (yr * w.double()).sum().backward()
    assert rel(yh, yr) < tol
    assert rel(flat_h.grad, flat_r.grad) < tol
    # per segment too: every active module's weight and bias gradient
    for s in st.layout.segments:
        if s.layer >= 0:
            b = flat_r.grad[s.offset:s.offset + s.numel]
            if float(b.norm()) > 0:
                assert rel(flat_h.grad[s.offset:s.offset + s.numel], b) < 10 * tol, s.name
    # inactive modules get exactly zero gradient
    inactive = (masks.sum(0) == 0).cpu().numpy()
    for s in st.layout.segments:
        if s.layer >= 0 and inactive[s.layer, s.module]:
            assert float(flat_h.grad[s.offset:s.offset + s.numel].abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["never", "always"], ids=["valu", "mfma"])
@pytest.mark.parametrize("rpp", [5, 16, 37])
def test_typed_fc_trunk_matches_oracle(hip_lib, rpp, mode):
    """K19: skip / fc / residual module types (pathnet.py:122-196) vs trunk_forward_ref, fwd + grad, on the
    VALU kernels and on the fp32-MFMA kernels."""
    from pathnet_gym_amd.algo.supervised import supervised_config
    from pathnet_gym_amd.ops import typed_fc
    cfg = supervised_config(L=3, M=10, N=3, width=20, din=300)
    typed_fc.set_mfma(mode)
    try:
        _typed_vs_oracle(cfg, 7, rpp, (300,), rpp, 1e-5 if mode == "never" else 2e-5)
    finally:
        typed_fc.set_mfma("auto")


def test_typed_fc_wide_layers_use_mfma(hip_lib):
    """Widths > 64 (beyond the VALU kernels): 3072 -> 160 -> 160 -> 160 with module2 types, MFMA path."""
    from pathnet_gym_amd.algo.supervised import supervised_config
    cfg = supervised_config(L=4, M=10, N=3, width=160, din=3072)
    _typed_vs_oracle(cfg, 6, 24, (3072,), 2, 2e-5)


def test_typed_conv_modules_match_oracle(hip_lib):
    """conv_module (pathnet.py:170-183): VALID conv + bias + ReLU modules as typed GEMMs over im2col rows,
    then an fc layer; fwd + grad vs trunk_forward_ref."""
    from pathnet_gym_amd.config import LayerSpec, PathNetConfig
    from pathnet_gym_amd.ops import typed_fc
    cfg = PathNetConfig(L=3, M=6, N=2, input_shape=(32, 32, 3),
                        layers=[LayerSpec("conv", 8, kernel=5, stride=2), LayerSpec("conv", 16, kernel=3, stride=2),
                                LayerSpec("fc", 80)], trunk_scale="none", num_actions=10)
    for mode in ("auto", "always"):
        typed_fc.set_mfma(mode)
        try:
            _typed_vs_oracle(cfg, 5, 6, (32, 32, 3), 4, 2e-5)
        finally:
            typed_fc.set_mfma("auto")


def test_supervised_hip_backend_trains(hip_lib):
    from pathnet_gym_amd.algo.supervised import SupervisedPathNet, make_digits, supervised_config
    cfg = supervised_config(L=3, M=10, N=3, width=20)
    sp = SupervisedPathNet(cfg, population=16, num_tasks=1, device=DEV, seed=0)
    assert sp.backend == "hip"
    data = make_digits("mnist", 1024, 0, DEV)
    accs = []
    for gen in range(8):
        acc = sp.train_generation(data, 0, 10, 16, 0.05, gen)
        sp.pop.step(acc.astype(np.float32), gen)
        accs.append(float(acc.max()))
    assert accs[-1] > 0.5


@pytest.mark.parametrize("window,T", [pytest.param(0, 7, id="0"), pytest.param(3, 7, id="3"),
                                      pytest.param(3, 70, id="3-T70")])
def test_fitness_update_kernel_matches_reference(hip_lib, window, T):
    """Per-path fitness from the rollout's (done, episode return) pairs (a3c_training_thread.py:145-147).  T = 70 is
    more than the kernel's 64 threads: the t += blockDim.x loop and 2 T floats of dynamic LDS."""
    from pathnet_gym_amd.ops import _lib
    P, E = 5, 48
    rng = np.random.RandomState(4)
    dones = (rng.rand(T, P, E) < 0.05).astype(np.uint8)
    dones[:, 3, :] = 0                                   # a path with no finished episode keeps its fitness
    epret = rng.randint(-21, 22, size=(T, P, E)).astype(np.float32)
    fit0 = rng.randn(P).astype(np.float32)
    cnt0 = rng.randint(0, 3, size=P).astype(np.float32)
    sum0 = (cnt0 * 2.0).astype(np.float32)
    # numpy reference of the per-path scan
    fit_ref, cnt_ref, sum_ref = fit0.copy(), cnt0.copy(), sum0.copy()
    for p in range(P):
        nep = sret = 0.0
        for t in range(T):
            c = float(dones[t, p].sum())
            s = float((epret[t, p] * dones[t, p]).sum())
            if c > 0:
                fit_ref[p] = s / c
            nep += c
            sret += s
        if window > 0:
            cnt_ref[p] += nep
            sum_ref[p] += sret
            fit_ref[p] = sum_ref[p] / cnt_ref[p] if cnt_ref[p] >= window else -1000.0
    d = torch.from_numpy(dones).to(DEV)
    r = torch.from_numpy(epret).to(DEV)
    fit = torch.from_numpy(fit0).to(DEV)
    cnt = torch.from_numpy(cnt0).to(DEV)
    sm = torch.from_numpy(sum0).to(DEV)
    counters = torch.full((4,), 7.0, device=DEV)
    part = torch.full((P, 2), 5.0, device=DEV)
    _lib.call("launch_fitness_update", d.data_ptr(), r.data_ptr(), T, P, E, fit.data_ptr(), counters.data_ptr(),
              cnt.data_ptr(), sm.data_ptr(), window, part.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    np.testing.assert_allclose(fit.cpu().numpy(), fit_ref, rtol=1e-6)
    c = counters.cpu().numpy()
    assert c[0] == T * P * E and c[1] == dones.sum() and c[2] == (epret * dones).sum() and c[3] == 0
    # non-integer returns (Doom): the fixed-order sums make fitness bit-identical run to run
    rf = torch.from_numpy(epret * 0.37 + 0.011).to(DEV)
    outs = []
    for _ in range(3):
        f2 = torch.from_numpy(fit0).to(DEV)
        c2 = torch.zeros(4, device=DEV)
        _lib.call("launch_fitness_update", d.data_ptr(), rf.data_ptr(), T, P, E, f2.data_ptr(), c2.data_ptr(),
                  torch.from_numpy(cnt0).to(DEV).data_ptr(), torch.from_numpy(sum0).to(DEV).data_ptr(), 0,
                  part.data_ptr(), _lib.stream())
        torch.cuda.synchronize()
        outs.append((f2.cpu().numpy().copy(), c2.cpu().numpy().copy()))
    for f2, c2 in outs[1:]:
        assert np.array_equal(f2, outs[0][0]) and np.array_equal(c2, outs[0][1])
    if window > 0:
        np.testing.assert_allclose(cnt.cpu().numpy(), cnt_ref)
        np.testing.assert_allclose(sm.cpu().numpy(), sum_ref)
