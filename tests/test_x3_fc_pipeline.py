"""The fc1 forward GEMM (fc_fwd_mm2_x3, runtime k-step count) built for two workgroups per CU (4 waves per SIMD,
128 VGPRs) against its one-workgroup-per-CU build (fast_conv_set_x3_fc_fwd_wpe(2)): the same source, so every output
is equal bit for bit."""
import numpy as np
import pytest
import torch

from pathnet_gym_amd.algo.ga import get_geopath
from pathnet_gym_amd.config import LayerSpec, PathNetConfig, preset
from pathnet_gym_amd.models.acnet import ACPathNet
from pathnet_gym_amd.ops.pathnet_ops import _plane

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cfg():
    return PathNetConfig(L=5, M=10, N=4, input_shape=(160, 120, 4),
                         layers=[LayerSpec("conv", 8, 8, 4), LayerSpec("conv", 8, 4, 2), LayerSpec("conv", 8, 3, 1),
                                 LayerSpec("fc", 256), LayerSpec("fc", 256)],
                         trunk_scale="M", num_actions=6)


def _masks(cfg):
    """Three paths; in both fc layers 1, 4 and 5 active modules, modules 4 and 6-8 without a user, module 9 with one
    path (16 or 32 rows of a 128-row block) and modules 0-3 with two."""
    rng = np.random.RandomState(3)
    m = np.stack([get_geopath(cfg.L, cfg.M, cfg.N, rng) for _ in range(3)])
    for l in (3, 4):
        m[:, l, :] = 0
        m[0, l, 9] = 1
        m[1, l, 0:4] = 1
        m[2, l, 0:4] = 1
        m[2, l, 5] = 1
    return m


@pytest.fixture(scope="module")
def conv_stack(hip_lib):
    """The model and the conv3 output of one batch per (E, T), computed once and left unchanged."""
    cfg = _cfg()
    m = ACPathNet(cfg, 3, DEV, "hip", seed=7, compute_dtype="fp32x")
    m.set_paths(_masks(cfg))
    cache = {}

    def get(E, T):
        if (E, T) not in cache:
            hp = m.hip
            g = torch.Generator(device="cpu").manual_seed(2)
            x = torch.randint(0, 256, (T * 3 * E, 160, 120, 4), generator=g, dtype=torch.uint8).to(DEV)
            for l in range(3):
                Y = hp.alloc_act(l, (T, 3 * E, hp.geoms[l].out_feat))
                b, rows = hp.alloc_bits(l, T, 3 * E)
                hp.layer_fwd(l, x, Y, b, 3, E, T, 0, rows)
                x = Y
            torch.cuda.synchronize()
            cache[(E, T)] = x
        return cache[(E, T)]
    return m, get


@pytest.mark.parametrize("parts", [0, 2, 3, 8])
@pytest.mark.parametrize("E,T", [(16, 1), (16, 2), (32, 1)])
def test_x3_fc_forward_two_per_cu_build_bit_equal(hip_lib, conv_stack, E, T, parts):
    """fc1 (K = 1408, 44 k-steps: the build under test) and fc2 (K = 256, module-major here too: the constant-count
    build, 8 k-steps, with 4 or 8 parts fewer k-steps per part than register sets) under both builds: the output
    planes and the ReLU bit words of both layers are equal.  parts: the k split (0 = by rows: 4 here; 3 ships above
    768 rows)."""
    m, get = conv_stack
    hp, lib = m.hip, hip_lib
    x3 = get(E, T)
    outs = []
    hp.fc_fwd_mm_min_k = 0
    lib.fast_conv_set_x3_fc_ks_parts(parts)
    try:
        for wpe in (2, 4):
            lib.fast_conv_set_x3_fc_fwd_wpe(wpe)
            x, keep = x3, []
            for l in (3, 4):
                Y = hp.alloc_act(l, (T, 3 * E, hp.geoms[l].out_feat))
                b, rows = hp.alloc_bits(l, T, 3 * E)
                hp.layer_fwd(l, x, Y, b, 3, E, T, 0, rows)
                # fc1's output is an fp16 pair (both planes kept), fc2's is fp32
                keep += [torch.stack([Y, _plane(Y, 1, torch.float16)]) if Y.dtype == torch.float16 else Y.clone(),
                         b.clone()]
                x = Y
            torch.cuda.synchronize()
            outs.append(keep)
    finally:
        hp.fc_fwd_mm_min_k = 1024
        lib.fast_conv_set_x3_fc_ks_parts(0)
        lib.fast_conv_set_x3_fc_fwd_wpe(0)
    assert float(outs[0][0].float().abs().sum()) > 0 and float(outs[0][2].float().abs().sum()) > 0
    for name, a, b in zip(("fc1 Y", "fc1 bits", "fc2 Y", "fc2 bits"), outs[0], outs[1]):
        assert torch.equal(a, b), name


def test_x3_fc_forward_builds_same_training_run(hip_lib):
    """5 updates of a 4-path deterministic trainer on the shipped path (frame ring, hipGraphs, device GA) under each
    build: equal weights, fitness and genotypes."""
    from pathnet_gym_amd.algo.trainer import PathNetTrainer

    def run(wpe):
        hip_lib.fast_conv_set_x3_fc_fwd_wpe(wpe)
        cfg = preset("pong")
        cfg.paths, cfg.envs_per_path, cfg.a2c.t_max = 4, 16, 5
        cfg.compute_dtype = "fp32x"
        cfg.frame_ring = True
        cfg.use_graph = True
        cfg.ga.backend = "device"
        cfg.deterministic = True
        tr = PathNetTrainer(cfg, device=DEV)
        tr.env.max_episode_steps = 7
        for _ in range(5):
            tr.update()
        tr.flush()
        torch.cuda.synchronize()
        return (tr.model.store.flat.detach().clone(), tr.engine.fitness.clone(), tr.engine.ga_dev["geno"].clone())
    try:
        a, b = run(2), run(4)
    finally:
        hip_lib.fast_conv_set_x3_fc_fwd_wpe(0)
    for name, x, y in zip(("params", "fitness", "genotypes"), a, b):
        assert torch.equal(x, y), name
