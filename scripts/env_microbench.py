#!/usr/bin/env python3
"""Micro-benchmark of the on-device env step kernels: Pong (packed stack push vs frame ring) and the rectangle
games' frame-ring step (``game_step`` + ``rects16_ring_push``, timed together and each alone).

    python scripts/env_microbench.py [--envs 2048] [--iters 200] [--games Centipede,DoomBasic,...] [--meta]
Prints one JSON line per variant with the mean kernel time (us) measured with HIP events.

``--meta`` adds the meta game of the nine Doom levels (``meta_step`` + ``rects16_ring_push_lv``): every env on one
level (nine lines), the levels spread evenly env by env (every wave holds all nine) and in nine contiguous blocks (a
wave holds one or two), each with the single-table rasteriser on the same padded scenes next to the ``_lv`` one.  The
envs are held on their levels for the timing: only their own level is unlocked and the table's targets are moved out
of reach, so no episode scores and nothing unlocks.
"""
from __future__ import annotations

import argparse
import json

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--games", default="Centipede,DoomBasic,DoomDefendCenter,DoomTakeCover",
                    help="rectangle games to time on the frame ring (empty: Pong only)")
    ap.add_argument("--meta", action="store_true", help="also time the meta game of the nine Doom levels")
    args = ap.parse_args()
    from pathnet_gym_amd import _build
    _build.build()
    from pathnet_gym_amd.envs.pong import PongVec
    from pathnet_gym_amd.ops import envs as henv
    dev = "cuda:0"
    B = args.envs
    env = PongVec(B, device=dev, backend="hip", seed=3)
    env.reset()
    acts = torch.randint(0, 6, (B,), dtype=torch.int32, device=dev)
    r = torch.empty(B, device=dev)
    d = torch.empty(B, dtype=torch.uint8, device=dev)
    e = torch.empty(B, device=dev)
    stack_a = env.obs.reshape(B, -1).contiguous()
    stack_b = torch.empty_like(stack_a)
    frames = torch.zeros(B, 24, 160 * 120, dtype=torch.uint8, device=dev)
    fc = torch.zeros(2, B, dtype=torch.uint8, device=dev)

    def timeit(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.iters):
            fn()
        t.record()
        torch.cuda.synchronize()
        return s.elapsed_time(t) * 1e3 / args.iters

    base_fs = env.frameskip
    for fs in (base_fs, 0):
        env.frameskip = fs
        us_p = timeit(lambda: henv.pong_step_into(env, acts, stack_a, stack_b, r, d, e))
        us_r = timeit(lambda: henv.pong_step_ring_into(env, acts, frames, 5, fc[0], fc[1], r, d, e))
        print(json.dumps({"envs": B, "frameskip": fs, "packed_us": round(us_p, 2), "ring_us": round(us_r, 2)}))
    env.frameskip = base_fs

    from pathnet_gym_amd.envs.atari_games import GAMES
    gen = torch.Generator().manual_seed(1)
    for name in [x.strip() for x in args.games.split(",") if x.strip()]:
        g = GAMES[name](B, device=dev, seed=3, backend="hip")
        g.reset()
        for _ in range(50):           # a mid-episode state: objects on screen, episodes ending at different steps
            g.step(torch.randint(0, g.num_actions, (B,), generator=gen).to(dev))
        a = torch.randint(0, g.num_actions, (B,), generator=gen).to(device=dev, dtype=torch.int32)

        def logic():
            g._hip_run(a, None, r, d, e)

        def raster():
            henv.rects16_ring_push(g._rects, g._gray_tab, g._bg_gray, frames, 5, fc[0], fc[1], d, g._tab32)

        us_l, us_r = timeit(logic), timeit(raster)
        us = timeit(lambda: g.step_ring_into(a, frames, 5, fc[0], fc[1], r, d, e))
        print(json.dumps({"game": name, "envs": B, "rects": g._rects.shape[1], "state_ints": g._st32.shape[1],
                          "ring_step_us": round(us, 2), "game_step_us": round(us_l, 2),
                          "rects16_ring_push_us": round(us_r, 2)}))

    if not args.meta:
        return
    from pathnet_gym_amd.envs.doom.constants import LEVEL_NAMES
    from pathnet_gym_amd.envs.doom_meta_games import NL, DoomMetaVec
    ar = torch.arange(B, device=dev)
    settings = [("all on " + n, torch.full((B,), l, device=dev)) for l, n in enumerate(LEVEL_NAMES)]
    settings += [("spread env by env", ar % NL), ("nine blocks", ar * NL // B)]
    for label, levels in settings:
        m = DoomMetaVec(B, device=dev, seed=3, backend="hip")
        rows, j = m._st32.clone(), m.NSU
        rows[:, j] = levels.to(torch.int32)
        rows[:, j + 1] = (1 << levels).to(torch.int32)
        m.load_packed(rows)
        m._level_tab[:, 1] = m._level_tab[:, 0] + 10 ** 6
        m.reset()
        for _ in range(50):
            m.step(torch.randint(0, m.num_actions, (B,), generator=gen).to(dev))
        assert torch.equal(m._lv8.long(), levels), label
        a = torch.randint(0, m.num_actions, (B,), generator=gen).to(device=dev, dtype=torch.int32)
        one = m._gray_tab[int(levels[0])].contiguous()
        us_l = timeit(lambda: m._hip_run(a, None, r, d, e))
        us_lv = timeit(lambda: m._hip_ring_push(frames, 5, fc[0], fc[1], d))
        us_1 = timeit(lambda: henv.rects16_ring_push(m._rects, one, m._bg_gray, frames, 5, fc[0], fc[1], d, m._tab32))
        us = timeit(lambda: m.step_ring_into(a, frames, 5, fc[0], fc[1], r, d, e))
        print(json.dumps({"game": "DoomMeta", "levels": label, "envs": B, "rects": m._rects.shape[1],
                          "state_ints": m._st32.shape[1], "ring_step_us": round(us, 2), "meta_step_us": round(us_l, 2),
                          "rects16_ring_push_lv_us": round(us_lv, 2), "rects16_ring_push_us": round(us_1, 2)}))
        m.close()


if __name__ == "__main__":
    main()
