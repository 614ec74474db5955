"""A/B of the LSTM rollout step: the fused recurrent head (ivln_cma_step_lstm_fwd, ops.CMA_STEP_MODE 0) against the
unfused op chain (CMA_STEP_MODE -1), both in ONE process on one GPU (machines differ by ~6 %, so the two sides of a
comparison must share one).

  python tools/cma_step_lstm_ab.py [--envs 4 8] [--reps 5] [--replays 200] [--out FILE]

Per batch size and setting: a fresh STATE_ENCODER.rnn_type LSTM policy (same seed), a fresh capture of the gt-semantics
step as bench.py captures it (three graphs on two streams), 50 warm-up replays, then `reps` repetitions of `replays`
replayed steps between two device synchronisations; the settings alternate inside every repetition.  Reports median,
min and max of the per-step time per setting, and the difference of the medians against the larger min-max spread.
The first replayed step of the two settings is compared as well (largest difference of the recurrent state)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivln_ce_amd  # noqa: E402,F401
from ivln_ce_amd import ops  # noqa: E402


def make_policy(dev, seed=0):
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.policy import MapCMAPolicy
    from ivln_ce_amd.spaces import Box, Dict, Discrete

    cfg = get_config(opts=[
        "MODEL.policy_name", "MapCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
        "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.PROGRESS_MONITOR.use", True,
        "MODEL.STATE_ENCODER.rnn_type", "LSTM",
    ])
    space = Dict({
        "depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "occupancy_map": Box(0, 255, (64, 64), np.uint8),
        "semantic_map": Box(0, 255, (64, 64), np.uint8), "instruction": Box(0, 2504, (200,), np.int64),
    })
    torch.manual_seed(seed)
    pol = MapCMAPolicy.from_config(cfg, space, Discrete(4)).to(dev).eval()
    assert pol.net.fused_head_form == "lstm"
    return cfg, pol


def build(mode, B, obs, dev):
    """fresh policy + capture with CMA_STEP_MODE = mode; -> (runner, transform, calls of the fused entry while building)"""
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper

    ops.CMA_STEP_MODE = mode
    cfg, pol = make_policy(dev)
    tr = GTSemanticsIterativeMapper.from_config(cfg)
    calls = []
    real = ops.cma_step_lstm
    ops.cma_step_lstm = lambda d, mode=None: (calls.append(1), real(d, mode))[1]
    try:
        runner = GraphedRollout(pol, [tr], obs[0], deterministic=True, streams="split")
    finally:
        ops.cma_step_lstm = real
    tr.mapping_module.reset()
    runner.reset_state()
    return runner, tr, len(calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ivln_ce_amd.synthetic import SyntheticRollout

    dev = torch.device("cuda:0")
    lines = [f"LSTM rollout step, gt semantics, hipGraph replay (3 graphs on 2 streams): fused head (CMA_STEP_MODE 0) vs unfused "
             f"chain (-1); {args.reps} repetitions of {args.replays} replays per setting, alternating, one process",
             f"device: {torch.cuda.get_device_name(0)}"]
    saved = ops.CMA_STEP_MODE
    try:
        for B in args.envs:
            roll = SyntheticRollout(B=B, seed=1234)
            n_pool = 64
            obs = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in roll.step().items()} for _ in range(n_pool)]
            side = {}
            for mode in (0, -1):
                runner, tr, n_calls = build(mode, B, obs, dev)
                assert (n_calls > 0) == (mode == 0), (mode, n_calls)
                side[mode] = dict(runner=runner, tr=tr, ms=[], i=0)
            # the first step (same observations, zero state) in both settings: what the two forms differ by
            for m in (0, -1):
                side[m]["runner"].step(obs[0])
            torch.cuda.synchronize()
            dstate = float((side[0]["runner"].rnn_states - side[-1]["runner"].rnn_states).abs().max())
            lines.append(f"envs {B}  first replayed step: max |state(fused) - state(unfused)| = {dstate:.2e}")
            for m in (0, -1):
                for _ in range(args.warmup):
                    side[m]["runner"].step(obs[side[m]["i"] % n_pool])
                    side[m]["i"] += 1
            torch.cuda.synchronize()
            for rep in range(args.reps):
                for m in ((0, -1) if rep % 2 == 0 else (-1, 0)):
                    sd = side[m]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.replays):
                        sd["runner"].step(obs[sd["i"] % n_pool])
                        sd["i"] += 1
                    torch.cuda.synchronize()
                    sd["ms"].append(1e3 * (time.perf_counter() - t0) / args.replays)
            med = {}
            for m in (0, -1):
                ms = side[m]["ms"]
                side[m]["tr"].mapping_module.check_status()
                med[m] = statistics.median(ms)
                lines.append(f"envs {B}  {'fused  ' if m == 0 else 'unfused'}  median {med[m]:.4f} ms  min {min(ms):.4f}  max {max(ms):.4f}"
                             f"  per step   [{', '.join(f'{x:.4f}' for x in ms)}]")
            spread = max(max(side[m]["ms"]) - min(side[m]["ms"]) for m in (0, -1))
            diff = med[0] - med[-1]
            verdict = ("fused slower than unfused by more than the spread" if diff > spread else
                       "fused faster than unfused by more than the spread" if -diff > spread else "within the spread")
            lines.append(f"envs {B}  fused - unfused = {1e3 * diff:+.1f} us per step; min-max spread {1e3 * spread:.1f} us: {verdict}")
            del side
            torch.cuda.synchronize()
    finally:
        ops.CMA_STEP_MODE = saved
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
