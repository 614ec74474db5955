"""What MODEL.INSTRUCTION_ENCODER.sensor_uuid = "rxr_instruction" costs in the rollout step: the front kernel of the
feature path (ivln_text_feat_front_f32) at (B, 512, 768) in the steady state (all rows clean) and with every row dirty,
beside a device-to-device copy of the same bytes in the same run, and the gt-semantics rollout step (hipGraph replay,
3 forked streams) with token instructions, with features and the per-episode cache, and with features re-encoded at
every step (IVLN_CACHE_INSTRUCTION=0).

    python tools/text_feat_cost.py [--envs 8] [--rounds 7] [--steps 200] [--settings tokens,features_cached,features_uncached]

Launch times: device events around each single launch - the kernel plus the gaps to the event records beside it, NOT a
kernel time from a trace -, the variants alternating, median / min / max over `rounds` batches of 100 launches after a
warm-up batch.  Step times: host clock around `steps` replays that end in a synchronise, the settings alternating round by
round after two warm-up rounds.  `--settings tokens` times the token step alone and uses nothing of the feature path: the
same file runs on a checkout from before the feature, which is how the token step is compared with its parent.  Prints one
JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L, E = 512, 768


def _three(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


def front_kernel(B, rounds, dev):
    from ivln_ce_amd import ops

    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, L, E, generator=g)
    x[:, 80:] = 0
    x = x.to(dev)
    dst = torch.empty_like(x)
    cache = ops.InstructionStepCache(B, L, 4, 128, dev, key=None, ndir=1, feat=E)

    def cached():
        ops.text_feat_front(x, cache=cache)

    # (`before` runs ahead of the first event: an invalidated cache makes every row dirty)
    variants = {"front_clean_us": (None, cached), "front_dirty_us": (cache.invalidate, cached),
                "front_lengths_only_us": (None, lambda: ops.text_feat_front(x)), "d2d_copy_us": (None, lambda: dst.copy_(x))}
    times = {k: [] for k in variants}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
    for rnd in range(1 + rounds):
        for name, (before, fn) in variants.items():
            ops.text_feat_front(x, cache=cache)  # (the cache holds x: `clean` finds nothing to do)
            for a, b in ev:
                if before is not None:
                    before()
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(1e3 * statistics.median(a.elapsed_time(b) for a, b in ev))
    res = {k: _three(v) for k, v in times.items()}
    res["bytes"] = x.numel() * 4
    return res


def _runner(kind, B, dev):
    """(runner, observations) of one setting: its own policy, mapper and captured graphs"""
    from ivln_ce_amd import ops
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper
    from ivln_ce_amd.policy import MapCMAPolicy
    from ivln_ce_amd.spaces import Box, Dict, Discrete
    from ivln_ce_amd.synthetic import SyntheticRollout

    feats = kind != "tokens"
    opts = ["MODEL.policy_name", "MapCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
            "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.PROGRESS_MONITOR.use", True]
    sp = {"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "occupancy_map": Box(0, 255, (64, 64), np.uint8),
          "semantic_map": Box(0, 255, (64, 64), np.uint8)}
    if feats:
        opts += ["MODEL.INSTRUCTION_ENCODER.sensor_uuid", "rxr_instruction", "MODEL.INSTRUCTION_ENCODER.embedding_size", E]
        sp["rxr_instruction"] = Box(-np.inf, np.inf, (L, E), np.float32)
    else:
        sp["instruction"] = Box(0, 2504, (200,), np.int64)
    cfg = get_config(opts=opts)
    torch.manual_seed(0)
    pol = MapCMAPolicy.from_config(cfg, Dict(sp), Discrete(4)).to(dev).eval()
    roll = SyntheticRollout(B=B, seed=1, **(dict(text_features=(L, E)) if feats else {}))
    obs = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in roll.step().items()} for _ in range(4)]
    ops.CACHE_INSTRUCTION = kind != "features_uncached"  # (read when the step is captured)
    try:
        runner = GraphedRollout(pol, [GTSemanticsIterativeMapper.from_config(cfg)], obs[0], deterministic=True, streams=True)
    finally:
        ops.CACHE_INSTRUCTION = True
    return runner, obs


def rollout_step(kinds, B, rounds, steps, dev):
    runs = {k: _runner(k, B, dev) for k in kinds}
    times = {k: [] for k in kinds}
    for rnd in range(2 + rounds):
        for k, (runner, obs) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                runner.step(obs[i & 3])
            torch.cuda.synchronize()
            if rnd >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    return {f"step_{k}_ms": _three(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--settings", default="tokens,features_cached,features_uncached")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_feat_cost: needs the GPU (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    res = {"envs": a.envs, "L": L, "E": E}
    kinds = tuple(a.settings.split(","))
    if any(k != "tokens" for k in kinds):
        res.update(front_kernel(a.envs, a.rounds, dev))
    res.update(rollout_step(kinds, a.envs, a.rounds, a.steps, dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
