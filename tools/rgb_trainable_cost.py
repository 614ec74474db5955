"""What MODEL.RGB_ENCODER.trainable costs: the update of LatentCMAPolicy at T x N rows with the encoder trainable (rgb
frames in the batch: forward_train + train.rgb_encoder_backward) against the frozen default (cached rgb_features), and
the bytes _ResNet50Body.forward_train keeps per image.

    python tools/rgb_trainable_cost.py [--T 64] [--N 8] [--size 224] [--rounds 5]

Both policies live in one process and alternate (2 warm-up rounds, then the median of `rounds`), host clock around
update_agent + synchronize; depth features come cached in both cases.  Prints one JSON line."""
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


def _policy(trainable, dev):
    from ivln_ce_amd import latent_policy  # noqa: F401
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry
    from ivln_ce_amd.spaces import Box, Dict, Discrete

    cfg = get_config(opts=["MODEL.policy_name", "LatentCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
                           "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.RGB_ENCODER.trainable", trainable])
    space = Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "rgb": Box(0, 255, (224, 224, 3), np.uint8),
                  "instruction": Box(0, 2504, (200,), np.int64)})
    torch.manual_seed(0)
    return baseline_registry.get_policy("LatentCMAPolicy").from_config(cfg, space, Discrete(4)).to(dev).train()


def _saved_bytes(save):
    """bytes of the distinct storages the saves hold"""
    seen = {}

    def walk(o):
        if torch.is_tensor(o):
            seen[o.untyped_storage().data_ptr()] = o.untyped_storage().nbytes()
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)

    walk(save)
    return sum(seen.values()), len(seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from ivln_ce_amd.trainers import FlatAdam, update_agent

    dev = torch.device("cuda:0")
    T, N, TN = a.T, a.N, a.T * a.N
    g = torch.Generator().manual_seed(1)
    pols = {"frozen": _policy(False, dev), "trainable": _policy(True, dev)}
    opts = {k: FlatAdam(p, lr=2.5e-4) for k, p in pols.items()}
    instr = torch.zeros(N, 200)
    for n in range(N):
        instr[n, :20 + 7 * n] = torch.randint(2, 2504, (20 + 7 * n,), generator=g).float()
    common = {"depth_features": torch.randn(TN, 128, 4, 4, generator=g).to(dev), "instruction": instr.repeat(T, 1).to(dev)}
    obs = {"frozen": dict(common, rgb_features=torch.rand(TN, 2048, 4, 4, generator=g).to(dev)),
           "trainable": dict(common, rgb=torch.randint(0, 256, (TN, a.size, a.size, 3), generator=g, dtype=torch.uint8).to(dev))}
    prev = torch.randint(0, 4, (TN, 1), generator=g).to(dev)
    nd = torch.ones(T, N, dtype=torch.uint8)
    nd[0] = 0
    nd = nd.view(-1, 1).to(dev)
    tgt, w = torch.randint(0, 4, (T, N), generator=g).to(dev), torch.ones(T, N).to(dev)

    res = {"T": T, "N": N, "size": a.size}
    cnn = pols["trainable"].net.rgb_encoder.cnn
    state = {k: v.clone() for k, v in cnn.state_dict().items()}
    for B in (1, 8):  # (the saves per image do not depend on the batch)
        save = {}
        with torch.no_grad():
            cnn.forward_train(obs["trainable"]["rgb"][:B], save)
        nbytes, tensors = _saved_bytes(save)
        res[f"saved_MiB_per_image_B{B}"] = round(nbytes / B / 2 ** 20, 2)
        res["saved_tensors"] = tensors
        del save
    cnn.load_state_dict(state)  # (the running statistics as they were)

    times, peak = {k: [] for k in pols}, {}
    for rnd in range(2 + a.rounds):
        for k, pol in pols.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            update_agent(pol, opts[k], obs[k], prev, nd, tgt, w, hidden_size=512)
            torch.cuda.synchronize()
            if rnd >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3)
            peak[k] = torch.cuda.max_memory_allocated() / 2 ** 30
    for k in pols:
        res[f"{k}_ms"] = [round(statistics.median(times[k]), 2), round(min(times[k]), 2), round(max(times[k]), 2)]
        res[f"{k}_peak_GiB"] = round(peak[k], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
