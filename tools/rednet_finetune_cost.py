"""What a RedNet fine-tune step costs: ms per RedNetTrainer.step at B x size x size for trainable "all" and "decoder", and
the frozen forward (PredictSemantics, the rollout's path) in the same process.

    python tools/rednet_finetune_cost.py [--B 8] [--size 256] [--rounds 5] [--augment] [--out <file>]

The legs alternate (2 warm-up rounds, then the median (min - max) of `rounds`), host clock around the call + synchronize.
--augment adds the two step legs with on-device augmentation (a fresh record per image and step: host sampling, one
ops.seg_augment launch in place of the two normalisation launches) to the same call, and times the augmentation launch
alone: device events around 20 back-to-back launches.  Prints the report and writes it to --out
(profiles/rednet_finetune_cost.txt; with --augment profiles/rednet_augment_cost.txt)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--augment", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "rednet_augment_cost.txt" if a.augment else "rednet_finetune_cost.txt")
    from ivln_ce_amd import ops
    from ivln_ce_amd.rednet import PredictSemantics, RedNet
    from ivln_ce_amd.rednet_train import AugmentConfig, RedNetTrainer, sample_augment

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    B, S = a.B, a.size
    obs = {"rgb": torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(dev),
           "depth": torch.rand(B, S, S, 1, generator=g).to(dev),
           "semantic12": torch.randint(0, 13, (B, S, S, 1), generator=g).to(torch.uint8).to(dev)}
    torch.manual_seed(0)
    trainers = {k: RedNetTrainer(RedNet(PredictSemantics.CFG).to(dev).train(), trainable=k) for k in ("all", "decoder")}
    frozen = PredictSemantics(dev, model=RedNet(PredictSemantics.CFG).to(dev).eval())
    runs = {"step, trainable=all": lambda: trainers["all"].step(obs), "step, trainable=decoder": lambda: trainers["decoder"].step(obs),
            "frozen forward": lambda: frozen(obs)}
    if a.augment:
        aug = {k: RedNetTrainer(RedNet(PredictSemantics.CFG).to(dev).train(), trainable=k, augment=AugmentConfig(), seed=1)
               for k in ("all", "decoder")}
        runs["step + augment, all"] = lambda: aug["all"].step(obs)
        runs["step + augment, decoder"] = lambda: aug["decoder"].step(obs)
    times, peak = {k: [] for k in runs}, {}
    for rnd in range(2 + a.rounds):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            with torch.no_grad():
                fn()
            torch.cuda.synchronize()
            if rnd >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3)
            peak[k] = torch.cuda.max_memory_allocated() / 2 ** 30
    lines = [f"RedNet fine-tune cost, B = {B}, {S} x {S}, {torch.cuda.get_device_name(0)}: ms, median (min - max) of "
             f"{a.rounds} alternating rounds after 2 warm-up rounds; host clock around the call + synchronize"]
    for k in runs:
        t = times[k]
        lines.append(f"  {k:26s} {statistics.median(t):9.2f} ({min(t):.2f} - {max(t):.2f})   peak {peak[k]:.2f} GiB allocated")
    if a.augment:
        gen = torch.Generator().manual_seed(2)
        labels = obs["semantic12"][..., 0].contiguous()
        ev, per_launch = [torch.cuda.Event(enable_timing=True) for _ in range(2)], []
        for rnd in range(2 + a.rounds):
            geom, photo = sample_augment(AugmentConfig(), B, S, S, gen)
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(20):
                ops.seg_augment(obs["rgb"], obs["depth"], labels, geom, photo)
            ev[1].record()
            torch.cuda.synchronize()
            if rnd >= 2:
                per_launch.append(ev[0].elapsed_time(ev[1]) / 20 * 1e3)
        moved = B * S * S * (3 + 4 + 1 + 16 + 1)  # (u8 rgb, f32 depth and u8 labels read once; four f32 planes and u8 labels written)
        lines.append(f"  seg_augment alone, us per launch: {statistics.median(per_launch):.1f} ({min(per_launch):.1f} - "
                     f"{max(per_launch):.1f}), device events around 20 back-to-back launches incl. their allocations; "
                     f"{moved / 1e6:.1f} MB of compulsory traffic per launch")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
