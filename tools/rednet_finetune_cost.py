"""What a RedNet fine-tune step costs: ms per RedNetTrainer.step at B x size x size for trainable "all" and "decoder", and
the frozen forward (PredictSemantics, the rollout's path) in the same process.

    python tools/rednet_finetune_cost.py [--B 8] [--size 256] [--rounds 5] [--out profiles/rednet_finetune_cost.txt]

The three alternate (2 warm-up rounds, then the median (min - max) of `rounds`), host clock around the call + synchronize.
Prints the report and writes it to --out."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rednet_finetune_cost.txt"))
    a = ap.parse_args()
    from ivln_ce_amd.rednet import PredictSemantics, RedNet
    from ivln_ce_amd.rednet_train import RedNetTrainer

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
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
