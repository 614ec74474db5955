"""The CPU side of the fine-tuning overfit test: tests/rednet_twin.py's fp32 twin with torch.optim.Adam on the test's one
fixed structured batch (64 x 64, B = 4, 20 steps, the test's learning rate) -> tests/golden/rednet_overfit_cpu.json.
Recorded once (about ten seconds of CPU) so that the GPU test only reads it; it shows that the batch can be learned from by
plain torch, and the GPU test asserts no closeness to it.   python tests/golden/gen_rednet_overfit_curve.py"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import rednet_twin as RW  # noqa: E402
from det_init import det_fill  # noqa: E402

LR, STEPS = 1e-3, 20

if __name__ == "__main__":
    torch.set_num_threads(8)
    state = {k: v.clone() for k, v in det_fill(RW.RedNetTwin(), seed=1, conv_gain=0.6).state_dict().items()}
    losses, before, after = RW.twin_overfit(state, RW.structured_batch(), LR, STEPS)
    assert losses[-1] < losses[0] and after > before, (losses, before, after)
    out = dict(lr=LR, steps=STEPS, losses=losses, miou_before=before, miou_after=after)
    json.dump(out, open(os.path.join(HERE, "rednet_overfit_cpu.json"), "w"), indent=1)
    print(out)
