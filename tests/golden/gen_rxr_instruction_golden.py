"""Generate tests/golden/rxr_instruction.npz by running the REFERENCE's own `InstructionEncoder`
(ivlnce_baselines/models/encoders/instruction_encoder.py:11-94) with `sensor_uuid = "rxr_instruction"` - no embedding
layer, observations["rxr_instruction"] (B, L, E) pre-computed features, lengths = the NUMBER of non-zero rows - on seeded
inputs, with weights from tests/golden/det_init.py.  Build container only:
    python tests/golden/gen_rxr_instruction_golden.py
hidden_size 128, embedding_size 8, final_state_only False, B = 4, L = 6; row patterns: full; 2 rows; 1 row; a zero row at
t = 1 between non-zero rows 0, 2, 3 (count 3: the recurrence runs over rows 0, 1, 2 - the case that tells a count from the
index of the last non-zero row).  Cells: LSTM and GRU, one and two directions.  Inputs and outputs only, a few KB."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_shim  # noqa: E402

_ref_shim.install()
torch.set_num_threads(4)
from det_init import det_fill  # noqa: E402

from ivlnce_baselines.models.encoders.instruction_encoder import InstructionEncoder  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
B, L, E, H = 4, 6, 8, 128
NONZERO_ROWS = [[0, 1, 2, 3, 4, 5], [0, 1], [0], [0, 2, 3]]


def features():
    g = torch.Generator().manual_seed(512768)
    x = torch.zeros(B, L, E)
    for b, rows in enumerate(NONZERO_ROWS):
        x[b, rows] = torch.randn(len(rows), E, generator=g)
    return x


def main():
    x = features()
    d = {"rxr_instruction": x.numpy()}
    for cell in ("LSTM", "GRU"):
        for bidir in (True, False):
            cfg = _ref_shim.default_model_config().MODEL.INSTRUCTION_ENCODER
            cfg.sensor_uuid, cfg.rnn_type, cfg.bidirectional = "rxr_instruction", cell, bidir
            cfg.hidden_size, cfg.embedding_size, cfg.final_state_only = H, E, False
            enc = det_fill(InstructionEncoder(cfg), seed=0)
            assert not hasattr(enc, "embedding_layer")
            with torch.no_grad():
                out = enc({"rxr_instruction": x})
            d[f"out/{cell}/{int(bidir)}"] = out.numpy()
            print(cell, bidir, tuple(out.shape), float(out.abs().max()))
    np.savez_compressed(os.path.join(OUT, "rxr_instruction.npz"), **d)
    print("rxr_instruction.npz", os.path.getsize(os.path.join(OUT, "rxr_instruction.npz")), "bytes")


if __name__ == "__main__":
    main()
