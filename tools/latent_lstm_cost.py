"""What `MODEL.STATE_ENCODER.rnn_type: LSTM` costs in Latent-CMA, next to the GRU configuration of the same checkout, and
what the tour-memory step kernel (include/ivln_tour_state.h) saves over the same work issued from Python.

  python tools/latent_lstm_cost.py [--root DIR] [--cells GRU,LSTM] [--rounds R] [--no-seq]

  A  rollout step (hipGraph replay, B = 4, frames: both ResNets run) and DAgger update (T = 64, N = 5, cached features),
     per memory mode, for each cell type.  The configurations are measured in turn, R rounds; a line per configuration
     gives the median round and the spread (min .. max) of the rounds - a difference inside the spread is no difference.
  B  the variant's first-encoder sequence at T = 64, N = 8, H = 512, saves on (the update's form):
       one call   ops.linear_gemm (W_ih[:, :I0] x + b_ih for all rows) + ops.lstm_seq_tour (T launches from one C call)
       composed   T x (ops.tour_memory + ops.lstm_step on the full [x | memory] row) + the trailing ops.tour_memory,
                  2T + 1 launches, each a Python -> ctypes round trip
     same inputs; the outputs are compared (another summation order: W_ih x is split at I0 in the one-call form).

--root: import the package from ANOTHER checkout of this project (its own built library), e.g. the parent commit, to put
its GRU figures beside this one's in the same session; a checkout without the LSTM option is measured with --cells GRU
--no-seq.  Times are host clocks around work that ends in a device synchronise."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--cells", default="GRU,LSTM")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-seq", action="store_true")
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivln_ce_amd  # noqa: E402,F401
from ivln_ce_amd import latent_policy, ops  # noqa: E402,F401
from ivln_ce_amd.config import get_config  # noqa: E402
from ivln_ce_amd.graphed import GraphedRollout  # noqa: E402
from ivln_ce_amd.registry import baseline_registry  # noqa: E402
from ivln_ce_amd.spaces import Box, Dict, Discrete  # noqa: E402
from ivln_ce_amd.synthetic import SyntheticRollout  # noqa: E402
from ivln_ce_amd.trainers import FlatAdam, update_agent  # noqa: E402
from ivln_ce_amd.utils import trim_instruction_padding  # noqa: E402

dev = torch.device("cuda:0")
TAG = (args.tag + " ") if args.tag else ""
SPACE = Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32), "rgb": Box(0, 255, (224, 224, 3), np.uint8),
              "instruction": Box(0, 2504, (200,), np.int64)})
MODES = ("plain", "tour", "variant")


def policy(cell, mode):
    opts = ["MODEL.policy_name", "LatentCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
            "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE", "MODEL.tour_memory", mode == "tour",
            "MODEL.tour_memory_variant", mode == "variant", "MODEL.memory_at_end", mode == "variant"]
    if cell != "GRU":
        opts += ["MODEL.STATE_ENCODER.rnn_type", cell, "MODEL.STATE_ENCODER.latent_lstm", True]
    torch.manual_seed(0)
    return baseline_registry.get_policy("LatentCMAPolicy").from_config(get_config(opts=opts), SPACE, Discrete(4)).to(dev)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def report(name, rounds, unit=1e3, what="ms"):
    med = statistics.median(rounds)
    print(f"{TAG}{name:46s} median {unit * med:9.3f} {what}   spread {unit * min(rounds):9.3f} .. {unit * max(rounds):9.3f}  "
          f"({len(rounds)} rounds)", flush=True)
    return med


def part_a(cells):
    B, T, N = 4, 64, 5
    roll = SyntheticRollout(B=B, seed=5, with_rgb=True)
    obs = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in roll.step().items()} for _ in range(8)]
    g = torch.Generator().manual_seed(0)
    TN = T * N
    instr = torch.zeros(N, 200)
    instr[:, :80] = torch.randint(2, 2504, (N, 80), generator=g).float()
    o = {"rgb_features": torch.rand(TN, 2048, 4, 4, generator=g).to(dev),
         "depth_features": torch.randn(TN, 128, 4, 4, generator=g).to(dev),
         "instruction": trim_instruction_padding({"instruction": instr.repeat(T, 1)})["instruction"].to(dev)}
    prev = torch.randint(0, 4, (TN, 1), generator=g).to(dev)
    ep = torch.ones(T, N, dtype=torch.uint8)
    ep[0] = 0
    ep = ep.view(-1, 1).to(dev)
    tour = torch.ones(TN, 1, dtype=torch.uint8, device=dev)
    tgt = torch.randint(0, 4, (T, N), generator=g).to(dev)
    w = torch.ones(T, N, device=dev)
    runs = {}
    for cell in cells:
        for mode in MODES:
            p = policy(cell, mode)
            runner = GraphedRollout(p.eval(), [], obs[0], deterministic=True, streams=False)
            pt = policy(cell, mode).train()
            opt = FlatAdam(pt, lr=2.5e-4)
            rnn = torch.zeros(N, pt.net.num_recurrent_layers, 512, device=dev)
            runs[(cell, mode, "step")] = (lambda i, r=runner: r.step(obs[i % 8]), 100)
            runs[(cell, mode, "update")] = (lambda i, pt=pt, opt=opt, rnn=rnn: update_agent(
                pt, opt, o, prev, ep, tgt, w, tour_not_done_masks=tour, rnn_states=rnn), 8)
    for fn, n in runs.values():  # warm up every shape
        timed(fn, max(3, n // 10))
    res = {k: [] for k in runs}
    for _ in range(args.rounds):  # the configurations in turn, round after round
        for k, (fn, n) in runs.items():
            res[k].append(timed(fn, n))
    print(f"{TAG}A. Latent-CMA rollout step (graph replay, B = {B}, frames) and update (T = {T}, N = {N}, cached features)")
    for (cell, mode, kind), r in res.items():
        report(f"{kind:6s} {cell:4s} {mode}", r)


def part_b():
    T, N, H, I0 = 64, 8, 512, 416
    rows = T * N
    g = torch.Generator().manual_seed(1)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dev)  # noqa: E731
    w_ih, w_hh, b_ih, b_hh = r(4 * H, I0 + H, k=0.03), r(4 * H, H, k=0.04), r(4 * H, k=0.1), r(4 * H, k=0.1)
    xb, st = r(rows, I0), r(N, 5, H, k=0.3)
    ep = (torch.rand(rows, generator=g) < 0.9).to(torch.uint8).to(dev)
    tour = (torch.rand(rows, generator=g) < 0.97).to(torch.uint8).to(dev)

    def bufs():
        x = torch.empty(rows, I0 + H, device=dev)
        x[:, :I0] = xb
        return dict(x=x, out=torch.empty(rows, H, device=dev), so=torch.zeros(N, 5, H, device=dev),
                    sv=tuple(torch.empty(rows, H, device=dev) for _ in range(5)))

    a, b = bufs(), bufs()

    def one_call(_):
        gi = ops.linear_gemm(a["x"][:, :I0], w_ih, b_ih, w_prefix=True)
        ops.lstm_seq_tour(gi, w_ih, w_hh, b_hh, st[:, 0], st[:, 1], st[:, 4], ep, tour, a["out"], a["x"][:, I0:], a["so"][:, 0],
                          a["so"][:, 1], a["so"][:, 4], T, N, a["sv"])

    def composed(_):
        x, out, so, sv = b["x"], b["out"], b["so"], b["sv"]
        mem = x[:, I0:]
        for t in range(T):
            sl, sp = slice(t * N, (t + 1) * N), slice((t - 1) * N, t * N)
            ops.tour_memory(st[:, 4] if t == 0 else mem[sp], None if t == 0 else out[sp], tour[sl], mem[sl])
            ops.lstm_step(x[sl], None, st[:, 0] if t == 0 else out[sp], st[:, 1] if t == 0 else so[:, 1], ep[sl], w_ih, w_hh,
                          b_ih, b_hh, out[sl], so[:, 1], so[:, 0] if t == T - 1 else None, tuple(s[sl] for s in sv))
        ops.tour_memory(mem[(T - 1) * N:], out[(T - 1) * N:], None, so[:, 4])

    for fn in (one_call, composed):
        timed(fn, 5)
    diff = max(float((a[k] - b[k]).abs().max()) for k in ("x", "out", "so"))
    diff = max(diff, max(float((p - q).abs().max()) for p, q in zip(a["sv"], b["sv"])))
    res = {"one call": [], "composed": []}
    for _ in range(args.rounds):
        res["one call"].append(timed(one_call, 30))
        res["composed"].append(timed(composed, 30))
    print(f"{TAG}B. first-encoder sequence of the variant, T = {T}, N = {N}, H = {H}, I0 = {I0}, saves on "
          f"(max |one call - composed| over every output {diff:.3e})")
    m1 = report("one call: GEMM + ivln_lstm_seq_tour_fwd_f32", res["one call"], 1e6, "us")
    m2 = report(f"composed: {2 * T + 1} launches from Python", res["composed"], 1e6, "us")
    inside = min(res["composed"]) <= max(res["one call"])
    print(f"{TAG}   one call / composed = {m1 / m2:.3f}; per step {1e6 * m1 / T:.2f} us against {1e6 * m2 / T:.2f} us; "
          f"{'the spreads OVERLAP: no difference shown' if inside else 'outside the spread of either'}")


if __name__ == "__main__":
    print(f"{TAG}{torch.cuda.get_device_name(0)}; torch {torch.__version__}; package from {'this checkout' if not args.tag else args.tag}")
    part_a([c for c in args.cells.split(",") if c])
    if not args.no_seq:
        part_b()
