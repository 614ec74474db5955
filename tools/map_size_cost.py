"""What an egocentric map other than 64 x 64 cells costs.

  attention  the head's two short attentions of a rollout step at 8 rows (Ck = 256; depth: 16 positions, 128 value channels;
             map: --map-positions positions, 256 value channels): `pair` = ops.attn_pair, one launch, against `generic` = the
             two ops.attn calls it replaces (four launches and two logits workspaces), launched eagerly (host clock around
             --calls calls that end in a synchronise) and replayed from a graph of --calls calls (device time per call)
  step       the replayed gt-semantics rollout step (GTSemanticsIterativeMapper + MapCMAPolicy.act, graphed.GraphedRollout in
             split mode) at --envs envs for --maps: 64x64 takes the fused recurrent head, every other size the unfused chain

    python tools/map_size_cost.py [--map-positions 6,42,256] [--maps 64x64,32x48,128x128] [--envs 4] [--rounds 5]

One process, the settings alternating round by round after two warm-up rounds; [median, min, max] over `rounds`.  A
difference counts only outside the spread of the rounds.  Prints one JSON line per measurement."""
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


def _three(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


def attention(i_map, rounds, calls, dev):
    from ivln_ce_amd import ops

    rows, h2, d_out, m_out, i_dep, scale = 8, 256, 128, 256, 16, 0.0625
    g = torch.Generator().manual_seed(i_map)
    q = torch.randn(rows, h2, generator=g).to(dev)
    dkv = torch.randn(rows, h2 + d_out, i_dep, generator=g).to(dev)
    mkv = torch.randn(rows, h2 + m_out, i_map, generator=g).to(dev)
    x2 = torch.zeros(rows, 1184, device=dev)
    o_dep, o_map = x2[:, 768:768 + d_out], x2[:, 896:896 + m_out]

    def pair():
        ops.attn_pair(q, dkv[:, :h2], dkv[:, h2:], o_dep, mkv[:, :h2], mkv[:, h2:], o_map, scale)

    def generic():
        ops.attn(q, dkv[:, :h2], dkv[:, h2:], None, scale, o_dep)
        ops.attn(q, mkv[:, :h2], mkv[:, h2:], None, scale, o_map)

    forms = {"pair": pair, "generic": generic}
    graphs = {}
    side = torch.cuda.Stream(dev)
    for k, fn in forms.items():
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            fn()
            side.synchronize()
            with torch.cuda.graph(gr, stream=side):
                for _ in range(calls):
                    fn()
        graphs[k] = gr
    eager, replay = {k: [] for k in forms}, {k: [] for k in forms}
    for rnd in range(2 + rounds):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            graphs[k].replay()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rnd >= 2:
                eager[k].append((t1 - t0) * 1e6 / calls)
                replay[k].append((t2 - t1) * 1e6 / calls)
    res = {"measure": "attention", "rows": rows, "I_dep": i_dep, "I_map": i_map, "calls": calls, "rounds": rounds}
    for k in forms:
        res[f"{k}_eager_us"], res[f"{k}_replay_us"] = _three(eager[k]), _three(replay[k])
    return res


class Step:
    def __init__(self, rows, cols, B, dev):
        from ivln_ce_amd.config import get_config
        from ivln_ce_amd.graphed import GraphedRollout
        from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper
        from ivln_ce_amd.policy import MapCMAPolicy
        from ivln_ce_amd.spaces import Box, Dict, Discrete
        from ivln_ce_amd.synthetic import SyntheticRollout

        cfg = get_config(opts=["MODEL.policy_name", "MapCMAPolicy", "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False,
                               "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE",
                               "RL.POLICY.OBS_TRANSFORMS.EGOCENTRIC_MAPPER.height_meters", rows / 10.0,
                               "RL.POLICY.OBS_TRANSFORMS.EGOCENTRIC_MAPPER.width_meters", cols / 10.0])
        self.tr = GTSemanticsIterativeMapper.from_config(cfg)
        self.tr.sizing["b_max"] = B
        space = self.tr.transform_observation_space(Dict({"depth": Box(0.0, 1.0, (256, 256, 1), np.float32),
                                                          "instruction": Box(0, 2504, (200,), np.int64)}))
        assert space.spaces["occupancy_map"].shape == (rows, cols), space.spaces["occupancy_map"].shape
        torch.manual_seed(0)
        self.policy = MapCMAPolicy.from_config(cfg, space, Discrete(4)).to(dev).eval()
        roll = SyntheticRollout(B=B, seed=1)
        self.obs = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in roll.step().items()} for _ in range(4)]
        self.fused = self.policy.net._fused_head_eligible({"instruction": self.obs[0]["instruction"]}, None)
        self.runner = GraphedRollout(self.policy, [self.tr], self.obs[0], deterministic=True, streams="split")
        self.tr.mapping_module.reset()
        self.runner.reset_state()

    def run(self, steps):
        for i in range(steps):
            self.runner.step(self.obs[i & 3])


def steps_cost(maps, B, rounds, steps, dev):
    runs = {f"{r}x{c}": Step(r, c, B, dev) for r, c in maps}
    times = {k: [] for k in runs}
    for rnd in range(2 + rounds):
        for k, st in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.run(steps)
            torch.cuda.synchronize()
            if rnd >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {"measure": "step", "envs": B, "steps": steps, "rounds": rounds}
    for k, st in runs.items():
        res[f"{k}_ms"] = _three(times[k])
        res[f"{k}_head"] = "fused" if st.fused else "unfused"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-positions", default="6,42,256")
    ap.add_argument("--maps", default="64x64,32x48,128x128")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_size_cost: needs the GPU (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    for i_map in (int(p) for p in a.map_positions.split(",") if p):
        print(json.dumps(attention(i_map, a.rounds, a.calls, dev)), flush=True)
    maps = [tuple(int(v) for v in m.split("x")) for m in a.maps.split(",") if m]
    if maps:
        print(json.dumps(steps_cost(maps, a.envs, a.rounds, a.steps, dev)), flush=True)


if __name__ == "__main__":
    main()
