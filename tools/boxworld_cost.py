"""What an env step costs the host loop: milliseconds per `envs.step` + `utils.batch_obs` (the observations stacked on the
device, ending in a synchronise) at `--envs` envs under the scripted expert's actions, for
  synthetic  `SyntheticVectorEnv`: frames from the host's random generator, copied to the device by batch_obs
  boxworld   `BoxWorldVectorEnv`: frames ray-cast on the device (csrc/boxworld.hip), batch_obs stacks device views
each with `with_rgb` off and on.

    python tools/boxworld_cost.py [--envs 8] [--rounds 5] [--steps 50]

Host clock around `steps` steps, the settings alternating round by round in one process after two warm-up rounds (the
protocol of tools/known_map_cost.py); median / min / max over `rounds`.  The synthetic backend is the yardstick of the
box-world one in the same call.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTINGS = [(backend, rgb) for rgb in (False, True) for backend in ("synthetic", "boxworld")]


def _three(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


class Setting:
    def __init__(self, backend, with_rgb, n, dev):
        from ivln_ce_amd.config import get_config
        from ivln_ce_amd.envs import construct_envs

        cfg = get_config(opts=["NUM_ENVIRONMENTS", n, "ENV_BACKEND", backend])
        # (episodes enough for every round: an env restarts the next one by itself)
        self.envs = construct_envs(cfg, auto_reset_done=True, iterative=False, with_rgb=with_rgb, n_episodes=64)
        self.dev = dev
        self.obs = self.envs.reset()

    def steps(self, n):
        from ivln_ce_amd.utils import batch_obs

        for _ in range(n):
            actions = [int(o["shortest_path_sensor"][0]) for o in self.obs]
            self.obs = [out[0] for out in self.envs.step(actions)]
            batch_obs(self.obs, self.dev)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boxworld_cost: needs the GPU (a CPU run gives no time)")
    os.environ.pop("IVLN_ENV_BACKEND", None)  # (the override would make every setting the same backend)
    dev = torch.device("cuda:0")
    runs = {k: Setting(*k, a.envs, dev) for k in SETTINGS}
    times = {k: [] for k in SETTINGS}
    for rnd in range(2 + a.rounds):
        for k, st in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.steps(a.steps)
            if rnd >= 2:
                times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    res = {"envs": a.envs, "steps": a.steps, "rounds": a.rounds, "unit": "ms per envs.step + batch_obs [median, min, max]"}
    for backend, rgb in SETTINGS:
        res[f"{backend}_{'rgb' if rgb else 'norgb'}_ms"] = _three(times[(backend, rgb)])
    for st in runs.values():
        st.envs.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
