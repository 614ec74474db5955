"""Synthetic vector environment speaking both step protocols of the reference's `ExtendedVectorEnv`
(ivlnce_baselines/common/env_utils.py:117-254; SURVEY.md Appendix D: num_envs, reset(), step(list[int]), reset_at,
pause_at, current_episodes(), number_of_episodes, observation_spaces, action_spaces, close()):

  episodic   (`VLNCEDaggerEnv`)     reset() -> [obs]; step(a) -> [(obs, reward, done, info)]; reset_at(i) -> [obs]
  iterative  (`VLNCEIterativeEnv`)  reset() -> [(obs, tour_done, produce_action)];
                                    step(a) -> [(obs, reward, agent_episode_done, sim_episode_done, tour_done,
                                                 produce_action, info)];  reset_at(i) -> [(obs, tour_done, produce_action)]

and, like the reference's workers, resets a finished env inside `step` only when `auto_reset_done` (the collection
loops; evaluation resets through `reset_at`).  The iterative env walks the reference's phases
(ivlnce_baselines/common/environments.py:36-356): after the agent's episode an oracle conveys the agent to the goal
("oracle_goal"), and - when the next episode belongs to the same tour - from there to the next start pose
("oracle_start"); `agent_episode_done` is True in every oracle step, `produce_action` False while the oracle drives,
`tour_done` is only ever reported by a reset, `info["dtw_data"]` carries the positions logged since the last reset
whenever an agent or sim episode ends.  ENVIRONMENT.ITERATIVE.{ORACLE_PHASES, ORACLE_GOAL_PHASE,
PRECISE_EPISODE_START, ORACLE_STEP_ERROR_LIMIT} are honoured.

Habitat-Sim, MP3D and R2R-CE do not exist on the GPU box (simulator side is out of scope, SURVEY.md section 2 rows
8-9): this stand-in feeds the hot path observations of exactly the sensor dtypes/shapes of section 8a row A0, a
scripted expert (`shortest_path_sensor`) and a kinematic agent in obstacle-free space (0.25 m forward / 15 degree
turns; the oracle is a turn-then-advance follower), so positions, tours and t-nDTW are meaningful.

`BoxWorldVectorEnv` (ENV_BACKEND "boxworld") is the same env in a consistent 3-D world: each env lives in a room with
boxes, its depth / semantic12 / rgb are ray-cast from the pose by the mapper's camera model - on the device, where the
mapper and RedNet read them (boxworld.py, csrc/boxworld.hip) - and the agent collides with walls and boxes.
"""
import math
from types import SimpleNamespace
from typing import List

import numpy as np

from .measures import SDTW, ndtw
from .spaces import Box, Dict, Discrete

STOP, FORWARD, LEFT, RIGHT = 0, 1, 2, 3
STEP_M, TURN_RAD = 0.25, math.radians(15.0)


def _advance(pose, heading, a):
    """One kinematic action; returns the new heading (pose is updated in place)."""
    if a == FORWARD:
        pose[0] += np.float32(-STEP_M * math.sin(heading))
        pose[2] += np.float32(-STEP_M * math.cos(heading))
    elif a == LEFT:
        heading += TURN_RAD
    elif a == RIGHT:
        heading -= TURN_RAD
    return heading


def _wrap(a):
    return (a + math.pi) % (2.0 * math.pi) - math.pi


def instruction_features(tokens, L, E):
    """Stand-in for RxRInstructionSensor's pre-computed BERT features (habitat_extensions/sensors.py:119): an (L, E) float32
    array that is a pure function of an instruction's token row - one standard-normal row per token (at most L), zero rows
    past its length, drawn from a generator of its own seeded by the tokens (no other random stream moves)."""
    tok = np.asarray(tokens, np.int64).reshape(-1)
    n = min(int(np.count_nonzero(tok)), int(L))
    seed = int((tok * (np.arange(tok.size, dtype=np.int64) + 1)).sum() % (2 ** 31 - 1))
    out = np.zeros((int(L), int(E)), np.float32)
    out[:n] = np.random.RandomState(seed).standard_normal((n, int(E))).astype(np.float32)
    return out


class _SynthEnv:
    def __init__(self, idx, seed, cfg, episodes_per_tour=3, n_episodes=8, min_len=6, max_len=14, with_rgb=False,
                 with_semantic=True, iterative=False):
        self.idx = idx
        self.rng = np.random.RandomState(seed)
        d = cfg.TASK_CONFIG.SIMULATOR.DEPTH_SENSOR
        self.H, self.W = d.HEIGHT, d.WIDTH
        r = cfg.TASK_CONFIG.SIMULATOR.RGB_SENSOR
        self.rgb_hw = (r.HEIGHT, r.WIDTH)
        self.with_rgb, self.with_semantic = with_rgb, with_semantic
        self.max_steps = cfg.TASK_CONFIG.ENVIRONMENT.MAX_EPISODE_STEPS
        nd = cfg.TASK_CONFIG.TASK.NDTW
        self.ndtw_fdtw, self.ndtw_success_distance = bool(nd.FDTW), float(nd.SUCCESS_DISTANCE)
        it = cfg.TASK_CONFIG.ENVIRONMENT.ITERATIVE
        self.iterative = iterative
        self.oracle_phases, self.oracle_goal_phase = bool(it.ORACLE_PHASES), bool(it.ORACLE_GOAL_PHASE)
        self.precise_start, self.oracle_limit = bool(it.PRECISE_EPISODE_START), int(it.ORACLE_STEP_ERROR_LIMIT)
        # TASK.INSTRUCTION_SENSOR_UUID "rxr_instruction": pre-computed (L, E) text features in place of the tokens
        self.text_features = None
        if cfg.TASK_CONFIG.TASK.INSTRUCTION_SENSOR_UUID == "rxr_instruction":
            self.text_features = (int(cfg.TASK_CONFIG.TASK.RXR_INSTRUCTION_SENSOR.max_text_len),
                                  int(cfg.MODEL.INSTRUCTION_ENCODER.embedding_size))
        self.episodes = []
        starts = np.random.RandomState(seed + 7)  # own stream: scripts / tokens / frames keep their round-1 values
        for e in range(n_episodes):
            n = self.rng.randint(min_len, max_len + 1)
            script = list(self.rng.choice([FORWARD, FORWARD, LEFT, RIGHT], size=n - 1)) + [STOP]
            tokens = np.zeros(200, np.int64)
            L = self.rng.randint(10, 81)
            tokens[:L] = self.rng.randint(2, 2504, size=L)
            off = starts.uniform(-1.0, 1.0, size=2) if iterative else (0.0, 0.0)
            start = np.array([float(idx) * 3.0 + off[0], 1.25, off[1]], np.float32)
            ep = SimpleNamespace(episode_id=f"{idx}_{e}", tour_id=f"tour{idx}_{e // episodes_per_tour}",
                                 scene_id=f"scene{idx}", script=script, tokens=tokens, start=start, start_heading=0.0)
            if self.text_features is not None:
                ep.features = instruction_features(tokens, *self.text_features)
                ep.features.setflags(write=False)  # (handed out at every step without a copy)
            ep.goal = np.array(self._gt_positions(ep)[-1], np.float32)
            self.episodes.append(ep)
        self.ep_i = -1          # nothing loaded: the first reset has no previous episode
        self.phase = "agent"
        self.dtw_data = []      # iterative protocol: positions since the last reset (environments.py:79-86)
        self._tour_log = []     # episodic protocol: every first-pass position (t-nDTW extension, see dtw_data())
        self.exhausted = False  # every episode played once: stop logging (eval pauses the env)
        self.pose = np.zeros(3, np.float32)
        self.heading = 0.0
        self.t = 0
        self._oracle_steps = 0

    @property
    def current_episode(self):
        return self.episodes[self.ep_i % len(self.episodes)]

    # -- observations / metrics ------------------------------------------------------------------
    def _obs(self):
        ep = self.current_episode
        col = self.rng.rand(1, self.W, 1).astype(np.float32)
        depth = np.clip(0.2 + 0.6 * col + 0.02 * self.rng.rand(self.H, self.W, 1).astype(np.float32), 0, 1)
        expert = ep.script[self.t] if (self.phase == "agent" and self.t < len(ep.script)) else STOP
        obs = {
            "depth": depth.astype(np.float32),
            "instruction": ep.tokens.copy(),
            "world_robot_pose": self.pose.copy(),
            "world_robot_orientation": np.array([0.0, self.heading], np.float64),
            "env_name": ep.scene_id,
            "progress": np.array([min(1.0, self.t / max(1, len(ep.script)))], np.float64),
            "shortest_path_sensor": np.array([float(expert)], np.float64),
        }
        if self.text_features is not None:
            del obs["instruction"]
            obs["rxr_instruction"] = ep.features
        if self.with_semantic:
            obs["semantic12"] = self.rng.randint(0, 13, size=(self.H, self.W, 1)).astype(np.uint8)
        if self.with_rgb:
            obs["rgb"] = self.rng.randint(0, 256, size=(*self.rgb_hw, 3)).astype(np.uint8)
        return obs

    @staticmethod
    def _gt_positions(ep):
        pose, heading = ep.start.copy(), ep.start_heading
        pts = [[float(x) for x in pose]]
        for a in ep.script:
            heading = _advance(pose, heading, a)
            if a == FORWARD:
                pts.append([float(x) for x in pose])
        return pts

    def _metrics(self, action, done):
        success = float(done and int(action) == STOP)
        ndtw_v = 0.0
        if done:  # per-episode nDTW / SDTW against the scripted expert's path (measures.py:152-230)
            agent = [p for i, p in enumerate(self._positions) if i == 0 or p != self._positions[i - 1]]
            ndtw_v = ndtw(agent, self._gt_positions(self.current_episode), self.ndtw_success_distance, self.ndtw_fdtw)
        return {"distance_to_goal": float(np.linalg.norm((self.pose - self.current_episode.goal)[[0, 2]])),
                "success": success, "spl": 0.0, "ndtw": ndtw_v, "sdtw": SDTW.get_metric(success, ndtw_v),
                "path_length": STEP_M * self.t, "oracle_success": 0.0, "steps_taken": float(self.t)}

    def _load_next_episode(self):
        if self.ep_i + 1 >= len(self.episodes):
            self.exhausted = True
        self.ep_i += 1
        self.t = 0

    def _place_at_start(self):
        ep = self.current_episode
        self.pose, self.heading = ep.start.copy(), ep.start_heading
        self._positions = [[float(x) for x in self.pose]]

    def _agent_step(self, action):
        self.heading = _advance(self.pose, self.heading, int(action))
        self.t += 1
        self._positions.append([float(x) for x in self.pose])
        return int(action) == STOP or self.t >= min(self.max_steps, 4 * len(self.current_episode.script))

    # -- episodic protocol --------------------------------------------------------------------------
    def _log_episodic(self):
        if not self.exhausted:
            self._tour_log.append({"position": [float(x) for x in self.pose], "phase": "agent",
                                   "episode_id": self.current_episode.episode_id})

    def reset_episodic(self):
        self._load_next_episode()
        self.phase = "agent"
        self._place_at_start()
        self._log_episodic()
        return self._obs()

    def step_episodic(self, action, auto_reset):
        done = self._agent_step(action)
        self._log_episodic()
        info = self._metrics(action, done)
        obs = self.reset_episodic() if (done and auto_reset) else self._obs()
        return obs, 0.0, done, info

    # -- iterative protocol -------------------------------------------------------------------------
    def _oracle_action(self, position_to, heading_to):
        """Turn-then-advance follower with the stopping rules of `_get_next_action` (environments.py:195-229): STOP
        within one forward step of the target and, when a heading is asked for, within half a turn of it."""
        dx, dz = float(position_to[0] - self.pose[0]), float(position_to[2] - self.pose[2])
        if math.hypot(dx, dz) >= STEP_M:
            delta = _wrap(math.atan2(-dx, -dz) - self.heading)
            if abs(delta) >= TURN_RAD / 2:
                return LEFT if delta > 0 else RIGHT
            return FORWARD
        if heading_to is not None:
            delta = _wrap(heading_to - self.heading)
            if abs(delta) >= TURN_RAD / 2:
                return LEFT if delta > 0 else RIGHT
        return STOP

    def _oracle_action_safe(self, position_to, heading_to, teleport_on_failure):
        """`_get_next_action_safe` (:149-193): past ORACLE_STEP_ERROR_LIMIT the oracle gives up (teleporting to the
        target if asked to) and calls STOP."""
        if 0 <= self.oracle_limit <= self._oracle_steps:
            if teleport_on_failure:
                self.pose = np.array(position_to, np.float32)
                if heading_to is not None:
                    self.heading = heading_to
            return STOP
        return self._oracle_action(position_to, heading_to)

    def _next_phase(self):
        self.phase = {"agent": "oracle_goal", "oracle_goal": "oracle_start", "oracle_start": "agent"}[self.phase]
        self._oracle_steps = 0

    def reset(self):
        """(:91-147) -> (observations, tour_done, produce_action)."""
        self.dtw_data = []
        self.phase = "agent"
        self._oracle_steps = 0
        first = self.ep_i < 0
        prev_tour = None if first else self.current_episode.tour_id
        prev_pose, prev_heading = self.pose.copy(), self.heading
        self._load_next_episode()
        self._place_at_start()
        observations = self._obs()
        if first:
            return observations, True, True
        tour_done = prev_tour != self.current_episode.tour_id
        produce_action = True
        if tour_done or not self.oracle_phases:
            return observations, tour_done, produce_action
        # same tour: back to where the previous episode ended; the oracle walks to the new start from there
        self.phase = "oracle_start"
        self.pose, self.heading = prev_pose, prev_heading
        ep = self.current_episode
        if self._oracle_action_safe(ep.start, ep.start_heading, True) == STOP:
            self._next_phase()
            self._positions = [[float(x) for x in self.pose]]
        else:
            produce_action = False
        return observations, tour_done, produce_action

    def _step_oracle(self):
        ep = self.current_episode
        to, heading_to = (ep.goal, None) if self.phase == "oracle_goal" else (ep.start, ep.start_heading)
        self.heading = _advance(self.pose, self.heading, self._oracle_action(to, heading_to))
        nxt = self._oracle_action_safe(to, heading_to, self.phase == "oracle_start")
        if nxt == STOP:
            if self.phase == "oracle_start":
                if self.precise_start:
                    self.pose, self.heading = ep.start.copy(), ep.start_heading
                self._positions = [[float(x) for x in self.pose]]
            self._next_phase()
        else:
            self._oracle_steps += 1
        return self._obs()

    def step(self, action, auto_reset):
        """(:287-356) -> (observations, reward, agent_episode_done, sim_episode_done, tour_done, produce_action, info)."""
        agent_done, sim_done, tour_done, produce_action, info = True, False, False, False, {}
        if not self.exhausted:
            self.dtw_data.append({"position": [float(x) for x in self.pose], "phase": self.phase,
                                  "episode_id": self.current_episode.episode_id})
        if self.phase == "agent":
            agent_done = self._agent_step(action)
            produce_action = True
            info = self._metrics(action, agent_done)
            if agent_done:
                self._next_phase()
                produce_action = False
                if not self.oracle_phases:
                    self.phase = "agent"
                    sim_done = True
                elif (self._oracle_action_safe(self.current_episode.goal, None, False) == STOP
                      or not self.oracle_goal_phase):
                    self._next_phase()
                    sim_done = True
            observations = self._obs()
        elif self.phase == "oracle_goal":
            observations = self._step_oracle()
            sim_done = self.phase == "oracle_start"
        else:
            observations = self._step_oracle()
            produce_action = self.phase == "agent"
        if agent_done or sim_done:
            info["dtw_data"] = [dict(p) for p in self.dtw_data]  # the worker pipe pickles it: a snapshot
        if auto_reset and sim_done:
            observations, tour_done, produce_action = self.reset()
        return observations, 0.0, agent_done, sim_done, tour_done, produce_action, info

    def expert_path(self):
        """Positions of the scripted expert for every episode, tour-grouped (ground truth for t-nDTW: what
        `EVAL.ITERATIVE_GT_PATHS[split]` holds for the real dataset)."""
        out = {}
        for ep in self.episodes:
            pose, heading = ep.start.copy(), ep.start_heading
            pts = [{"position": [float(x) for x in pose], "phase": "agent", "episode_id": ep.episode_id}]
            for a in ep.script:
                heading = _advance(pose, heading, a)
                pts.append({"position": [float(x) for x in pose], "phase": "agent", "episode_id": ep.episode_id})
            out.setdefault(ep.tour_id, []).extend(pts)
        return out


class SyntheticVectorEnv:
    _ENV = _SynthEnv  # the per-env class (BoxWorldVectorEnv: _BoxEnv)

    def __init__(self, config, num_envs=None, seed=None, rank=0, world=1, iterative=None, auto_reset_done=True,
                 **env_kw):
        n = num_envs if num_envs is not None else config.NUM_ENVIRONMENTS
        seed = config.TASK_CONFIG.SEED if seed is None else seed
        self.iterative = ("Iterative" in str(config.ENV_NAME)) if iterative is None else bool(iterative)
        self.auto_reset_done = bool(auto_reset_done)
        # envs sharded round-robin over ranks like construct_envs splits scenes (env_utils.py:77-99)
        ids = [i for i in range(n * world) if i % world == rank]
        # RGB frames only for policies that read them (RedNet-predicted semantics, Latent-CMA): they are 150 KB
        # of host RNG per step and env otherwise
        needs_rgb = (config.MODEL.policy_name == "LatentCMAPolicy"
                     or any("Predicted" in t for t in config.RL.POLICY.OBS_TRANSFORMS.ENABLED_TRANSFORMS))
        env_kw.setdefault("with_rgb", needs_rgb)
        self._envs: List[_SynthEnv] = [self._ENV(i, seed + 1000 * i, config, iterative=self.iterative, **env_kw)
                                       for i in ids]
        self._paused: List[_SynthEnv] = []
        d = config.TASK_CONFIG.SIMULATOR.DEPTH_SENSOR
        sp = {
            "depth": Box(0.0, 1.0, (d.HEIGHT, d.WIDTH, 1), np.float32),
            "instruction": Box(0, 2504, (200,), np.int64),
            "world_robot_pose": Box(-1e6, 1e6, (3,), np.float32),
            "world_robot_orientation": Box(-1e6, 1e6, (2,), np.float64),
            "semantic12": Box(0, 12, (d.HEIGHT, d.WIDTH, 1), np.uint8),
            "progress": Box(0.0, 1.0, (1,), np.float64),
            "shortest_path_sensor": Box(0.0, 100.0, (1,), np.float64),
        }
        if config.TASK_CONFIG.TASK.INSTRUCTION_SENSOR_UUID == "rxr_instruction":
            del sp["instruction"]
            sp["rxr_instruction"] = Box(-np.inf, np.inf, self._envs[0].text_features if self._envs else (512, 768), np.float32)
        if env_kw["with_rgb"]:
            r = config.TASK_CONFIG.SIMULATOR.RGB_SENSOR
            sp["rgb"] = Box(0, 255, (r.HEIGHT, r.WIDTH, 3), np.uint8)
        self.observation_spaces = [Dict(dict(sp)) for _ in self._envs]
        self.action_spaces = [Discrete(4) for _ in self._envs]

    @property
    def num_envs(self):
        return len(self._envs)

    @property
    def number_of_episodes(self):
        return [len(e.episodes) for e in self._envs]

    def reset(self):
        return [e.reset() if self.iterative else e.reset_episodic() for e in self._envs]

    def step(self, actions):
        if self.iterative:
            return [e.step(a, self.auto_reset_done) for e, a in zip(self._envs, actions)]
        return [e.step_episodic(a, self.auto_reset_done) for e, a in zip(self._envs, actions)]

    def reset_at(self, i):
        return [self._envs[i].reset() if self.iterative else self._envs[i].reset_episodic()]

    def pause_at(self, i):
        self._paused.append(self._envs.pop(i))
        self.observation_spaces.pop(i)
        self.action_spaces.pop(i)

    def current_episodes(self):
        return [e.current_episode for e in self._envs]

    def dtw_data(self):
        """Episodic protocol only: the first-pass positions of every env, tour-grouped.  (The reference's episodic
        evaluation reports no t-nDTW; the iterative one collects `infos["dtw_data"]`.)"""
        out = {}
        for e in self._envs + self._paused:
            for p in e._tour_log:
                tour = next(ep.tour_id for ep in e.episodes if ep.episode_id == p["episode_id"])
                out.setdefault(tour, []).append(p)
        return out

    def gt_paths(self):
        out = {}
        for e in self._envs + self._paused:
            out.update(e.expert_path())
        return out

    def close(self):
        self._envs, self._paused = [], []


class _BoxEnv(_SynthEnv):
    """`_SynthEnv` in a box-world scene (boxworld.make_scene): the episodes, scripts and tokens are drawn exactly as the
    parent draws them, then every script is simulated against the scene and a FORWARD that would be blocked is replaced
    by a LEFT turn, so the scripted expert and `expert_path` are collision-free.  The agent is a disc of
    SIMULATOR.AGENT_0.RADIUS: a FORWARD that would leave the room or enter a box footprint grown by the radius leaves the
    pose unchanged.  A blocked oracle step uses up the oracle's error budget at once (`_oracle_action_safe` gives up,
    teleporting where the parent would): the turn-then-advance follower has no way round a box.  The frames are not made
    here: the vector env renders all its envs in one call and fills them in."""

    def __init__(self, idx, seed, cfg, **kw):
        super().__init__(idx, seed, cfg, **kw)
        from .boxworld import intrinsics, make_scene

        sim = cfg.TASK_CONFIG.SIMULATOR
        self.radius = float(sim.AGENT_0.RADIUS)
        self.depth_cam = (math.radians(float(sim.DEPTH_SENSOR.HFOV)), float(sim.DEPTH_SENSOR.MIN_DEPTH),
                          float(sim.DEPTH_SENSOR.MAX_DEPTH))
        self.rgb_hfov = math.radians(float(sim.RGB_SENSOR.HFOV))
        self.depth_f = intrinsics(self.H, self.W, self.depth_cam[0])
        self.rgb_f = intrinsics(*self.rgb_hw, self.rgb_hfov)
        self.scene_name = f"bw{idx}"
        self.scene = make_scene(seed + 13, cfg, origin=(float(idx) * 3.0, 0.0, 0.0),
                                starts=[ep.start for ep in self.episodes])
        self.scene_index = -1  # its entry in the device renderer's table (BoxWorldVectorEnv)
        self._oracle_blocked = False
        for ep in self.episodes:
            if self.scene.blocked(ep.start, self.radius):
                raise ValueError(f"box-world scene {self.scene_name}: the start of episode {ep.episode_id} is not free "
                                 "(BOXWORLD.ROOM_SIZE too small for the episode starts?)")
            ep.scene_id = self.scene_name
            pose, heading = ep.start.copy(), ep.start_heading
            for t, a in enumerate(ep.script):
                if a == FORWARD and self._forward_blocked(pose, heading):
                    a = ep.script[t] = LEFT
                heading = _advance(pose, heading, a)
            ep.goal = np.array(self._gt_positions(ep)[-1], np.float32)

    def _forward_blocked(self, pose, heading):
        p = pose.copy()
        _advance(p, heading, FORWARD)
        return self.scene.blocked(p, self.radius)

    def _move(self, a):
        """One action under collision; False when a FORWARD was blocked (the pose is unchanged)."""
        if a == FORWARD and self._forward_blocked(self.pose, self.heading):
            return False
        self.heading = _advance(self.pose, self.heading, a)
        return True

    def _obs(self):
        ep = self.current_episode
        expert = ep.script[self.t] if (self.phase == "agent" and self.t < len(ep.script)) else STOP
        obs = {
            "depth": None,  # (filled by the vector env's batched render, like semantic12 / rgb below)
            "instruction": ep.tokens.copy(),
            "world_robot_pose": self.pose.copy(),
            "world_robot_orientation": np.array([0.0, self.heading], np.float64),
            "env_name": ep.scene_id,
            "progress": np.array([min(1.0, self.t / max(1, len(ep.script)))], np.float64),
            "shortest_path_sensor": np.array([float(expert)], np.float64),
        }
        if self.text_features is not None:
            del obs["instruction"]
            obs["rxr_instruction"] = ep.features
        if self.with_semantic:
            obs["semantic12"] = None
        if self.with_rgb:
            obs["rgb"] = None
        return obs

    def render_host(self, obs):
        """The CPU path: this env's frames from `boxworld.render_reference`, as numpy arrays."""
        from .boxworld import render_reference

        pose, heading = obs["world_robot_pose"], float(obs["world_robot_orientation"][1])
        _, dmin, dmax = self.depth_cam
        f = render_reference(self.scene, pose, heading, self.H, self.W, *self.depth_f, dmin, dmax, with_rgb=False)
        obs["depth"] = f["depth"][..., None]
        if self.with_semantic:
            obs["semantic12"] = f["labels"][..., None]
        if self.with_rgb:
            obs["rgb"] = render_reference(self.scene, pose, heading, *self.rgb_hw, *self.rgb_f, dmin, dmax)["rgb"]

    def _agent_step(self, action):
        self._move(int(action))
        self.t += 1
        self._positions.append([float(x) for x in self.pose])
        return int(action) == STOP or self.t >= min(self.max_steps, 4 * len(self.current_episode.script))

    def _oracle_action_safe(self, position_to, heading_to, teleport_on_failure):
        if self._oracle_blocked:  # the budget is spent: the parent's give-up branch
            self._oracle_blocked = False
            if teleport_on_failure:
                self.pose = np.array(position_to, np.float32)
                if heading_to is not None:
                    self.heading = heading_to
            return STOP
        return super()._oracle_action_safe(position_to, heading_to, teleport_on_failure)

    def _next_phase(self):
        super()._next_phase()
        self._oracle_blocked = False

    def _step_oracle(self):
        ep = self.current_episode
        to, heading_to = (ep.goal, None) if self.phase == "oracle_goal" else (ep.start, ep.start_heading)
        self._oracle_blocked = not self._move(self._oracle_action(to, heading_to))
        nxt = self._oracle_action_safe(to, heading_to, self.phase == "oracle_start")
        if nxt == STOP:
            if self.phase == "oracle_start":
                if self.precise_start:
                    self.pose, self.heading = ep.start.copy(), ep.start_heading
                self._positions = [[float(x) for x in self.pose]]
            self._next_phase()
        else:
            self._oracle_steps += 1
        return self._obs()


class BoxWorldVectorEnv(SyntheticVectorEnv):
    """`SyntheticVectorEnv` whose observations are a consistent 3-D world (ENV_BACKEND "boxworld"): env i lives in scene
    `bw{i}` and its depth, semantic12 and rgb are ray-cast from its pose by the mapper's own camera model (boxworld.py).
    Same step protocols, kwargs, observation keys, dtypes, shapes and spaces as the parent.  On a GPU all envs of a step
    are rendered in ONE call (csrc/boxworld.hip) and the three frame entries of every observation are device-tensor views
    of the batched buffers, valid through the next step - `utils.batch_obs` stacks them without a host round trip; on the
    CPU they are numpy arrays from `boxworld.render_reference` (the same bits).  `device`: where to render ("cpu", a cuda
    device; default: cuda:TORCH_GPU_ID when there is one)."""
    _ENV = _BoxEnv

    def __init__(self, config, *args, device=None, **kw):
        import torch

        super().__init__(config, *args, **kw)
        if device is None:
            device = torch.device("cuda", int(config.TORCH_GPU_ID)) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self._renderer = None
        if self.device.type == "cuda" and self._envs:
            from .boxworld import BoxWorldRenderer

            e0 = self._envs[0]
            hfov, dmin, dmax = e0.depth_cam
            self._renderer = BoxWorldRenderer(self.device, len(self._envs), (e0.H, e0.W), hfov, dmin, dmax,
                                              rgb_hw=e0.rgb_hw if e0.with_rgb else None, rgb_hfov_rad=e0.rgb_hfov)
            for e in self._envs:
                e.scene_index = self._renderer.add_scene(e.scene)

    def _fill(self, observations):
        """The frames of every env's observation: one render call on a GPU."""
        envs = self._envs
        if self._renderer is None:
            for e, o in zip(envs, observations):
                e.render_host(o)
            return
        fr = self._renderer.render([e.scene_index for e in envs], [o["world_robot_pose"] for o in observations],
                                   [o["world_robot_orientation"][1] for o in observations], with_rgb=envs[0].with_rgb)
        for b, (e, o) in enumerate(zip(envs, observations)):
            self._assign(e, o, {k: v[b] for k, v in fr.items()})

    @staticmethod
    def _assign(e, o, fr):
        o["depth"] = fr["depth"]
        if e.with_semantic:
            o["semantic12"] = fr["labels"]
        if e.with_rgb:
            o["rgb"] = fr["rgb"]

    def reset(self):
        out = super().reset()
        if out:
            self._fill([x[0] for x in out] if self.iterative else out)
        return out

    def step(self, actions):
        out = super().step(actions)
        if out:
            self._fill([x[0] for x in out])
        return out

    def reset_at(self, i):
        out = super().reset_at(i)
        e, o = self._envs[i], (out[0][0] if self.iterative else out[0])
        if self._renderer is None:
            e.render_host(o)
        else:  # row i's own buffers: the other envs' views of the last step stay what they are
            self._assign(e, o, self._renderer.render_row(i, e.scene_index, o["world_robot_pose"],
                                                         o["world_robot_orientation"][1], with_rgb=e.with_rgb))
        return out

    def scenes(self):
        """{scene name: boxworld.Scene} of every env, paused ones included."""
        return {e.scene_name: e.scene for e in self._envs + self._paused}

    def check_status(self):
        if self._renderer is not None:
            self._renderer.check_status()

    def close(self):
        super().close()
        self._renderer = None


def construct_envs(config, env_class=None, auto_reset_done=True, rank=0, world=1, **kw):
    """The vector env the trainers of this package drive (the reference: env_utils.py:25-114; `auto_reset_done`
    False = `construct_envs_auto_reset_false`).  The step protocol follows `config.ENV_NAME` ("Iterative" in the
    name -> the 7-tuple protocol) unless `iterative=` says otherwise.

    Two backends exist in this scope (simulator side: SURVEY.md section 2 rows 8-9), neither of them Habitat: "synthetic"
    (`SyntheticVectorEnv`: frames are noise, the default of this package's config) and "boxworld" (`BoxWorldVectorEnv`:
    frames ray-cast from the pose in a room with boxes, on the device).  The choice is explicit: `config.ENV_BACKEND` or
    the IVLN_ENV_BACKEND environment variable; anything else fails loudly instead of silently training on synthetic
    observations.  The trainers themselves speak the reference's env protocol, so a Habitat `ExtendedVectorEnv` can be
    handed to them where Habitat exists."""
    import os

    backend = os.environ.get("IVLN_ENV_BACKEND") or str(getattr(config, "ENV_BACKEND", "synthetic"))
    if backend == "boxworld":
        return BoxWorldVectorEnv(config, rank=rank, world=world, auto_reset_done=auto_reset_done, **kw)
    if backend != "synthetic":
        raise NotImplementedError(
            f"ENV_BACKEND={backend!r}: ivln_ce_amd.envs builds the synthetic and the boxworld vector envs only; real "
            "Habitat envs come from the reference's construct_envs (same step protocol)")
    return SyntheticVectorEnv(config, rank=rank, world=world, auto_reset_done=auto_reset_done, **kw)
