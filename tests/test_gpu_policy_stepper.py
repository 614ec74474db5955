"""The rollout loops' step driver (trainers._PolicyStepper) without envs: replayed as captured graphs against eager, across
a pause - the way bench.py's collection leg drives the sampled driver (trainers._RolloutStepper)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Envs:
    """What `_pause_envs` needs of a vector env."""

    def __init__(self, n):
        self.num_envs = n

    def pause_at(self, idx):
        self.num_envs -= 1


def test_deterministic_driver_replayed_equals_eager_across_a_pause(same_depth_path):
    """Six steps of `_episode_script` at B = 4 through `_PolicyStepper.step`, as the episodic eval loop calls it.  After the
    third step env 1 pauses: `before_pause` on the next (still four-row) batch, then `_pause_envs` drops row 1 from the
    state, the mask and that batch, and the remaining observations arrive with three rows.  With `use_graph` the driver
    has to capture for four rows (warm-up, mapper reset), take the step after the pause eagerly on the batch
    `before_pause` mapped, and capture again for three rows WITHOUT stepping the mapper's world cloud; every step's
    actions and recurrent state then equal the eager driver's bit for bit (the depth encoder pinned to the launch chain
    for both)."""
    same_depth_path(0)
    from test_gpu_policy import _episode_script, make_policy

    from ivln_ce_amd import trainers
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.obs_transforms import GTSemanticsIterativeMapper, apply_obs_transforms_batch

    dev = torch.device("cuda:0")
    cfg = get_config()
    pol = make_policy()
    B, steps, pause_after, keep = 4, 6, 3, [0, 2, 3]
    obs, _ = _episode_script(B, steps)

    def run(use_graph):
        tr = trainers.BaseVLNCETrainer.__new__(trainers.BaseVLNCETrainer)
        tr.config, tr.device, tr.policy = cfg, dev, pol
        tr.rank, tr.local_rank, tr.world = 0, 0, 1
        tr.obs_transforms = [GTSemanticsIterativeMapper.from_config(cfg)]
        captures, replayed = [], []
        make_runner, stepper = tr._make_runner, trainers._PolicyStepper(tr, False, use_graph, deterministic=True)
        launch = stepper.launch

        def points():  # of the world cloud (the transformer creates its mapper with the first batch it sees)
            mapper = tr.obs_transforms[0].mapping_module
            return 0 if mapper is None else mapper.status()[1]

        def counted_make_runner(*a, **k):
            before = points()
            runner = make_runner(*a, **k)
            captures.append((before, points()))
            return runner

        def logged_launch(*a):
            out = launch(*a)
            replayed.append(out[2])
            return out

        tr._make_runner, stepper.launch = counted_make_runner, logged_launch

        def batch_of(t, rows=None):  # the loops' `_batch(..., transform=not use_graph)`
            rows = range(B) if rows is None else rows
            b = {k: (v[list(rows)] if torch.is_tensor(v) else [v[i] for i in rows]) for k, v in obs[t].items()}
            return b if use_graph else apply_obs_transforms_batch(b, tr.obs_transforms)

        rnn, prev, masks = tr._initial_state(cfg, B)
        envs, out = _Envs(B), []
        batch = batch_of(0)
        for t in range(steps):
            masks = batch["not_done_masks"]
            with torch.no_grad():
                prev, rnn = stepper.step(batch, rnn, prev, (masks,))
            out.append((prev.clone(), rnn.clone()))
            if t + 1 == steps:
                break
            if t + 1 == pause_after:
                batch = stepper.before_pause(batch_of(t + 1))
                envs, rnn, masks, prev, batch, _ = tr._pause_envs([1], envs, rnn, masks, prev, batch)
                assert envs.num_envs == len(keep) and rnn.shape[0] == len(keep)
            else:
                batch = batch_of(t + 1, rows=None if t + 1 < pause_after else keep)
        stepper.close()
        tr._check_mappers()
        return out, captures, replayed

    eager, captures, replayed = run(False)
    assert captures == [] and replayed == [False] * steps
    graphed, captures, replayed = run(True)
    assert replayed == [True, True, True, False, True, True], "only the step right after the pause runs eagerly"
    assert len(captures) == 2, "one capture per batch size"
    assert captures[1][0] == captures[1][1] > 0, f"the re-capture stepped the world cloud: {captures[1]}"
    for t in range(steps):
        assert graphed[t][0].shape[0] == (B if t < pause_after else len(keep))
        assert torch.equal(graphed[t][0], eager[t][0]), f"actions step {t}"
        assert torch.equal(graphed[t][1], eager[t][1]), f"rnn step {t}"
