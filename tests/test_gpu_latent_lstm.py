"""GPU: Latent-CMA with LSTM state encoders (`MODEL.STATE_ENCODER.rnn_type: LSTM`) against the float64 torch oracle of
tests/latent_lstm_ref.py (pinned to the reference's own numbers by tests/test_latent_lstm_host.py), in the three memory
modes: episodic ("plain"), `tour_memory` ("tour") and `tour_memory_variant` + `memory_at_end` ("variant"), whose first
encoder runs through ivln_lstm_seq_tour_fwd_f32 (include/ivln_tour_state.h).

Bars
  rollout steps / build_distribution   logits 1e-4, features and states 2e-4 (tests/test_gpu_latent.py,
                                       tests/test_gpu_lstm_state.py)
  one update                           loss and every gradient  err <= 4 * e32 + 4 * 2^-24 * max|ref|  against float64
                                       autograd of the oracle's loss, e32 = the oracle's own float32 run
                                       (tests/test_gpu_instruction_options._Bar, factor 4)
  graph replay                         the bytes of the eager step
Cached image features everywhere except the graph test, one N = 2 step loop on frames.  Every comparison is printed before
anything is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

from latent_lstm_ref import MODES, LatentCMAPolicyLSTMRef, make_policy

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
DEV = "cuda:0"
EPS = 2.0 ** -24
T, N, H = 3, 2, 512


class _Bar:
    """tests/test_gpu_instruction_options._Bar"""

    def __init__(self, case):
        self.case, self.bad = case, []

    def check(self, name, got, ref64, ref32, factor=4.0):
        got = got.detach().cpu().double().reshape(-1)
        r64, r32 = ref64.detach().double().reshape(-1), ref32.detach().double().reshape(-1)
        assert got.shape == r64.shape == r32.shape, (name, got.shape, r64.shape, r32.shape)
        err, e32, mx = float((got - r64).abs().max()), float((r32 - r64).abs().max()), float(r64.abs().max())
        bar = factor * e32 + 4 * EPS * mx
        ok = err <= bar  # (False for NaN)
        line = f"{self.case:18s} {name:58s} hip {err:.3e}  e32 {e32:.3e}  max|ref| {mx:.3e}  bar {bar:.3e}  {'ok' if ok else 'OVER'}"
        print(line)
        if not ok:
            self.bad.append(line)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


_batches = {}


def _batch(mode):
    """A time-major (T, N) batch on cached features: every row starts an episode at t = 0, row 0 also a tour; row 1 starts
    its next episode at t = 2 INSIDE its tour.  A carried state in the tour modes (the variant keeps only its memory slot,
    iterative_dagger_trainer.py:58-60)."""
    if mode in _batches:
        return _batches[mode]
    from gen_latent_update_features import features

    seed = 300 + MODES.index(mode)
    g = torch.Generator().manual_seed(seed)
    rgb_np, dep_np = features(seed, T, N)
    instr = torch.zeros(N, 200)
    for n, ln in enumerate((41, 7)):
        instr[n, :ln] = torch.randint(2, 2504, (ln,), generator=g).float()
    obs = {"rgb_features": torch.from_numpy(rgb_np), "depth_features": torch.from_numpy(dep_np),
           "instruction": instr.repeat(T, 1), "progress": torch.rand(T * N, 1, generator=g)}
    ep, tour = torch.ones(T, N, dtype=torch.uint8), torch.ones(T, N, dtype=torch.uint8)
    ep[0] = 0
    ep[2, 1] = 0
    tour[0, 0] = 0
    L = 5 if mode == "variant" else 4
    h0 = torch.zeros(N, L, H) if mode == "plain" else 0.3 * torch.randn(N, L, H, generator=g)
    if mode == "variant":
        h0[:, :4] = 0
    w = torch.where(torch.rand(T, N, generator=g) < 0.5, torch.tensor(3.2), torch.tensor(1.0))
    w[2, 0] = 0.0
    _batches[mode] = dict(obs=obs, prev=torch.randint(0, 4, (T * N, 1), generator=g), ep=ep.view(-1, 1), tour=tour.view(-1, 1),
                          h0=h0, targets=torch.randint(0, 4, (T, N), generator=g), weights=w)
    return _batches[mode]


def _dev(x):
    return {k: v.to(DEV) for k, v in x.items()} if isinstance(x, dict) else x.to(DEV)


@pytest.mark.parametrize("mode", MODES)
def test_rollout_steps_and_distribution_match_the_oracle(mode):
    torch.set_num_threads(8)
    b = _batch(mode)
    pol = make_policy("LSTM", mode).to(DEV).eval()
    ref = LatentCMAPolicyLSTMRef(mode).load_from(pol).double().eval()
    assert pol.net.num_recurrent_layers == b["h0"].shape[1] == ref.net.num_recurrent_layers
    seen = {}
    pol.net.register_forward_hook(lambda mod, args, o: seen.__setitem__("f", o[0]))
    # a carried state in every mode, so that the episode mask has something to clear
    g = torch.Generator().manual_seed(9)
    rnn = 0.3 * torch.randn(N, pol.net.num_recurrent_layers, H, generator=g)
    rnn_d, rnn_r = rnn.to(DEV), rnn.double()
    worst = []
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        o = {k: v[sl] for k, v in b["obs"].items()}
        prev, ep, tour = b["prev"][sl], b["ep"][sl], b["tour"][sl]
        with torch.no_grad():
            act, rnn_d = pol.act_iterative(_dev(o), rnn_d, _dev(prev), _dev(ep), _dev(ep), _dev(tour), _dev(ep),
                                           deterministic=True)
            lg = pol.action_distribution.raw_logits(seen["f"])
            lr, rnn_r, fr = ref.act_step({k: v.double() for k, v in o.items()}, rnn_r, prev, ep, tour)
        e = (float((lg.cpu().double() - lr).abs().max()), float((seen["f"].cpu().double() - fr).abs().max()),
             float((rnn_d.cpu().double() - rnn_r).abs().max()))
        print(f"{mode:8s} step {t}: logits {e[0]:.3e}  features {e[1]:.3e}  states {e[2]:.3e}")
        worst.append(e)
        assert float((lr.max(-1, keepdim=True).values - lr.gather(1, act.cpu())).max()) < 2e-4  # the oracle's arg-max, up to ties
    if mode == "variant":  # the slot did something: cleared for row 0 at the tour start, pooled afterwards
        assert bool((rnn_r[:, 4] >= rnn_r[:, 0]).all()) and torch.equal(rnn_d[:, 4], torch.max(rnn_d[:, 4], rnn_d[:, 0]))
    # build_distribution over T * N rows as the trainers call it: autograd on, saves taken
    pol.train()
    dist, rnn_out = pol.build_distribution(_dev(b["obs"]), _dev(b["h0"]), _dev(b["prev"]), _dev(b["ep"]), _dev(b["tour"]))
    assert dist.logits.requires_grad
    with torch.no_grad():
        lr, st_r, _ = ref.build_logits({k: v.double() for k, v in b["obs"].items()}, b["h0"].double(), b["prev"], b["ep"],
                                       b["tour"])
    e_l = float((dist.logits.detach().cpu().double() - torch.log_softmax(lr, -1)).abs().max())
    e_s = float((rnn_out.cpu().double() - st_r).abs().max())
    print(f"{mode:8s} build_distribution T={T}: logits {e_l:.3e}  states {e_s:.3e}")
    assert all(e[0] < 1e-4 and e[1] < 2e-4 and e[2] < 2e-4 for e in worst), worst
    assert e_l < 1e-4 and e_s < 2e-4
    # the GRU configuration built beside it keeps its 2 / 3 state slots, and runs
    gru = make_policy("GRU", mode).to(DEV).eval()
    Lg = 3 if mode == "variant" else 2
    assert gru.net.num_recurrent_layers == Lg
    o = {k: v[:N] for k, v in b["obs"].items()}
    with torch.no_grad():
        _, st = gru.act_iterative(_dev(o), torch.zeros(N, Lg, H, device=DEV), _dev(b["prev"][:N]), _dev(b["ep"][:N]),
                                  _dev(b["ep"][:N]), _dev(b["tour"][:N]), _dev(b["ep"][:N]), deterministic=True)
    assert tuple(st.shape) == (N, Lg, H) and bool(torch.isfinite(st).all())


@pytest.mark.parametrize("mode", MODES)
def test_update_loss_and_every_gradient_match_float64_autograd(mode):
    from ivln_ce_amd.aux_losses import AuxLosses
    from ivln_ce_amd.trainers import FlatAdam, update_agent

    torch.set_num_threads(8)
    b = _batch(mode)
    use_pm = mode == "plain"
    pol = make_policy("LSTM", mode, use_pm=use_pm).to(DEV).train()
    res = {}
    for dt in (torch.float64, torch.float32):
        ref = LatentCMAPolicyLSTMRef(mode, use_pm=use_pm).load_from(pol).to(dt).train()
        loss, _, _, _, states = ref.update_loss({k: v.to(dt) for k, v in b["obs"].items()}, b["h0"].to(dt), b["prev"], b["ep"],
                                                b["tour"], b["targets"], b["weights"].to(dt))
        loss.backward()
        res[dt] = dict(loss=loss.detach(), states=states.detach(),
                       grads={k: p.grad.detach() for k, p in ref.named_parameters() if p.grad is not None})
    opt = FlatAdam(pol, lr=2.5e-4)
    if use_pm:
        AuxLosses.activate()
    try:
        out = update_agent(pol, opt, _dev(b["obs"]), _dev(b["prev"]), _dev(b["ep"]), _dev(b["targets"]), _dev(b["weights"]),
                           hidden_size=H, step_grad=False, tour_not_done_masks=_dev(b["tour"]), rnn_states=_dev(b["h0"]))
    finally:
        AuxLosses.deactivate()
    r64, r32 = res[torch.float64], res[torch.float32]
    bar = _Bar(mode + " update")
    bar.check("loss", torch.tensor(out[0]), r64["loss"], r32["loss"])
    bar.check("states out", out[3], r64["states"], r32["states"])
    params = dict(pol.named_parameters())
    assert len(r64["grads"]) >= 38
    for k, g64 in r64["grads"].items():
        assert params[k].grad is not None, k
        bar.check(k[4:] if k.startswith("net.") else k, params[k].grad, g64, r32["grads"][k])
    # a parameter the loss does not reach (the progress monitor when it is off) may carry a gradient of exact zeros only
    extra = [k for k, p in params.items() if p.grad is not None and k not in r64["grads"] and bool((p.grad != 0).any())]
    assert not extra, extra
    bar.done()


@pytest.mark.parametrize("mode", MODES)
def test_graph_replay_of_the_step_is_bit_identical_to_eager(mode, same_depth_path):
    """on frames: the RGB ResNet-50 and the depth ResNet run inside the step"""
    same_depth_path(0)
    from ivln_ce_amd.graphed import GraphedRollout
    from ivln_ce_amd.synthetic import SyntheticRollout

    steps = 3
    pol = make_policy("LSTM", mode).to(DEV).eval()
    roll = SyntheticRollout(B=N, seed=17, with_rgb=True)
    obs = []
    for t in range(steps):
        o = roll.step()
        o["instruction"][1, 11:] = 0
        o = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in o.items()}
        o["not_done_masks"] = torch.tensor([[0], [0]] if t == 0 else ([[1], [1]] if t == 1 else [[1], [0]]),
                                           dtype=o["not_done_masks"].dtype, device=DEV)
        obs.append(o)
    L = pol.net.num_recurrent_layers
    rnn = torch.zeros(N, L, H, device=DEV)
    prev = torch.zeros(N, 1, dtype=torch.long, device=DEV)
    eager = []
    for o in obs:
        with torch.no_grad():
            a, rnn = pol.act(dict(o), rnn, prev, o["not_done_masks"], deterministic=True)
        prev = a
        eager.append((a.clone(), rnn.clone()))
    assert bool((eager[-1][1] != 0).any())
    runner = GraphedRollout(pol, [], obs[0], deterministic=True)
    runner.reset_state()
    for t, o in enumerate(obs):
        a = runner.step(o)
        torch.cuda.synchronize()
        assert torch.equal(a, eager[t][0]), f"actions step {t}"
        assert torch.equal(runner.rnn_states.view(torch.int32), eager[t][1].view(torch.int32)), f"rnn step {t}"


@pytest.mark.parametrize("mode", MODES)
def test_one_iterative_dagger_iteration_trains_the_lstm_encoders(tmp_path, mode):
    import ivln_ce_amd  # noqa: F401
    from ivln_ce_amd import trainers  # noqa: F401
    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.registry import baseline_registry
    from latent_lstm_ref import mode_opts

    torch.manual_seed(0)
    np.random.seed(0)
    cfg = get_config(opts=[
        "TRAINER_NAME", "iterative_dagger", "NUM_ENVIRONMENTS", 2, "MODEL.policy_name", "LatentCMAPolicy",
        "MODEL.INSTRUCTION_ENCODER.use_pretrained_embeddings", False, "MODEL.DEPTH_ENCODER.ddppo_checkpoint", "NONE",
        "MODEL.STATE_ENCODER.rnn_type", "LSTM", "MODEL.STATE_ENCODER.latent_lstm", True, "RL.POLICY.OBS_TRANSFORMS.ENABLED_TRANSFORMS", [],
        "IL.DAGGER.iterations", 1, "IL.DAGGER.update_size", 4, "IL.DAGGER.p", 1.0, "IL.epochs", 1, "IL.batch_size", 2,
        "IL.DAGGER.lmdb_features_dir", str(tmp_path / "traj"), "CHECKPOINT_FOLDER", str(tmp_path / "ckpt"),
        "RESULTS_DIR", str(tmp_path / "res"), "EVAL_CKPT_PATH_DIR", str(tmp_path / "ckpt"),
        "TASK_CONFIG.ENVIRONMENT.ITERATIVE.ENABLED", True, *mode_opts(mode),
    ])
    tr = baseline_registry.get_trainer("iterative_dagger")(cfg)
    log = tr.train()
    assert len(log) >= 1 and all(np.isfinite(l["loss"]) for l in log), log
    net = tr.policy.net
    assert net.num_recurrent_layers == (5 if mode == "variant" else 4)
    # RNNStateEncoder's initialiser leaves the biases at exactly zero and the weights orthogonal (W^T W = I for the tall
    # (4H, K) matrices): after an update neither holds any more
    for name in ("state_encoder", "second_state_encoder"):
        rnn = getattr(net, name).rnn
        for w in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            cur = getattr(rnn, w).detach().cpu().double()
            assert bool(torch.isfinite(cur).all()), f"{name}.{w}"
            if "bias" in w:
                assert bool((cur != 0).any()), f"{name}.{w} did not move"
            else:
                off = float((cur.T @ cur - torch.eye(cur.shape[1], dtype=torch.float64)).abs().max())
                print(f"{mode:8s} {name}.{w}: |W^T W - I| {off:.3e}")
                assert off > 1e-5, f"{name}.{w} did not move"
