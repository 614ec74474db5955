"""Golden vectors for the Latent-CMA policy with LSTM state encoders (`MODEL.STATE_ENCODER.rnn_type: LSTM`): the
REFERENCE's own `LatentCMANet` (ivlnce_baselines/models/latent_cma_policy.py:195-497) on the CPU, its
`build_distribution` + the loss of `IterativeDaggerTrainer._update_agent` + autograd, as in gen_latent_update_golden.py.
habitat-lab's `build_rnn_state_encoder` is not part of the shim, so - in this generator only - the name the reference
imports is replaced with one that returns an LSTM RNNStateEncoder (tests/lstm_state_ref.LSTMStateEncoderRef: nn.LSTM,
state (N, 2, H) = [h | c], both masked before every step).
  plain - episodic memory, progress monitor on, h0 = 0, an episode boundary inside the batch
  tour  - `tour_memory`: both LSTMs reset with the TOUR mask, carried state
Third, the evidence for what DESIGN.md ("Latent-CMA with LSTM state encoders") says about the tour-memory variant: the reference is
built with `tour_memory_variant` + `memory_at_end` and LSTM encoders, its forward is run, and the exception it raises -
torch.max of the (N, 1, H) memory slot with the (N, 2, H) [h | c] slice assigned into the (N, 1, H) slot,
latent_cma_policy.py:434-439 - is stored as text in latent_lstm_tour.npz (`variant_raises`, `variant_error`).
Only small tensors are stored (logits, states, loss, gradient norms, a few small gradients); the feature tensors are
regenerated in the tests from seeds (gen_latent_update_features.py).
Build container only:  python tests/golden/gen_latent_lstm_golden.py -> tests/golden/latent_lstm_{plain,tour}.npz
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: lstm_state_ref
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root: oracle (imported by lstm_state_ref)
import _ref_shim  # noqa: E402

_ref_shim.install()
torch.set_num_threads(8)
from det_init import det_fill  # noqa: E402
from gen_latent_update_features import features  # noqa: E402
from lstm_state_ref import LSTMStateEncoderRef  # noqa: E402

import ivlnce_baselines.models.latent_cma_policy as ref_latent  # noqa: E402
from ivlnce_baselines.common.aux_losses import AuxLosses  # noqa: E402


def _build_lstm(input_size, hidden_size, rnn_type="GRU", num_layers=1):
    assert str(rnn_type) == "LSTM" and num_layers == 1, (rnn_type, num_layers)  # the config key reaches the builder
    return LSTMStateEncoderRef(input_size, hidden_size)


ref_latent.build_rnn_state_encoder = _build_lstm
T, N = 3, 2


def make_policy(mode):
    cfg = _ref_shim.default_model_config()
    cfg.MODEL.policy_name = "LatentCMAPolicy"
    cfg.MODEL.STATE_ENCODER.rnn_type = "LSTM"
    cfg.MODEL.tour_memory = mode == "tour"
    cfg.MODEL.tour_memory_variant = mode == "variant"
    cfg.MODEL.memory_at_end = mode == "variant"
    cfg.MODEL.PROGRESS_MONITOR.use = mode == "plain"
    sp = sys.modules["gym.spaces"]
    space = sp.Dict({"depth": sp.Box(0.0, 1.0, (256, 256, 1), np.float32), "rgb": sp.Box(0, 255, (224, 224, 3), np.uint8),
                     "instruction": sp.Box(0, 2504, (200,), np.int64)})
    pol = ref_latent.LatentCMAPolicy.from_config(cfg, space, sp.Discrete(4))
    det_fill(pol, seed=0, conv_gain=1.0)
    return pol.double().train()  # float64: the goldens are the reference's arithmetic, not its rounding


def inputs(mode, seed, L):
    g = torch.Generator().manual_seed(seed)
    TN = T * N
    rgb_np, dep_np = features(seed, T, N)
    instr1 = torch.zeros(N, 200, dtype=torch.long)
    for b, n in enumerate([57, 9]):
        instr1[b, :n] = torch.randint(2, 2504, (n,), generator=g)
    instr = instr1.unsqueeze(0).expand(T, N, 200).reshape(TN, 200).float()  # batch_to casts observations to f32
    progress = torch.rand(TN, 1, generator=g)
    prev = torch.randint(0, 4, (TN, 1), generator=g)
    tgt = torch.randint(0, 4, (T, N), generator=g)
    w = torch.where(torch.rand(T, N, generator=g) < 0.3, torch.tensor(3.2), torch.tensor(1.0))
    w[2:, 0] = 0.0  # a padded (shorter) trajectory
    ep = torch.ones(T, N, dtype=torch.uint8)
    ep[0] = 0     # every batch row starts an episode (tour_dataset.py:90-93)
    ep[2, 1] = 0  # ... and row 1 starts its next episode INSIDE its tour
    tour = torch.ones(T, N, dtype=torch.uint8)
    tour[0, 0] = 0  # only trajectory 0 starts a new tour; the other continues its own (tour_dataset.py:280-281)
    h0 = torch.zeros(N, L, 512) if mode == "plain" else 0.3 * torch.randn(N, L, 512, generator=g)
    if mode == "variant":
        h0[:, : L - 1] = 0  # iterative_dagger_trainer.py:58-60: episodic slots cleared, tour slot kept
    obs = {"rgb_features": torch.from_numpy(rgb_np).double(), "depth_features": torch.from_numpy(dep_np).double(),
           "instruction": instr, "progress": progress.double()}
    return obs, h0.double(), prev, tgt, w.double(), ep.view(-1, 1), tour.view(-1, 1)


def gen(mode, seed, extra=None):
    pol = make_policy(mode)
    L = pol.net.num_recurrent_layers
    assert L == 4, L
    obs, h0, prev, tgt, w, ep, tour = inputs(mode, seed, L)
    AuxLosses.clear()
    if mode == "plain":
        AuxLosses.activate()
    else:
        AuxLosses.deactivate()
    dist, rnn_out = pol.build_distribution(obs, h0.clone().detach(), prev, ep, tour)
    logits = dist.logits.view(T, N, -1)
    ce = F.cross_entropy(logits.permute(0, 2, 1), tgt, reduction="none")
    action_loss = ((w * ce).sum(0) / w.sum(0)).mean()
    aux = AuxLosses.reduce((w > 0).view(-1)) if mode == "plain" else 0.0
    loss = action_loss + aux
    loss.backward()
    AuxLosses.deactivate()
    d = dict(T=T, N=N, seed=seed, instruction=obs["instruction"].numpy(), progress=obs["progress"].numpy(), prev=prev.numpy(),
             targets=tgt.numpy(), weights=w.numpy(), ep=ep.numpy(), tour=tour.numpy(), h0=h0.numpy(),
             logits=logits.detach().numpy(), rnn_out=rnn_out.detach().numpy(), loss=float(loss),
             action_loss=float(action_loss), aux_loss=float(aux), state_dict_keys=np.array(sorted(pol.state_dict().keys())))
    named = dict(pol.named_parameters())
    n_grad = 0
    for k, p in named.items():
        if p.grad is not None:
            d["gradnorm/" + k] = float(p.grad.norm())
            n_grad += 1
    full = ["action_distribution.linear.weight", "net.rgb_kv.bias", "net.rgb_linear.2.bias", "net.text_q.bias",
            "net.prev_action_embedding.weight", "net.state_encoder.rnn.bias_hh_l0",
            "net.second_state_encoder.rnn.bias_ih_l0", "net.instruction_encoder.encoder_rnn.bias_ih_l0_reverse",
            "net.rgb_encoder.spatial_embeddings.weight", "net.depth_encoder.spatial_embeddings.weight"]
    if mode == "plain":
        full.append("net.progress_monitor.weight")
    for k in full:
        d["grad/" + k] = named[k].grad.numpy()
    d.update(extra or {})
    name = f"latent_lstm_{mode}.npz"
    np.savez_compressed(os.path.join(HERE, name), **d)
    print(name, "loss", float(loss), float(action_loss), float(aux), "params with grad", n_grad,
          os.path.getsize(os.path.join(HERE, name)) // 1024, "KiB")


def variant_evidence(seed):
    """The reference with LSTM encoders and `tour_memory_variant`: built, run, and what it raises."""
    pol = make_policy("variant")
    L = pol.net.num_recurrent_layers
    w_ih = tuple(pol.net.state_encoder.rnn.weight_ih_l0.shape)
    obs, h0, prev, _, _, ep, tour = inputs("variant", seed, L)
    AuxLosses.deactivate()
    try:
        pol.build_distribution(obs, h0.clone().detach(), prev, ep, tour)
        raised, kind, text = False, "", ""
    except Exception as e:  # noqa: BLE001  (whatever it is, it is the record)
        raised, kind, text = True, type(e).__name__, str(e)
    print("variant: num_recurrent_layers", L, "weight_ih_l0", w_ih, "raises", raised, kind, text)
    return dict(variant_raises=raised, variant_error_type=kind, variant_error=text, variant_num_recurrent_layers=L,
                variant_weight_ih_shape=np.array(w_ih))


if __name__ == "__main__":
    gen("plain", 201)
    gen("tour", 202, extra=variant_evidence(203))
