"""GPU: rednet_train.RedNetTrainer - one update against the float64 twin's loss, overfitting one structured batch, and the
way back into the rollout (save -> fresh RedNet -> PredictSemantics).  Bars: the loss 2e-5 (the update tests' loss bar,
tests/test_gpu_train.py), one Adam step moves every element by at most lr * 1.001 + 1e-9 (same file); the frozen forward
against forward_train in eval mode twice the forward bar of tests/test_gpu_rednet_train.py."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "golden"))
import rednet_twin as RW  # noqa: E402

DEV = torch.device("cuda:0")


def _write(name, lines):
    from kernel_bar import _log_dir

    os.makedirs(_log_dir(), exist_ok=True)
    open(os.path.join(_log_dir(), name), "w").write("\n".join(lines) + "\n")


def _state():
    from det_init import det_fill

    return {k: v.clone() for k, v in det_fill(RW.RedNetTwin(), seed=1, conv_gain=0.6).state_dict().items()}


def _model(state):
    from ivln_ce_amd.rednet import RedNet

    m = RedNet({"n_classes": 13})
    m.load_state_dict(state)
    return m.to(DEV).train()


def _dev(obs):
    return {k: v.to(DEV) for k, v in obs.items()}


@pytest.mark.parametrize("trainable", ["all", "decoder"])
def test_one_step_gives_the_twins_loss_and_moves_every_trainable_element_by_at_most_lr(trainable):
    from ivln_ce_amd import ops
    from ivln_ce_amd.rednet_train import RedNetTrainer

    torch.set_num_threads(min(8, torch.get_num_threads()))
    state = _state()
    obs = RW.structured_batch(B=2, seed=4)
    obs["semantic12"][0, :9, :13] = 255  # (an ignored patch)
    wt = torch.linspace(0.5, 1.5, 13)
    sw = (1.0, 0.5, 0.25, 0.25, 0.125)
    lr = 2e-4
    model = _model(state)
    tr = RedNetTrainer(model, lr=lr, trainable=trainable, class_weights=wt, ignore_label=255, scale_weights=sw)
    names = {k for k, _ in model.trainable_parameters(trainable)}
    assert set(tr.opt.names) == names and len(names) == (469 if trainable == "all" else 151)
    epoch = ops.WEIGHT_EPOCH
    loss = tr.step(_dev(obs))
    torch.cuda.synchronize()
    assert isinstance(loss, float) and len(tr.last_per_scale) == 5 and ops.WEIGHT_EPOCH > epoch
    # the twin: float64, train-mode BatchNorm (decoder: the encoders' BatchNorms on their running statistics - the frozen forward)
    twin = RW.build(state, torch.float64, True)
    if trainable == "decoder":
        for k, m in twin.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d) and k.startswith(("bn1", "layer")):
                m.eval()
    rgb, dep = RW.normalise(obs, torch.float64)
    with torch.no_grad():
        ref, per = RW.five_scale_loss(twin.forward_train(rgb, dep), obs["semantic12"], wt.double(), 255, sw)
    _write(f"rednet_trainer_step_{trainable}.log", [f"loss hip {loss:.7f} twin {float(ref):.7f}",
                                                     f"per scale hip {tr.last_per_scale} twin {[float(p) for p in per]}"])
    assert abs(loss - float(ref)) < 2e-5, (loss, float(ref))
    moved = 0
    for k, v in model.state_dict().items():
        d = float((v.detach().cpu().double() - state[k].double()).abs().max())
        if k in names:
            assert d <= lr * 1.001 + 1e-9, (k, d)
            moved += d > 0
        elif trainable == "decoder" and k.startswith(("conv1", "bn1", "layer")):
            assert d == 0.0, f"{k}: a frozen encoder tensor moved"
    assert moved > 0.9 * len(names), (moved, len(names))


def test_overfits_one_structured_batch_and_the_rollout_sees_the_new_weights(tmp_path):
    """64 x 64, B = 4, label = the depth in 4 bands, 20 steps: the last loss is below the first and mIoU on that batch rises.
    The fp32 twin with torch.optim.Adam learns from exactly this batch too (tests/golden/rednet_overfit_cpu.json, recorded on
    the CPU by tests/golden/gen_rednet_overfit_curve.py); both curves go to the log, no closeness between them is asserted.
    Then save -> a fresh RedNet -> PredictSemantics: the trainer's own predictions, and the frozen forward equals
    forward_train with every BatchNorm in eval mode - the folded cache was voided after the updates."""
    from ivln_ce_amd.rednet import PredictSemantics, RedNet
    from ivln_ce_amd.rednet_train import RedNetTrainer

    torch.set_num_threads(min(8, torch.get_num_threads()))
    cpu = json.load(open(os.path.join(HERE, "golden", "rednet_overfit_cpu.json")))
    assert cpu["losses"][-1] < cpu["losses"][0] and cpu["miou_after"] > cpu["miou_before"] and cpu["steps"] == 20
    obs = RW.structured_batch()
    dobs = _dev(obs)
    model = _model(_state())
    tr = RedNetTrainer(model, lr=cpu["lr"])
    with torch.no_grad():  # (fills the folded cache and the plan with the OLD weights)
        before = tr.evaluate([dobs])
    losses = [tr.step(dobs) for _ in range(cpu["steps"])]
    after = tr.evaluate([dobs])
    _write("rednet_trainer_overfit.log", [f"hip  losses {losses}", f"hip  mIoU {before['miou']:.4f} -> {after['miou']:.4f}, "
                                          f"pixel accuracy {before['pixel_acc']:.4f} -> {after['pixel_acc']:.4f}",
                                          f"cpu  losses {cpu['losses']}", f"cpu  mIoU {cpu['miou_before']:.4f} -> {cpu['miou_after']:.4f}"])
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    assert after["miou"] > before["miou"], (before["miou"], after["miou"])
    assert int(after["counts"].sum()) == obs["semantic12"].numel()

    path = os.path.join(tmp_path, "rednet_finetuned.pkl")
    tr.save(path)
    ckpt = torch.load(path, map_location="cpu")
    assert sorted(ckpt) == ["model_state"]
    fresh = RedNet({"n_classes": 13})
    fresh.load_state_dict(ckpt["model_state"])  # strict
    fresh = fresh.to(DEV).eval()
    ps = PredictSemantics(DEV, model=fresh)
    labels = ps(dobs)
    mine = tr.predict(dobs)
    assert labels.dtype == torch.uint8 and torch.equal(labels, mine), "the saved weights give the trainer's own predictions"
    assert RW.miou(labels.cpu(), obs["semantic12"]) == pytest.approx(after["miou"])
    # frozen forward == forward_train with every BatchNorm in eval mode
    two = {k: v[:2] for k, v in obs.items()}
    frozen = ps.scores(_dev(two)).clone()
    model.eval()
    rgb, dn = tr.inputs(_dev(two))
    with torch.no_grad():
        out = model.forward_train(rgb, dn, {})[0].clone()
    n32, n64 = RW.normalise(two, torch.float32), RW.normalise(two, torch.float64)
    with torch.no_grad():
        r32 = RW.build(ckpt["model_state"], torch.float32, False)(*n32)
        r64 = RW.build(ckpt["model_state"], torch.float64, False)(*n64)
    e32, mx = float((r32.double() - r64).abs().max()), float(r64.abs().max())
    bar = 4 * e32 + 2e-5 * mx
    e_pair, e_train, e_frozen = float((frozen - out).abs().max()), float((out.cpu().double() - r64).abs().max()), float((frozen.cpu().double() - r64).abs().max())
    _write("rednet_trainer_frozen_vs_train.log", [f"frozen vs forward_train(eval) {e_pair:.3e}; vs the float64 twin: forward_train "
                                                  f"{e_train:.3e}, frozen {e_frozen:.3e}; torch fp32 {e32:.3e}, max|ref| {mx:.3e}, bar {bar:.3e}"])
    assert e_pair <= 2 * bar, (e_pair, bar)
