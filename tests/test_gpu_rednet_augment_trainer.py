"""GPU: rednet_train.RedNetTrainer with augmentation - the deterministic state and structured_batch(B = 2) of
tests/test_gpu_rednet_trainer.py.  Identity records must be today's path bit for bit at the network's input; explicit records
give the float64 twin's loss (RedNetTwin on tests/seg_augment_ref.py's outputs) within that file's 2e-5 loss bar; sampled
records train reproducibly under a seed; evaluate never augments.  Figures go to rednet_augment_trainer.log first."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import rednet_twin as RW  # noqa: E402
import seg_augment_ref as AR  # noqa: E402
from kernel_bar import _log, _same_bytes  # noqa: E402

DEV = torch.device("cuda:0")
LOG = "rednet_augment_trainer.log"
IDENT = (torch.tensor([[4096, 0, 0, 0]] * 2, dtype=torch.int32), torch.tensor([[1.0, 1.0, 0.0, 0.0]] * 2))


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


def _grads(tr, G):
    return {k: G[p].detach().clone() for k, p in zip(tr.opt.names, tr.opt.params)}


def _apart(a, b):
    """(loss, per-scale, gradients) twice -> the largest absolute difference of each"""
    return (float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()),
            max(float((a[2][k] - b[2][k]).abs().max()) for k in a[2]))


def test_identity_records_are_the_unaugmented_path():
    from ivln_ce_amd.rednet_train import RedNetTrainer

    state = _state()
    obs = _dev(RW.structured_batch(B=2, seed=4))
    runs = []
    for records in (None, None, IDENT):
        tr = RedNetTrainer(_model(state), ignore_label=255)
        seen = {}
        inner = tr.model.forward_train

        def spy(rgb, dn, *a, _inner=inner, _seen=seen, **kw):
            _seen["rgb"], _seen["dn"] = rgb.clone(), dn.clone()
            return _inner(rgb, dn, *a, **kw)

        tr.model.forward_train = spy
        loss, per, G = tr.loss_and_gradients(obs, records)
        torch.cuda.synchronize()
        runs.append((loss.clone().cpu(), per.clone().cpu(), _grads(tr, G), seen))
        if records is not None:
            rgb, dn = RedNetTrainer.inputs(obs)
            assert _same_bytes(seen["rgb"], rgb) and _same_bytes(seen["dn"], dn), "forward_train saw other bytes than inputs()"
    assert _same_bytes(runs[0][3]["rgb"], runs[2][3]["rgb"]) and _same_bytes(runs[0][3]["dn"], runs[2][3]["dn"])
    base, mine = _apart(runs[0], runs[1]), _apart(runs[0], runs[2])
    _log(f"two un-augmented runs apart: loss {base[0]:.3e} per-scale {base[1]:.3e} gradients {base[2]:.3e}", LOG)
    _log(f"identity records vs un-augmented: loss {mine[0]:.3e} per-scale {mine[1]:.3e} gradients {mine[2]:.3e}", LOG)
    assert all(m <= b for m, b in zip(mine, base)), (mine, base)


def test_explicit_records_give_the_float64_twins_loss():
    from ivln_ce_amd.rednet_train import RedNetTrainer

    torch.set_num_threads(min(8, torch.get_num_threads()))
    state = _state()
    obs = RW.structured_batch(B=2, seed=4)
    H = W = 64
    q = 5734
    geom = [(q, AR.offset_range(H, q)[1], 3, 1), (q, 5, AR.offset_range(W, q)[1], 1)]
    photo = [(0.9, 1.1, -25.0, 0.0), (1.1, 0.95, 10.0, 0.0)]
    tr = RedNetTrainer(_model(state), ignore_label=255)
    loss, per, _ = tr.loss_and_gradients(_dev(obs), (torch.tensor(geom, dtype=torch.int32), torch.tensor(photo, dtype=torch.float32)))
    aug = AR.augment_batch(obs["rgb"].numpy(), obs["depth"][..., 0].numpy(), obs["semantic12"][..., 0].numpy(), geom, photo, 255,
                           np.float64)
    assert aug["inside"].all()
    twin = RW.build(state, torch.float64, True)
    with torch.no_grad():
        ref, ref_per = RW.five_scale_loss(twin.forward_train(torch.from_numpy(aug["rgb_n"]), torch.from_numpy(aug["depth_n"]).unsqueeze(1)),
                                          torch.from_numpy(aug["labels_a"]), None, 255)
        plain, _ = RW.five_scale_loss(twin.forward_train(*RW.normalise(obs, torch.float64)), obs["semantic12"], None, 255)
    _log(f"q {q} + flip: loss hip {float(loss):.7f} twin {float(ref):.7f} (un-augmented twin {float(plain):.7f}); per scale hip "
         f"{[float(x) for x in per.cpu()]} twin {[float(p) for p in ref_per]}", LOG)
    assert abs(float(plain) - float(ref)) > 1e-3, "the records change the loss: the comparison below is not the un-augmented one"
    assert abs(float(loss) - float(ref)) < 2e-5, (float(loss), float(ref))


def test_sampled_records_train_reproducibly_and_evaluate_never_augments():
    from ivln_ce_amd.rednet_train import AugmentConfig, RedNetTrainer

    state = _state()
    obs = _dev(RW.structured_batch(B=2, seed=4))
    finals, curves = [], []
    for _ in range(2):
        tr = RedNetTrainer(_model(state), augment=AugmentConfig(), seed=3)
        curves.append([tr.step(obs) for _ in range(3)])
        finals.append({k: v.detach().clone() for k, v in tr.model.state_dict().items()})
    _log(f"three augmented steps, seed 3: {curves[0]} and again {curves[1]}", LOG)
    assert all(np.isfinite(curves[0])) and curves[0] == curves[1]
    assert all(torch.equal(finals[0][k], finals[1][k]) for k in finals[0]), "the same seed gives the same weights"
    names = set(tr.opt.names)
    moved = sum(float((finals[0][k].cpu().double() - state[k].double()).abs().max()) > 0 for k in names)
    assert moved > 0.9 * len(names), (moved, len(names))
    other = RedNetTrainer(_model(state), augment=AugmentConfig(), seed=4)
    assert [other.step(obs) for _ in range(3)] != curves[0], "another seed draws other records"
    # evaluate: the frozen forward on the raw frames - a never-augmenting trainer with the same weights gives the same counts
    mine = tr.evaluate([obs])
    plain = RedNetTrainer(_model({k: v.cpu() for k, v in finals[1].items()})).evaluate([obs])
    _log(f"evaluate after augmented training: mIoU {mine['miou']:.6f}, never-augmenting trainer {plain['miou']:.6f}", LOG)
    assert np.array_equal(mine["counts"], plain["counts"]) and mine["miou"] == plain["miou"] and mine["pixel_acc"] == plain["pixel_acc"]
    assert torch.equal(tr.predict(obs), RedNetTrainer(_model({k: v.cpu() for k, v in finals[1].items()})).predict(obs))
