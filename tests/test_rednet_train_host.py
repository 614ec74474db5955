"""CPU: the host side of RedNet fine-tuning (ivln_ce_amd/rednet_train.py, tools/finetune_rednet.py) - what is decided
before any kernel runs."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_seg_loss_refuses_outputs_whose_sizes_are_not_the_labels_divided_by_an_integer():
    from ivln_ce_amd.rednet_train import seg_loss

    labels = torch.zeros(2, 64, 64, 1, dtype=torch.uint8)
    good = [torch.zeros(2, 13, 64 >> i, 64 >> i) for i in range(5)]
    for bad in ([torch.zeros(2, 13, 48, 48)], [torch.zeros(2, 13, 32, 16)], [torch.zeros(2, 13, 128, 128)], [torch.zeros(3, 13, 64, 64)],
                good[:4] + [torch.zeros(2, 13, 5, 5)]):
        with pytest.raises(ValueError):
            seg_loss(bad, labels, scale_weights=(1,) * len(bad))
    with pytest.raises(ValueError):
        seg_loss(good, labels, scale_weights=(1, 1, 1))
    with pytest.raises(ValueError):
        seg_loss(good, labels.float())
    with pytest.raises(ValueError):
        seg_loss(good, torch.zeros(2, 64, 64, 3, dtype=torch.uint8))


def test_trainable_sets_and_the_moved_helpers_keep_their_names():
    from ivln_ce_amd import latent_policy, rednet

    assert latent_policy._conv_bn_train is rednet._conv_bn_train and latent_policy._bottleneck_train is rednet._bottleneck_train
    m = rednet.RedNet({"n_classes": 13})
    every, dec = m.trainable_parameters("all"), m.trainable_parameters("decoder")
    assert len(every) == len(list(m.parameters())) == 469 and len(dec) == 151
    assert not any(k.startswith(("conv1", "bn1", "layer")) for k, _ in dec)
    with pytest.raises(ValueError):
        m.trainable_parameters("encoder")
    with pytest.raises(AssertionError):
        m.train()(torch.zeros(1, 3, 32, 32), torch.zeros(1, 1, 32, 32))  # `forward` stays the inference path


def test_checkpoint_has_the_key_the_loaders_read(tmp_path):
    from ivln_ce_amd.rednet import RedNet
    from ivln_ce_amd.rednet_train import checkpoint_dict

    m = RedNet({"n_classes": 13})
    ckpt = checkpoint_dict(m)
    assert list(ckpt) == ["model_state"] and all(v.device.type == "cpu" for v in ckpt["model_state"].values())
    path = os.path.join(tmp_path, "m.pkl")
    torch.save(ckpt, path)
    state = torch.load(path, map_location="cpu")["model_state"]  # (PredictSemantics.setup; the reference's load_model)
    assert next(iter(state)).split(".")[0] != "module"
    RedNet({"n_classes": 13}).load_state_dict(state)  # strict
    from oracle.rednet_ref import RedNetRef

    RedNetRef().load_state_dict(state)  # the reference's module names


def test_library_exports_what_the_segmentation_header_declares():
    import ctypes
    import re

    import __graft_entry__ as ge

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivln_seg_train.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", src)))
    assert names == ["ivln_seg_ce_f32", "ivln_seg_confusion_u8"]
    L = ctypes.CDLL(ge.build())
    assert all(hasattr(L, n) for n in names)
    # a NULL operand or a class count out of range is refused before anything is launched (no GPU needed to ask)
    assert L.ivln_seg_ce_f32(None, None, None, 1, 13, 1, 1, 1, -1, ctypes.c_double(1.0), None, None, None, 0, None, None) != 0
    assert L.ivln_seg_confusion_u8(None, None, ctypes.c_int64(1), 13, -1, None, None, None) != 0


def test_metrics_from_counts():
    from ivln_ce_amd.rednet_train import metrics_from_counts

    c = np.zeros((4, 4), dtype=np.int64)
    c[0, 0], c[0, 1], c[1, 1], c[2, 0] = 6, 2, 5, 3  # class 3 neither occurs nor is predicted
    m = metrics_from_counts(c)
    assert m["pixel_acc"] == pytest.approx(11 / 16)
    assert np.allclose(m["iou"][:3], [6 / 11, 5 / 7, 0.0]) and np.isnan(m["iou"][3])
    assert m["miou"] == pytest.approx((6 / 11 + 5 / 7 + 0.0) / 3)
    assert np.array_equal(m["counts"], c)


def test_the_finetune_tool_parses_its_arguments():
    tool = _tool("finetune_rednet")
    a = tool.parse_args(["--exp-config", "x.yaml", "--steps", "7", "--out", "o.pkl"])
    assert (a.exp_config, a.steps, a.out, a.init, a.trainable) == ("x.yaml", 7, "o.pkl", None, "all")
    a = tool.parse_args(["--exp-config", "x.yaml", "--steps", "3", "--out", "o.pkl", "--init", "i.pkl", "--trainable", "decoder"])
    assert (a.init, a.trainable) == ("i.pkl", "decoder")
    for bad in (["--steps", "3", "--out", "o"], ["--exp-config", "x", "--steps", "3", "--out", "o", "--trainable", "encoder"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
