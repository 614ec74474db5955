"""CPU: the host side of RedNet's training augmentation and class weights (include/ivln_seg_augment.h,
ivln_ce_amd/rednet_train.py, tools/finetune_rednet.py) - the records, what the entry points refuse before any launch, the
median-frequency weights and the tool's flags.  The records live in host memory, so the refusals need no GPU."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_augment_ref as AR  # noqa: E402

QS = (4096, 4097, 5734, 8192, 2048, 3000)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_twin_indices_do_not_depend_on_the_float_type():
    g = np.random.default_rng(0)
    for (H, W), (h, w) in (((3, 5), (2, 3)), ((7, 64), (7, 64)), ((8, 8), (16, 16))):
        rgb = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        depth = g.random((H, W), dtype=np.float32)
        labels = g.integers(0, 13, (H, W), dtype=np.uint8)
        for q in QS:
            for side in (0, 1):
                for flip in (0, 1):
                    geom = (q, AR.offset_range(H, q)[side], AR.offset_range(W, q)[side], flip)
                    a = AR.augment_image(rgb, depth, labels, geom, (0.9, 1.1, -25.0, 0.0), 255, np.float32)
                    b = AR.augment_image(rgb, depth, labels, geom, (0.9, 1.1, -25.0, 0.0), 255, np.float64)
                    for k in ("labels_a", "depth_src", "inside", "ys", "xs"):
                        assert np.array_equal(a[k], b[k]), (H, W, geom, k)
                    assert a["rgb_n"].dtype == np.float32 and b["rgb_n"].dtype == np.float64
                    assert np.abs(a["rgb_n"] - b["rgb_n"]).max() < 1e-4
                    assert (a["labels_a"][~a["inside"]] == 255).all() and a["inside"].all() == (q >= 4096)


def test_sample_augment_is_reproducible_stays_in_range_and_has_an_identity():
    from ivln_ce_amd.rednet_train import AugmentConfig, offset_range, sample_augment, scaled_size

    cfg = AugmentConfig()
    a = sample_augment(cfg, 16, 48, 64, torch.Generator().manual_seed(5))
    b = sample_augment(cfg, 16, 48, 64, torch.Generator().manual_seed(5))
    c = sample_augment(cfg, 16, 48, 64, torch.Generator().manual_seed(6))
    assert a[0].dtype == torch.int32 and a[1].dtype == torch.float32 and a[0].shape == a[1].shape == (16, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    # the record of one seed, written down: any machine gives these integers
    first = sample_augment(cfg, 1, 48, 64, torch.Generator().manual_seed(5))[0][0].tolist()
    assert first == a[0][0].tolist()
    # every range, at every q of the kernel test (scale pinned to q / 4096) and for a wide draw
    for q in QS:
        s = q / 4096.0
        wide = AugmentConfig(scale=(s, s), flip=0.5, saturation=(0.0, 2.0), gain=(0.5, 1.5), offset=(-40.0, 40.0))
        geom, photo = sample_augment(wide, 64, 7, 64, torch.Generator().manual_seed(q))
        assert (geom[:, 0] == q).all()
        for n, col in ((7, 1), (64, 2)):
            lo, hi = offset_range(n, q)
            assert lo <= int(geom[:, col].min()) and int(geom[:, col].max()) <= hi, (q, n)
            assert (lo, hi) == AR.offset_range(n, q) and scaled_size(n, q) == AR.scaled_size(n, q)
            if hi - lo >= 1:
                assert len(set(geom[:, col].tolist())) > 1, "the offsets vary"
        assert set(geom[:, 3].tolist()) == {0, 1}
        assert 0.0 <= float(photo[:, 0].min()) and float(photo[:, 0].max()) <= 2.0
        assert 0.5 <= float(photo[:, 1].min()) and float(photo[:, 1].max()) <= 1.5
        assert -40.0 <= float(photo[:, 2].min()) and float(photo[:, 2].max()) <= 40.0 and (photo[:, 3] == 0).all()
    geom, photo = sample_augment(cfg, 256, 64, 64, torch.Generator().manual_seed(1))
    assert 4096 <= int(geom[:, 0].min()) and int(geom[:, 0].max()) <= round(1.4 * 4096) and len(set(geom[:, 0].tolist())) > 100
    # the degenerate config is exactly the identity record
    ident = AugmentConfig(scale=(1, 1), flip=0, saturation=(1, 1), gain=(1, 1), offset=(0, 0))
    geom, photo = sample_augment(ident, 5, 64, 48, torch.Generator().manual_seed(2))
    assert geom.tolist() == [[4096, 0, 0, 0]] * 5 and photo.tolist() == [[1.0, 1.0, 0.0, 0.0]] * 5


def test_a_config_that_pads_needs_an_ignore_label_when_the_trainer_is_built():
    from ivln_ce_amd.rednet_train import AugmentConfig

    with pytest.raises(ValueError):
        AugmentConfig(scale=(0.8, 1.2)).validate(None)
    AugmentConfig(scale=(0.8, 1.2)).validate(255)
    AugmentConfig().validate(None)
    for bad in (AugmentConfig(scale=(0.4, 1.0)), AugmentConfig(scale=(1.0, 2.5)), AugmentConfig(scale=(1.2, 1.0)),
                AugmentConfig(flip=1.5), AugmentConfig(gain=(-0.1, 1.0)), AugmentConfig(offset=(0.0, float("inf")))):
        with pytest.raises(ValueError):
            bad.validate(255)
    # RedNetTrainer.__init__ validates before it touches the model (the GPU tests build real ones)
    import inspect

    from ivln_ce_amd.rednet_train import RedNetTrainer

    sig = inspect.signature(RedNetTrainer.__init__)
    assert sig.parameters["augment"].default is None and sig.parameters["seed"].default == 0
    with pytest.raises(ValueError):
        RedNetTrainer(None, augment=AugmentConfig(scale=(0.8, 1.2)), ignore_label=None)


def test_median_frequency_weights_against_hand_computed_counts():
    from ivln_ce_amd.rednet_train import median_frequency_weights

    # three images of 100 labelled pixels each: class 0 in all three (60 + 50 + 90), class 1 in two (40 + 30), class 2 in
    # one image only (20), class 3 in one image only (10), class 4 never
    pixels = [200, 70, 20, 10, 0]
    present = [300, 200, 100, 100, 0]
    freq = [200 / 300, 70 / 200, 20 / 100, 10 / 100]  # an even number of present classes: the median is the middle pair's mean
    med = (0.35 + 0.2) / 2
    w = median_frequency_weights(torch.tensor(pixels), torch.tensor(present))
    assert w.dtype == torch.float32 and tuple(w.shape) == (5,)
    assert np.allclose(w.numpy(), np.float32([med / f for f in freq] + [1.0]), rtol=1e-7, atol=0)
    # an odd number: the median class gets exactly 1
    w = median_frequency_weights(np.array([50, 10, 40]), np.array([100, 100, 100]))
    assert np.allclose(w.numpy(), np.float32([0.4 / 0.5, 0.4 / 0.1, 1.0]), rtol=1e-7, atol=0) and float(w[2]) == 1.0
    # nothing seen at all: uniform
    assert median_frequency_weights([0, 0], [0, 0]).tolist() == [1.0, 1.0]
    with pytest.raises(ValueError):
        median_frequency_weights([1, 2], [0, 5])
    with pytest.raises(ValueError):
        median_frequency_weights([1, 2], [1, 2, 3])


def _lib():
    import __graft_entry__ as ge

    L = ctypes.CDLL(ge.build())
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.ivln_seg_augment_f32.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    L.ivln_seg_class_counts_u8.argtypes = [vp, i32, ctypes.c_int64, i32, i32, vp, vp, vp, vp]
    return L


def test_library_exports_what_the_augmentation_header_declares():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivln_seg_augment.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", src)))
    assert names == ["ivln_seg_augment_f32", "ivln_seg_class_counts_u8"]
    L = _lib()
    assert all(hasattr(L, n) for n in names)
    import importlib.util as iu

    spec = iu.spec_from_file_location("ivln_build", os.path.join(ROOT, "ivln-ce_amd", "build.py"))
    build = iu.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "seg_augment.hip" in build.SOURCES


def test_both_entry_points_refuse_null_operands_and_bad_records_before_any_launch():
    """Every call below returns IVLN_E_INVALID (-1), the code only the checks in front of the launch give (a failed launch
    is IVLN_E_HIP): the device pointers are made-up non-NULL addresses that nothing dereferences."""
    L = _lib()
    INVALID = -1
    H, W = 48, 64
    fake = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(6)]  # rgb, depth, labels, rgb_n, depth_n, labels_a

    def call(geom, photo, B=1, ign=255, ops=fake, h=H, w=W, Hh=H, Ww=W, g_null=False, p_null=False):
        g = (ctypes.c_int32 * (4 * max(B, 1)))(*(list(geom) * max(B, 1)))
        p = (ctypes.c_float * (4 * max(B, 1)))(*(list(photo) * max(B, 1)))
        return L.ivln_seg_augment_f32(ops[0], ops[1], ops[2], B, h, w, Hh, Ww, None if g_null else ctypes.addressof(g),
                                      None if p_null else ctypes.addressof(p), ign, ops[3], ops[4], ops[5], None)

    ident_g, ident_p = (4096, 0, 0, 0), (1.0, 1.0, 0.0, 0.0)
    for i in range(6):  # each NULL operand
        assert call(ident_g, ident_p, ops=[None if j == i else f for j, f in enumerate(fake)]) == INVALID, i
    assert call(ident_g, ident_p, g_null=True) == INVALID and call(ident_g, ident_p, p_null=True) == INVALID
    assert call(ident_g, ident_p, B=65) == INVALID and call(ident_g, ident_p, B=0) == INVALID
    assert call(ident_g, ident_p, h=0) == INVALID and call(ident_g, ident_p, Ww=0) == INVALID and call(ident_g, ident_p, Hh=40000) == INVALID
    assert call(ident_g, ident_p, ign=256) == INVALID and call(ident_g, ident_p, ign=-2) == INVALID
    bad_geom = {
        "q below 2048": (2047, 0, 0, 0), "q above 8192": (8193, 0, 0, 0), "flip 2": (4096, 0, 0, 2), "flip -1": (4096, 0, 0, -1),
        "oy at q = 4096": (4096, 1, 0, 0), "ox at q = 4096": (4096, 0, -1, 0),
        "oy past the crop": (5734, AR.scaled_size(H, 5734) - H + 1, 0, 0), "oy negative in a crop": (5734, -1, 0, 0),
        "ox past the crop": (8192, 0, W + 1, 0), "oy positive in a pad": (2048, 1, 0, 0),
        "ox past the pad": (3000, 0, AR.scaled_size(W, 3000) - W - 1, 0),
    }
    for name, g in bad_geom.items():
        assert call(g, ident_p) == INVALID, name
    nan, inf = float("nan"), float("inf")
    for p in ((nan, 1, 0, 0), (1, inf, 0, 0), (1, 1, -inf, 0), (1, 1, 0, nan), (-0.5, 1, 0, 0), (1, -1e-3, 0, 0)):
        assert call(ident_g, p) == INVALID, p
    # a record that pads while there is no ignore label - in either axis alone too
    assert call((2048, 0, 0, 0), ident_p, ign=-1) == INVALID and call((4000, 0, 0, 0), ident_p, ign=-1) == INVALID
    assert AR.scaled_size(3, 3500) == 3 and AR.scaled_size(64, 3500) < 64
    assert call((3500, 0, 0, 0), ident_p, ign=-1, Hh=3, h=3) == INVALID
    # a bad record behind good ones is found as well
    g = (ctypes.c_int32 * 12)(4096, 0, 0, 0, 5734, 3, 4, 1, 4096, 0, 0, 7)
    p = (ctypes.c_float * 12)(*([1.0, 1.0, 0.0, 0.0] * 3))
    assert L.ivln_seg_augment_f32(fake[0], fake[1], fake[2], 3, H, W, H, W, ctypes.addressof(g), ctypes.addressof(p), 255, fake[3],
                                  fake[4], fake[5], None) == INVALID

    ok = ctypes.c_void_p(0x1000)
    for args in ((None, 2, 64, 13, -1, ok, ok, ok), (ok, 2, 64, 13, -1, None, ok, ok), (ok, 2, 64, 13, -1, ok, None, ok),
                 (ok, 2, 64, 13, -1, ok, ok, None), (ok, 0, 64, 13, -1, ok, ok, ok), (ok, 2, 0, 13, -1, ok, ok, ok),
                 (ok, 2, 64, 65, -1, ok, ok, ok), (ok, 2, 64, 0, -1, ok, ok, ok), (ok, 2, 64, 13, 256, ok, ok, ok)):
        assert L.ivln_seg_class_counts_u8(*args, None) == INVALID, args


def test_the_finetune_tool_parses_its_new_flags_and_keeps_its_defaults():
    tool = _tool("finetune_rednet")
    base = ["--exp-config", "x.yaml", "--steps", "7", "--out", "o.pkl"]
    a = tool.parse_args(base)
    assert (a.augment, a.seed, a.class_weights, a.holdout, a.eval_every) == (False, 0, "none", 0, 0)
    assert (a.exp_config, a.steps, a.out, a.init, a.trainable, a.lr, a.ignore_label) == ("x.yaml", 7, "o.pkl", None, "all", 2e-4, None)
    a = tool.parse_args(base + ["--augment", "--seed", "9", "--class-weights", "median", "--weight-batches", "3", "--holdout", "4",
                                "--eval-every", "50", "TORCH_GPU_ID", "0"])
    assert (a.augment, a.seed, a.class_weights, a.weight_batches, a.holdout, a.eval_every) == (True, 9, "median", 3, 4, 50)
    assert a.opts == ["TORCH_GPU_ID", "0"]
    for bad in (["--class-weights", "inverse"], ["--holdout", "-1"], ["--weight-batches", "0"], ["--eval-every", "-5"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
