"""CPU: the reference the trainable RGB encoder's gradients are compared with (tests/rgb_twin.py) - the mask-frozen float64
twin of the train-mode BatchNorm ResNet-50 agrees with torch's own fp32 autograd, free float64 autograd does not (ReLU and
max-pool kinks flip between the precisions).  That is why the GPU tests use the twin.  The per-tensor error of fp32
autograd against the twin goes to rgb_twin_cpu.log in the suite's log directory: the GPU tests' allowance rests on it."""
import ctypes
import os
import re

import torch

import rgb_twin as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frozen_twin_matches_fp32_autograd_and_free_float64_does_not():
    from kernel_bar import _log_dir

    torch.set_num_threads(min(8, torch.get_num_threads()))
    g = torch.Generator().manual_seed(11)
    x = RT.to_input(torch.randint(0, 256, (3, 64, 64, 3), generator=g, dtype=torch.uint8))
    d_feats = torch.randn(3, 2048, 4, 4, generator=g)
    state = RT.oracle_cnn().state_dict()
    r = RT.fp32_autograd_error(state, x, d_feats)
    e32, fp32, twin, feats, feats64, masks = r["e32"], r["fp32"], r["twin"], r["feats32"], r["feats64"], r["masks"]
    assert len(fp32) == len(list(RT.oracle_cnn().parameters())) == 159 and len(masks) == 49
    # the twin's forward is the fp32 pass's function: same features up to rounding (amplified by layer 4's BatchNorms over
    # 12 values; a wrong mask or pool index would be a difference of the features' own size)
    e_fwd = float((feats64 - feats.double()).abs().max())
    print(f"fp32 forward vs the twin's: {e_fwd:.2e} of max|features| {float(feats64.abs().max()):.2e}")
    assert e_fwd < 1e-2 * float(feats64.abs().max())

    free = RT.oracle_cnn(state).double()
    RT.features(free, x.double()).backward(d_feats.double())
    free = {k: p.grad.detach() for k, p in free.named_parameters()}
    scale = {k: float(twin[k].abs().max()) for k in twin}
    rel_twin = {k: e32[k] / scale[k] for k in twin}
    rel_free = {k: float((fp32[k].double() - free[k]).abs().max()) / scale[k] for k in twin}
    os.makedirs(_log_dir(), exist_ok=True)
    with open(os.path.join(_log_dir(), "rgb_twin_cpu.log"), "w") as f:
        for k in twin:
            f.write(f"{k}: max|twin| {scale[k]:.3e} fp32 autograd vs twin {e32[k]:.3e} (rel {rel_twin[k]:.2e}) "
                    f"vs free float64 {rel_free[k] * scale[k]:.3e} (rel {rel_free[k]:.2e})\n")
    med = lambda d: sorted(d.values())[len(d) // 2]  # noqa: E731
    print(f"fp32 autograd vs frozen twin: worst {max(rel_twin.values()):.2e} median {med(rel_twin):.2e}; vs free float64: "
          f"worst {max(rel_free.values()):.2e} median {med(rel_free):.2e}, "
          f"{sum(v > 1e-3 for v in rel_free.values())} of {len(free)} tensors over 1e-3")
    # fp32 rounding through 53 BatchNorms (the deepest over 12 values) against a kink-induced, finite difference
    assert max(rel_twin.values()) < 1e-3, max(rel_twin.values())
    assert med(rel_free) > 10 * max(rel_twin.values()) and med(rel_free) > 1e-3, (med(rel_free), max(rel_twin.values()))


def test_library_exports_every_entry_of_the_rgb_backward_header():
    """include/ivln_rgb_bwd.h (the code of include/ivln_hip.h and include/ivln_depth_bwd.h is pinned: later entry points get
    a header of their own) declares the three entry points, the library exports them, ops.py binds each, and NULL or
    non-positive arguments are refused before anything is launched."""
    import __graft_entry__ as ge

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivln_rgb_bwd.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", src)))
    assert names == ["ivln_adaptive_avgpool2d_bwd_f32", "ivln_bn_apply_f32", "ivln_bn_bwd_f32"]
    L = ctypes.CDLL(ge.build())
    assert all(hasattr(L, n) for n in names)
    ops_src = open(os.path.join(ROOT, "ivln-ce_amd", "ops.py")).read()
    assert all(f"L.{n}(" in ops_src for n in names)
    build_src = open(os.path.join(ROOT, "ivln-ce_amd", "build.py")).read()
    assert '"rgb_bwd.hip"' in build_src and "ivln_rgb_bwd.h" in build_src
    # refusals need no GPU: nothing is launched
    i64, f32, one = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p(16)
    assert L.ivln_bn_apply_f32(None, None, None, None, None, None, None, 1, 4, 4, 1, None, None) == -1
    assert L.ivln_bn_apply_f32(one, one, one, None, None, None, None, 1, 0, 4, 1, one, None) == -1
    assert L.ivln_bn_apply_f32(one, one, one, None, one, None, None, 1, 4, 4, 1, one, None) == -1  # x2 without its scale
    assert L.ivln_bn_bwd_f32(None, None, None, None, None, None, 1, 4, 4, 1, f32(1e-5), None, None, None, None, None,
                             i64(0), None) == -1
    assert L.ivln_bn_bwd_f32(one, one, one, one, one, None, 0, 4, 4, 1, f32(1e-5), one, None, one, one, one, i64(1 << 20),
                             None) == -1
    assert L.ivln_bn_bwd_f32(one, one, one, one, one, None, 1, 4, 4, 1, f32(1e-5), one, None, one, one, one, i64(4 * 4 + 1),
                             None) == -1  # the scratch is too small
    assert L.ivln_adaptive_avgpool2d_bwd_f32(None, 1, 1, 7, 7, 4, 4, i64(0), None, None) == -1
    assert L.ivln_adaptive_avgpool2d_bwd_f32(one, 1, 1, 7, 0, 4, 4, i64(0), one, None) == -1
    assert L.ivln_adaptive_avgpool2d_bwd_f32(one, 1, 8, 7, 7, 4, 4, i64(16), one, None) == -1  # stride below C * OH * OW
