"""CPU: the reference the trainable depth encoder's gradients are compared with (tests/depth_twin.py) - the mask-frozen
float64 twin agrees with torch's own fp32 autograd to fp32 rounding, free float64 autograd does not (ReLU and max-pool
kinks flip between the precisions).  That is why the GPU tests use the twin."""
import ctypes
import os
import re

import torch

import depth_twin as DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worst(got, ref):
    rel = {k: float((got[k].double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref}
    return max(rel.values()), sorted(rel.values())[len(rel) // 2], sum(v > 1e-3 for v in rel.values())


def test_frozen_twin_matches_fp32_autograd_and_free_float64_does_not():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    g = torch.Generator().manual_seed(11)
    depth = torch.rand(2, 256, 256, 1, generator=g)
    enc = DT.oracle_encoder()
    feats, masks, pool_idx = DT.record_masks(enc, depth)
    d_feats = torch.randn(feats.shape, generator=g)
    feats.backward(d_feats)
    fp32 = {k: p.grad.detach().clone() for k, p in enc.named_parameters()}
    assert len(fp32) == 162 and len(masks) == 50

    twin, feats64 = DT.twin_gradients(enc.state_dict(), depth, masks, pool_idx, d_feats)
    w_twin, med_twin, _ = _worst(fp32, twin)
    # the twin's forward is the fp32 pass's function: same features up to rounding
    assert float((feats64 - feats.detach().double()).abs().max()) < 1e-4

    free = DT.oracle_encoder(enc.state_dict()).double()
    free({"depth": depth.double()}).backward(d_feats.double())
    free = {k: p.grad.detach() for k, p in free.named_parameters()}
    w_free, med_free, over = _worst(fp32, free)
    print(f"fp32 autograd vs frozen twin: worst {w_twin:.2e} median {med_twin:.2e}; vs free float64: worst {w_free:.2e} "
          f"median {med_free:.2e}, {over} of {len(free)} tensors over 1e-3")
    assert w_twin < 1e-4, w_twin
    assert w_free > 1e-3, w_free


def test_library_exports_every_entry_of_the_depth_backward_header():
    """include/ivln_depth_bwd.h (the code of include/ivln_hip.h is pinned: later entry points get a header of their own)
    declares the three entry points, the library exports them, and ops.py binds each."""
    import __graft_entry__ as ge

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivln_depth_bwd.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", src)))
    assert names == ["ivln_groupnorm_bwd_f32", "ivln_maxpool3s2_bwd_f32", "ivln_weight_oi_transpose_f32"]
    L = ctypes.CDLL(ge.build())
    assert all(hasattr(L, n) for n in names)
    ops_src = open(os.path.join(ROOT, "ivln-ce_amd", "ops.py")).read()
    assert all(f"L.{n}(" in ops_src for n in names)
    # refusals need no GPU: nothing is launched
    assert L.ivln_groupnorm_bwd_f32(None, None, None, None, None, None, 1, 4, 4, 2, None, None, None, None, None,
                                    ctypes.c_int64(0), None) == -1
    assert L.ivln_maxpool3s2_bwd_f32(None, None, 1, 4, 4, None, None) == -1
    assert L.ivln_weight_oi_transpose_f32(None, None, 1, 1, 1, None) == -1
