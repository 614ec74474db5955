"""CPU: every entry point of include/ivln_hip.h's "Non-GEMM forward kernels" section has a per-kernel GPU test
(tests/test_gpu_forward_kernels.py::FWD_COVERED, which may point into another file of the suite), and three pieces of the
kernels' index arithmetic that the GPU tests' references and path assertions lean on - the adaptive average pool's window
bounds, the lanes-per-output choice and slab partition of the BatchNorm -> ReLU -> AvgPool2d(2) tail, the job / block
partition of the multi-tensor copy and add - restated in numpy and held to float64 torch at the GPU tests' shapes."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
OWN = "test_gpu_forward_kernels.py"


def _forward_section_functions():
    src = open(os.path.join(ROOT, "include", "ivln_hip.h")).read()
    start = src.index("Non-GEMM forward kernels (csrc/nn_ops.hip)")
    end = src.index("Fused recurrent / attention head of one rollout step")
    assert 0 < start < end
    sec = re.sub(r"/\*.*?\*/", "", src[src.rindex("/*", 0, start):src.rindex("/*", 0, end)], flags=re.S)
    return sorted(set(re.findall(r"\b(ivln_[a-z0-9_]+)\s*\(", sec)))


def _uncovered(names, covered):
    """(header entries without a key, keys whose value names no existing test_ function)"""
    no_entry = [n for n in names if n not in covered]
    no_test = []
    for n, t in covered.items():
        fname, _, test = t.rpartition("::")
        path = os.path.join(TESTS, fname or OWN)
        ok = test.startswith("test_") and os.path.exists(path) and re.search(r"^def %s\(" % re.escape(test), open(path).read(), flags=re.M)
        if not ok:
            no_test.append(f"{n} -> {t}")
    return no_entry, no_test


def test_every_forward_entry_point_has_a_kernel_test():
    import test_gpu_forward_kernels as K

    names = _forward_section_functions()
    assert len(names) >= 38 and "ivln_groupnorm_f32" in names and "ivln_rednet_fwd" in names and "ivln_copy2d_f32" in names
    assert "ivln_nconv_f32" not in names and "ivln_cma_step_fwd" not in names and "ivln_gemm_f32" not in names
    assert "ivln_colsum_f32" not in names   # named in a comment of the section only
    no_entry, no_test = _uncovered(names, K.FWD_COVERED)
    assert not no_entry, f"declared in the header's forward section without a test in FWD_COVERED: {no_entry}"
    assert not no_test, f"FWD_COVERED names tests that do not exist: {no_test}"
    stale = [n for n in K.FWD_COVERED if n not in names]
    assert not stale, f"FWD_COVERED lists functions the header's forward section does not declare: {stale}"
    # the pin itself: one entry less, or a test that does not exist (here or in the named file), is noticed
    short = dict(K.FWD_COVERED)
    short.pop("ivln_tour_memory_f32")
    assert _uncovered(names, short)[0] == ["ivln_tour_memory_f32"]
    assert _uncovered(names, dict(K.FWD_COVERED, ivln_add_f32="test_that_is_not_there"))[1]
    assert _uncovered(names, dict(K.FWD_COVERED, ivln_add_f32="test_gpu_kernels.py::test_that_is_not_there"))[1]
    assert _uncovered(names, dict(K.FWD_COVERED, ivln_add_f32="no_such_file.py::test_linear"))[1]
    # and the module's tests carry the gpu marker as a whole
    assert K.pytestmark.name == "gpu"


@pytest.mark.parametrize("H,W", [(8, 8), (7, 5), (3, 3), (1, 1)])
def test_adaptive_avgpool_window_bounds(H, W):
    """k_adaptive_avgpool2d's windows [floor(i*H/OH), ceil((i+1)*H/OH)) give F.adaptive_avg_pool2d in float64; a window of
    floor .. floor (the obvious off-by-one) does not, wherever H is no multiple of OH."""
    from test_gpu_forward_kernels import adaptive_windows

    OH = OW = 4
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H * 10 + W), dtype=torch.float64)
    want = F.adaptive_avg_pool2d(x, (OH, OW)).numpy()

    def pooled(hw, ww):
        out = np.zeros((2, 3, OH, OW))
        for i, (h0, h1) in enumerate(hw):
            for j, (w0, w1) in enumerate(ww):
                out[:, :, i, j] = x.numpy()[:, :, h0:h1, w0:w1].mean((2, 3))
        return out

    hw, ww = adaptive_windows(H, OH), adaptive_windows(W, OW)
    assert all(0 <= a < b <= H for a, b in hw) and all(0 <= a < b <= W for a, b in ww)
    assert np.abs(pooled(hw, ww) - want).max() < 1e-14
    if H % OH and H > OH:
        floor_only = [(a, max(a + 1, ((i + 1) * H) // OH)) for i, (a, _) in enumerate(hw)]
        assert np.abs(pooled(floor_only, ww) - want).max() > 1e-3


def _avgpool2_numpy(slabs, scale, shift, N, C, H, W, lpo):
    """k_scale_shift_relu_avgpool2 lane by lane in float64: lane gid serves output gid // lpo and slabs gid % lpo, + lpo, ...;
    lanes past the last output work on output 0 and stay in the xor shuffles; lane sub == 0 of a live output writes."""
    splits = slabs.shape[0]
    Ho, Wo = H // 2, W // 2
    total = N * C * Ho * Wo
    x = slabs.reshape(splits, C, N, H, W)
    lanes = -(-total * lpo // 256) * 256
    part = np.zeros((lanes, 4))
    for gid in range(lanes):
        sub, idx = gid % lpo, gid // lpo
        if idx >= total:
            idx = 0
        wo, ho, nc = idx % Wo, (idx // Wo) % Ho, idx // (Wo * Ho)
        c, n = nc % C, nc // C
        for z in range(sub, splits, lpo):
            part[gid] += x[z, c, n, 2 * ho:2 * ho + 2, 2 * wo:2 * wo + 2].reshape(4)
    off = lpo >> 1
    while off:
        part = part + part[np.arange(lanes) ^ off]
        off >>= 1
    y = np.zeros(total)
    for gid in range(0, total * lpo, lpo):
        idx = gid // lpo
        c = (idx // (Wo * Ho)) % C
        y[idx] = np.maximum(part[gid] * scale[c] + shift[c], 0.0).sum() * 0.25
    return y.reshape(N, C, Ho, Wo)


@pytest.mark.parametrize("splits", [1, 2, 3, 7, 16, 33])
def test_avgpool2_lanes_per_output_and_slab_partition(splits):
    """The launcher's lanes-per-output ladder at the GPU test's (1, 2, 4, 4) map, and its lane / slab partition: every slab
    is summed exactly once per output (float64 torch agrees), the idle lanes' idx = 0 work never reaches a result, and a
    partition that drops the last partial pass (slabs >= lpo * (splits // lpo)) is noticed whenever lpo does not divide
    splits."""
    from test_gpu_forward_kernels import lanes_per_output

    N, C, H, W = 1, 2, 4, 4
    total = N * C * (H // 2) * (W // 2)
    lpo = lanes_per_output(splits, total)
    assert lpo == {1: 1, 2: 2, 3: 2, 7: 4, 16: 16, 33: 16}[splits]
    assert (total * lpo) % 256 != 0 and lanes_per_output(64, 65536) == 1 and lanes_per_output(64, 8192) == 8
    g = torch.Generator().manual_seed(splits)
    slabs = torch.randn(splits, C, N * H * W, generator=g, dtype=torch.float64)
    scale, shift = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    x = slabs.sum(0).view(C, N, H, W).permute(1, 0, 2, 3)
    want = F.avg_pool2d(F.relu(x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)), 2).numpy()
    got = _avgpool2_numpy(slabs.numpy(), scale.numpy(), shift.numpy(), N, C, H, W, lpo)
    assert np.abs(got - want).max() < 1e-13
    if splits % lpo:
        short = _avgpool2_numpy(slabs.numpy()[:lpo * (splits // lpo)], scale.numpy(), shift.numpy(), N, C, H, W, lpo)
        assert np.abs(short - want).max() > 1e-3


def _multi_numpy(srcs, dsts, chunk, vec, aligned, add):
    """k_copy_multi / k_add_multi block by block on numpy arrays (elements: bytes or floats): block b finds its job in
    first_block, takes [off, min(size, off + chunk)), moves whole vectors of `vec` elements up to vend and the rest one by one
    (everything one by one when the job is not aligned).  Returns how often each destination element was written."""
    from test_gpu_forward_kernels import block_partition

    live = [j for j, s in enumerate(srcs) if len(s) > 0]
    sizes, first = block_partition([len(s) for s in srcs], chunk)
    assert sizes == [len(srcs[j]) for j in live]
    hits = [np.zeros(len(d), dtype=np.int64) for d in dsts]
    for b in range(first[-1]):
        m = 0
        while m + 1 < len(sizes) and b >= first[m + 1]:
            m += 1
        j = live[m]
        off = (b - first[m]) * chunk
        end = min(sizes[m], off + chunk)
        assert off < end, "a block without work"
        vend = off + ((end - off) // vec * vec if aligned else 0)
        for lo, hi in ((off, vend), (vend, end)):
            dsts[j][lo:hi] = dsts[j][lo:hi] + srcs[j][lo:hi] if add else srcs[j][lo:hi]
            hits[j][lo:hi] += 1
    return hits


@pytest.mark.parametrize("aligned", [True, False])
def test_copy_multi_and_add_multi_partition(aligned):
    """The GPU tests' job lists through the launchers' first_block table and the kernels' chunk / vector / tail arithmetic:
    every byte (float) of every non-empty job is moved exactly once, empty jobs take no block, and the block counts are the
    ones the GPU tests assert."""
    from test_gpu_forward_kernels import ADD_CHUNK, COPY_CHUNK, block_partition

    rng = np.random.default_rng(3)
    for sizes in ([1, 15, 16, 17, 16383, 16384, 16385, 3 * 16384 + 5], [100, 0, 50, 16400, 3, 0, 7, 33]):
        srcs = [rng.integers(0, 256, n, dtype=np.uint8) for n in sizes]
        dsts = [np.full(n, 0xA5, dtype=np.uint8) for n in sizes]
        hits = _multi_numpy(srcs, dsts, COPY_CHUNK, 16, aligned, add=False)
        assert all((h == 1).all() for h in hits) and all(np.array_equal(s, d) for s, d in zip(srcs, dsts))
    assert block_partition([16384], COPY_CHUNK)[1] == [0, 1] and block_partition([16385], COPY_CHUNK)[1] == [0, 2]
    for sizes in ([1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 3], [k % 7 + 1 for k in range(64)]):
        srcs = [rng.standard_normal(n).astype(np.float32) for n in sizes]
        base = [rng.standard_normal(n).astype(np.float32) for n in sizes]
        dsts = [b.copy() for b in base]
        hits = _multi_numpy(srcs, dsts, ADD_CHUNK, 4, aligned, add=True)
        assert all((h == 1).all() for h in hits)
        for s, b, d in zip(srcs, base, dsts):
            want = (torch.from_numpy(b).double() + torch.from_numpy(s).double()).float()   # one correctly rounded fp32 add
            assert torch.equal(torch.from_numpy(d), want)
    assert block_partition([4096], ADD_CHUNK)[1] == [0, 1] and block_partition([4097], ADD_CHUNK)[1] == [0, 2]
