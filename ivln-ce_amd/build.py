"""Builds libivln_hip.so (hand-written HIP kernels + the C ABI of include/ivln_hip.h) in-tree for
gfx950 with hipcc.  `python ivln-ce_amd/build.py` or `__graft_entry__.build()`.  hipcc
cross-compiles without a GPU; the .so is git-ignored but travels to the GPU box."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libivln_hip.so")

# per-file extra flags; the mapper must round every op exactly where written
SOURCES = {
    "mapper.hip": ["-ffp-contract=off"],
    # (the register-tiled variants' epilogue nests exceed the default pragma-unroll budget: left rolled, their accumulators
    #  were indexed dynamically and lived in scratch - 968 / 352 scratch instructions in these two files)
    "gemm_conv.hip": ["-mllvm", "-pragma-unroll-threshold=200000"],
    "conv_direct.hip": [],
    "gemm_vec.hip": ["-mllvm", "-pragma-unroll-threshold=200000"],
    "conv1x1_stream.hip": [],
    "conv_bf3.hip": [],
    "gn_conv.hip": [],
    "depth_net.hip": [],
    "group_conv.hip": [],
    "cma_step.hip": [],
    "state_rnn.hip": [],
    # (GRU instruction encoder: its register arrays are indexed by fully unrolled loops only - 0 scratch bytes)
    "instr_rnn.hip": [],
    "text_feat.hip": [],
    "nn_ops.hip": [],
    "train_ops.hip": [],
    "depth_bwd.hip": [],
    "rgb_bwd.hip": [],
    "seg_loss.hip": [],
    # (the augmentation's float steps round where they are written, as its float32 restatement in the tests does)
    "seg_augment.hip": ["-ffp-contract=off"],
    # (the renderer's float steps round where they are written: boxworld.render_reference equals it bit for bit)
    "boxworld.hip": ["-ffp-contract=off"],
    "dtw.cpp": [],
}
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_all(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hpp"))]
    headers.append(os.path.join(HERE, "..", "include", "ivln_hip.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_rednet_glue.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_depth_bwd.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_rgb_bwd.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_text_feat.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_known_lib.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_map_sizes.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_map_build.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_map_seed.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_seg_train.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_seg_augment.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_tour_state.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_depth_backbones.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_conv_ks_waves.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_boxworld.h"))
    headers.append(os.path.join(HERE, "..", "include", "ivln_mapper_debug.h"))
    procs = []
    for src, extra in SOURCES.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.rsplit(".", 1)[0] + ".o")
        objs.append(o)
        if force or _stale(o, [s] + headers):
            cmd = [hipcc] + COMMON + extra + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    if force or procs or _stale(OUT, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
