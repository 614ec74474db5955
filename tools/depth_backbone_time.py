"""Cost of the depth encoder on the DD-PPO backbones beyond ResNet-50 (MODEL.DEPTH_ENCODER.backbone), on an MI355X:

    python tools/depth_backbone_time.py [--out profiles/depth_backbones.txt] [--no-trace]

The encoder forward (256x256 depth -> (B, 128, 4, 4)) at 8 and at 4 images for `resnet50` on the conv + GroupNorm pair
path (ops.DEPTH_NET = 0, chain off - the form the other backbones run, so the yardstick of the same run) and for each
new backbone.  Every measurement is a child process of its own under its own time limit; the parent never opens the
GPU, runs one child at a time and stops at the first child that is killed, times out or aborts.
  time    the median over LOOPS timed loops of ITERS forwards each, a host clock around work that ends in a device
          synchronise, after WARM untimed forwards (eager launches: host enqueue included, as a rollout step pays it)
  shares  a second run of the child under `rocprofv3 --kernel-trace` (the profiler off for the times above): the kernel
          time of the grouped conv (k_gconv3x3_*) and of the SE launches (k_se_gate, k_se_apply) over all kernel time
There is no target: the figure to read a backbone against is the resnet50 pair path of the same run."""
import argparse
import glob
import os
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("resnet50", "resneXt50", "se_resnet50", "se_resneXt50", "se_resneXt101")
WARM, ITERS, LOOPS = 10, 20, 9
DEAD = (124, 137, 134, 139, -6, -9, -11)  # time limit, kill, abort, segmentation fault: nothing more is started after one


def child(name, B, traced):
    sys.path.insert(0, ROOT)
    import torch

    from ivln_ce_amd import ops
    from ivln_ce_amd.encoders import ResNetEncoder

    dev = torch.device("cuda:0")
    ops.DEPTH_NET, ops.CHAIN_GN_CONV = 0, False  # pair path for resnet50; the others have no other form
    torch.manual_seed(5)
    enc = ResNetEncoder((256, 256, 1), backbone=name).eval().to(dev)
    for p in enc.parameters():
        p.requires_grad_(False)
    depth = torch.rand(B, 256, 256, 1, generator=torch.Generator().manual_seed(2)).to(dev)
    obs = {"depth": depth}
    with torch.no_grad():
        for _ in range(WARM):
            enc(obs)
        torch.cuda.synchronize()
        if traced:  # (the profiler slows the host: kernel durations only, no wall time reported)
            for _ in range(ITERS):
                enc(obs)
            torch.cuda.synchronize()
            print("TRACED", flush=True)
            return
        ms = []
        for _ in range(LOOPS):
            t0 = time.perf_counter()
            for _ in range(ITERS):
                enc(obs)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / ITERS)
    print(f"RESULT {statistics.median(ms):.4f} {min(ms):.4f} {max(ms):.4f}", flush=True)


def shares(db):
    """rocpd kernel-trace database -> (total kernel ns, {family: ns}, launches per forward of each family)"""
    cur = sqlite3.connect(db).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    namecol = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    fam = {"k_gconv3x3": [0, 0], "k_se_gate": [0, 0], "k_se_apply": [0, 0]}
    total = 0
    for n, d in cur.execute(f"select {namecol}, (end - start) from kernels"):
        total += d
        for k in fam:
            if k in n:
                fam[k][0] += d
                fam[k][1] += 1
    return total, fam


def run_child(args, limit, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        return 124, ""
    return r.returncode, r.stdout + r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, metavar=("NAME", "B", "TRACED"))
    ap.add_argument("--out")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.child[2] == "1")
    lines = [f"depth encoder forward, 256x256 depth, eager launches; median of {LOOPS} loops of {ITERS} forwards after "
             f"{WARM} warm-up forwards (min .. max of the loops); resnet50 = conv + GroupNorm pair path",
             f"{'backbone':14s} {'B':>2s} {'ms/forward':>10s} {'min':>8s} {'max':>8s} {'vs resnet50 pairs':>18s}"]
    base, dead = {}, False
    for B in (8, 4):
        for name in NAMES:
            rc, out = run_child((name, B, 0), a.limit)
            res = [l for l in out.splitlines() if l.startswith("RESULT")]
            if rc != 0 or not res:
                lines.append(f"{name:14s} {B:2d} failed (exit {rc})")
                print(out[-2000:], file=sys.stderr)
                if rc in DEAD:
                    dead = True
                    break
                continue
            med, lo, hi = (float(x) for x in res[0].split()[1:])
            if name == "resnet50":
                base[B] = med
            lines.append(f"{name:14s} {B:2d} {med:10.3f} {lo:8.3f} {hi:8.3f} {med / base[B] if B in base else float('nan'):17.2f}x")
            print(lines[-1], flush=True)
        if dead:
            break
    if not a.no_trace and not dead:
        lines += ["", f"kernel-time shares (rocprofv3 --kernel-trace, {WARM + ITERS} forwards; launches per forward in brackets)",
                  f"{'backbone':14s} {'B':>2s} {'kernel ms/fwd':>13s} {'grouped conv':>16s} {'se_gate':>16s} {'se_apply':>16s}"]
        for B in (8,):  # (one batch size: the shares move little with it, and every traced child costs GPU time)
            for name in NAMES[1:]:
                with tempfile.TemporaryDirectory() as tmp:
                    rc, out = run_child((name, B, 1), a.limit + 60, prefix=("rocprofv3", "--kernel-trace", "-d", tmp, "--"))
                    dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
                    if rc != 0 or "TRACED" not in out or not dbs:
                        lines.append(f"{name:14s} {B:2d} trace failed (exit {rc}, {len(dbs)} database(s))")
                        print(out[-2000:], file=sys.stderr)
                        if rc in DEAD:
                            dead = True
                            break
                        continue
                    total, fam = shares(dbs[0])
                n = WARM + ITERS
                cell = lambda k: f"{100.0 * fam[k][0] / max(total, 1):5.1f}% [{fam[k][1] / n:4.1f}]"  # noqa: E731
                lines.append(f"{name:14s} {B:2d} {total / n * 1e-6:13.3f} {cell('k_gconv3x3'):>16s} {cell('k_se_gate'):>16s} {cell('k_se_apply'):>16s}")
                print(lines[-1], flush=True)
            if dead:
                break
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    sys.stdout.write(text)
    return 1 if dead else 0


if __name__ == "__main__":
    sys.exit(main())
