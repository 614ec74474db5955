"""The error bar and the small helpers the per-kernel GPU test files share (tests/test_gpu_train_kernels.py,
tests/test_gpu_train_gemms.py, tests/test_gpu_forward_kernels.py).  Not a conftest: plain functions, imported by name.

Error bar (no tuned constants): e32 = max|fp32 torch-CPU - float64| is the reference arithmetic's own fp32 noise on the
case's inputs; a kernel must stay within  4 * e32 + 4 * 2^-24 * max|float64|  (4: another summation order than torch's).
Every comparison is written to a log in the suite's log directory before anything is asserted; `log` names the file
(train_kernels.log unless a test file says otherwise)."""
import os
import re

import pytest
import torch

EPS = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_LOG = "train_kernels.log"
_log_open = set()


def _log_dir():
    """The suite's log directory: the git-ignored `*_out/` directory the other GPU tests write their parity logs to
    (relative to the working directory, like theirs); IVLN_TEST_LOG_DIR overrides."""
    if os.environ.get("IVLN_TEST_LOG_DIR"):
        return os.environ["IVLN_TEST_LOG_DIR"]
    for line in open(os.path.join(ROOT, ".gitignore")):
        if re.fullmatch(r"\w+_out/", line.strip()):
            return line.strip().rstrip("/")
    return "test_logs"


def _log(line, log=TRAIN_LOG):
    os.makedirs(_log_dir(), exist_ok=True)
    with open(os.path.join(_log_dir(), log), "a" if log in _log_open else "w") as f:
        f.write(line + "\n")
    _log_open.add(log)


class _Bar:
    """Collects the comparisons of one case: everything is logged before anything is asserted."""

    def __init__(self, case, log=TRAIN_LOG):
        self.case, self.bad, self.log = case, [], log

    def check(self, name, got, ref64, ref32, factor=4.0, mag=None):
        """mag: the magnitude the kernel's arithmetic rounds at where that is not max|ref64| (a derived quantity, stated
        at the call: never a tuned constant)"""
        got = got.detach().cpu().double().reshape(-1)
        r64 = ref64.detach().double().reshape(-1)
        r32 = ref32.detach().double().reshape(-1)
        assert got.shape == r64.shape == r32.shape, (name, got.shape, r64.shape, r32.shape)
        err = float((got - r64).abs().max())
        e32 = float((r32 - r64).abs().max())
        mx = float(r64.abs().max()) if mag is None else float(mag)
        bar = factor * e32 + 4 * EPS * mx
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
        ok = err <= bar  # (False for NaN)
        line = (f"{self.case:44s} {name:10s} hip {err:.3e}  e32 {e32:.3e}  hip/e32 {ratio:8.2f}  max|ref| {mx:.3e}  "
                f"bar {bar:.3e}  {'ok' if ok else 'OVER'}")
        _log(line, self.log)
        if not ok:
            self.bad.append(line)
        return err, bar

    def within(self, name, a, b, bar):
        """two kernel results of the same quantity: no further apart than that quantity's bar"""
        d = float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())
        ok = d <= bar
        _log(f"{self.case:44s} {name:10s} apart {d:.3e}  bar {bar:.3e}  {'ok' if ok else 'OVER'}", self.log)
        if not ok:
            self.bad.append(f"{name}: {d:.3e} apart, bar {bar:.3e}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _twice(fn):
    """fn() -> tuple of fresh fp32 output tensors; run twice, identical bytes required (fixed reduction orders)."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        assert _same_bytes(x, y), f"output {i} differs between two runs on the same inputs"
    return a


def _refused(code, fn, *args, **kw):
    """a launcher's precondition: the wrapper raises with that return code"""
    from ivln_ce_amd._lib import IvlnError

    with pytest.raises(IvlnError, match=r"\(%d\)" % code):
        fn(*args, **kw)
