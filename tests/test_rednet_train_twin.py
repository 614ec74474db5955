"""CPU: pins tests/rednet_twin.py's five-output training forward to the reference's own RedNet in train mode
(tests/golden/rednet_train.npz, written by tests/golden/gen_rednet_train_golden.py), and checks that the frozen twin is
the function the free pass computed - the property the fine-tuning tests' gradient references rest on."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import rednet_twin as RW  # noqa: E402
from det_init import det_fill  # noqa: E402


def _twin():
    return det_fill(RW.RedNetTwin(), seed=1, conv_gain=0.6)


def test_twin_training_forward_matches_the_reference_golden():
    """Bar: the golden is the reference's fp32 pass and the twin here is another fp32 pass of the same arithmetic, each away
    from the exact result by its own rounding noise, which train-mode BatchNorm over layer 4's eight values per channel
    amplifies (and which depends on the host's thread count and conv kernels).  e32 = max|fp32 twin - float64 twin| measures
    that noise on these inputs; two such passes differ by at most about 2 e32, so the bar is 4 e32 + 1e-5 per output and per
    statistic (on the host that wrote the golden the difference is zero)."""
    g = np.load(os.path.join(HERE, "golden", "rednet_train.npz"))
    torch.set_num_threads(min(8, torch.get_num_threads()))
    net, net64 = _twin().train(), _twin().double().train()
    rgb, depth = RW.golden_inputs()
    with torch.no_grad():
        outs = net.forward_train(rgb, depth)
        outs64 = net64.forward_train(rgb.double(), depth.double())
    out = outs[0]
    assert [tuple(o.shape[2:]) for o in outs] == [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)]
    e32 = [float((a.double() - b).abs().max()) for a, b in zip(outs, outs64)]

    def close(a, ref, e, scale=1.0):
        return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max()) <= scale * (4 * e + 1e-5)

    for i, name in ((1, "out2"), (2, "out3"), (3, "out4"), (4, "out5")):
        assert close(outs[i].numpy(), g[name], e32[i]), (name, e32[i])
    assert close(out[:, :, ::3, ::3].numpy(), g["out_s3"], e32[0]), e32[0]
    assert close(out.double().sum((2, 3)).numpy(), g["out_sums"], e32[0], scale=64 * 64)
    sd, sd64 = net.state_dict(), net64.state_dict()
    stats = sorted(k.split(":", 1)[1] for k in g.files if k.startswith("mean:"))
    assert len(stats) >= 10
    for name in stats:
        assert int(sd[name + ".num_batches_tracked"]) == 1, name
        for kind, key in (("mean:", ".running_mean"), ("var:", ".running_var")):
            e = float((sd[name + key].double() - sd64[name + key]).abs().max())
            assert close(sd[name + key].numpy(), g[kind + name], e), (name, key, e)


def test_frozen_twin_is_the_function_the_free_pass_computed():
    """Masks and pool indices recorded by a free fp32 pass, replayed: the same outputs, the same gradients and the same
    running statistics (bit for bit but for the order of a few sums: 1e-6 relative), every kink used exactly once."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    state = _twin().state_dict()
    g = torch.Generator().manual_seed(3)
    rgb, depth = torch.randn(2, 3, 32, 32, generator=g), torch.randn(2, 1, 32, 32, generator=g)
    d_outs = [torch.randn(2, 13, 32 >> i, 32 >> i, generator=g) for i in range(5)]
    free = RW.run(state, rgb, depth, d_outs, dtype=torch.float32)
    assert len(free["masks"]) == 2 + 2 * 16 * 3 + 5 + 2 * (6 + 4 + 3 + 3 + 3) and len(free["pools"]) == 2
    froz = RW.run(state, rgb, depth, d_outs, free["masks"], free["pools"], dtype=torch.float32)
    for a, b in zip(free["outs"], froz["outs"]):
        assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())
    assert sorted(free["grads"]) == sorted(froz["grads"]) and len(free["grads"]) == 469
    for k, a in free["grads"].items():
        assert float((a - froz["grads"][k]).abs().max()) <= 1e-5 * float(a.abs().max()) + 1e-12, k
    for k, a in free["bufs"].items():
        assert torch.allclose(a.double(), froz["bufs"][k].double(), rtol=1e-6, atol=1e-7), k
