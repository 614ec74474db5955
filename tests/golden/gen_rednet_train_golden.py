"""Golden vectors for RedNet's five-output TRAINING forward from the REFERENCE's own module
(ivlnce_baselines/common/mapping_module/rednet.py:224-256 with self.training) with det_init weights, B = 2, 64 x 64.
Build container only:  python tests/golden/gen_rednet_train_golden.py  -> tests/golden/rednet_train.npz

Kept small: out5 .. out2 whole, the full-resolution `out` at every third row and column (both parities of the final 2 x 2
stride-2 transposed conv) with its per-(image, class) sums in float64, and the running statistics of a handful of BatchNorms
from both encoders, the skips and the decoder after the one pass."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_shim  # noqa: E402

_ref_shim.install()
torch.set_num_threads(8)
from det_init import det_fill  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rednet_twin import golden_inputs  # noqa: E402  (tests/rednet_twin.py: the inputs the pin test feeds its twin)

from ivlnce_baselines.common.mapping_module.rednet import RedNet  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
STAT_LAYERS = ("bn1", "bn1_d", "layer1.0.downsample.1", "layer2_d.3.bn2", "layer4.2.bn3", "layer4_d.0.bn1", "agant0.1", "agant4.1",
               "deconv1.5.upsample.1", "deconv1.5.bn2", "deconv3.0.bn1", "final_conv.2.bn2")


if __name__ == "__main__":
    cfg = {"arch": "rednet", "resnet_pretrained": False, "finetune": True, "SUNRGBD_pretrained_weights": "",
           "n_classes": 13, "upsample_prediction": True, "load_model": ""}
    net = det_fill(RedNet(cfg), seed=1, conv_gain=0.6).train()
    rgb, depth = golden_inputs()
    with torch.no_grad():
        # (the reference's own `forward` unpacks two values and so cannot run in train mode: its two halves, as a training
        #  loop has to call them)
        out, out2, out3, out4, out5 = net.forward_upsample(*net.forward_downsample(rgb, depth))
    sd = net.state_dict()
    data = dict(out_s3=out[:, :, ::3, ::3].numpy(), out_sums=out.double().sum((2, 3)).numpy(), out2=out2.numpy(),
                out3=out3.numpy(), out4=out4.numpy(), out5=out5.numpy())
    for name in STAT_LAYERS:
        data[f"mean:{name}"] = sd[name + ".running_mean"].numpy()
        data[f"var:{name}"] = sd[name + ".running_var"].numpy()
        assert int(sd[name + ".num_batches_tracked"]) == 1
    path = os.path.join(OUT, "rednet_train.npz")
    np.savez_compressed(path, **data)
    print("out", tuple(out.shape), float(out.abs().max()), [tuple(o.shape) for o in (out2, out3, out4, out5)])
    print(os.path.getsize(path) // 1024, "KiB")
