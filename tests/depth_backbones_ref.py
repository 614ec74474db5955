"""TEST INFRASTRUCTURE ONLY - plain torch (CPU, float32 or float64) restatement of the DD-PPO depth backbones other than
ResNet-50: resneXt50, se_resnet50, se_resneXt50, se_resneXt101 of habitat-lab v0.1.7
habitat_baselines/rl/ddppo/policy/resnet.py, inside the `ResNetEncoder` shell of oracle/habitat_ext_ref.py (whose `ResNet`
and `_make_layer` carry the `cardinality` / `resneXt` hooks).  Imported by the tests, never by the package.

  ResNeXt bottleneck   expansion 2; the four layers run on doubled base planes (the stem keeps the undoubled width);
                       conv3x3(planes, planes, stride, groups=cardinality), cardinality = int(base_planes / 2) taken before
                       the doubling - with baseplanes 32: 16 groups of 4, 8, 16, 32 channels, outputs 128 ... 1024.
                       Every block of a layer gets the cardinality (the oracle file hands it to the first only, which
                       cannot matter for its ResNet-50).
  SE bottleneck        se = SE(planes * expansion, r=16): squeeze = AdaptiveAvgPool2d(1), excite = Linear(C, C/16) - ReLU -
                       Linear(C/16, C) - Sigmoid;  out = convs(x); out = se(out) * out; relu(out + identity).
  se_resneXt101        layers [3, 4, 23, 3].

PARITY UNPINNED, as the oracle's ResNet-50 is: habitat-lab cannot be imported here and the reference holds no golden
vectors for these modules, so this restatement IS the definition the HIP kernels are checked against.  What is pinned is
the structural contract with real DD-PPO checkpoints, which the encoder loads with strict=True: the state-dict key names
`backbone.layerL.i.convs.{0,1,3,4,6,7}.*`, `backbone.layerL.i.se.excite.{0,2}.{weight,bias}`, `backbone.layerL.0.downsample.{0,1}.*`."""
import os
import sys
import types

import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import habitat_ext_ref as R  # noqa: E402

NAMES = ("resneXt50", "se_resnet50", "se_resneXt50", "se_resneXt101")


class SE(nn.Module):
    def __init__(self, planes, r=16):
        super().__init__()
        self.squeeze = nn.AdaptiveAvgPool2d(1)
        self.excite = nn.Sequential(
            nn.Linear(planes, int(planes / r)),
            nn.ReLU(True),
            nn.Linear(int(planes / r), planes),
            nn.Sigmoid(),
        )

    def forward(self, x):
        b, c, _, _ = x.size()
        x = self.squeeze(x).view(b, c)
        return self.excite(x).view(b, c, 1, 1)


class Bottleneck(nn.Module):
    expansion = 4
    resneXt = False
    has_se = False

    def __init__(self, inplanes, planes, ngroups, stride=1, downsample=None, cardinality=1):
        super().__init__()
        self.convs = nn.Sequential(
            R.conv1x1(inplanes, planes),
            nn.GroupNorm(ngroups, planes),
            nn.ReLU(True),
            R.conv3x3(planes, planes, stride, groups=cardinality),
            nn.GroupNorm(ngroups, planes),
            nn.ReLU(True),
            R.conv1x1(planes, planes * self.expansion),
            nn.GroupNorm(ngroups, planes * self.expansion),
        )
        if self.has_se:
            self.se = SE(planes * self.expansion, r=16)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.convs(x)
        if self.has_se:
            out = self.se(out) * out
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class SEBottleneck(Bottleneck):
    has_se = True


class ResNeXtBottleneck(Bottleneck):
    expansion = 2
    resneXt = True


class SEResNeXtBottleneck(SEBottleneck):
    expansion = 2
    resneXt = True


class ResNet(R.ResNet):
    """The oracle's ResNet with the cardinality handed to EVERY block of a layer."""

    def _make_layer(self, block, ngroups, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                R.conv1x1(self.inplanes, planes * block.expansion, stride),
                nn.GroupNorm(ngroups, planes * block.expansion),
            )
        layers = [block(self.inplanes, planes, ngroups, stride, downsample, cardinality=self.cardinality)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, ngroups, cardinality=self.cardinality))
        return nn.Sequential(*layers)


def resneXt50(in_channels, base_planes, ngroups):
    return ResNet(in_channels, base_planes, ngroups, ResNeXtBottleneck, [3, 4, 6, 3], cardinality=int(base_planes / 2))


def se_resnet50(in_channels, base_planes, ngroups):
    return ResNet(in_channels, base_planes, ngroups, SEBottleneck, [3, 4, 6, 3])


def se_resneXt50(in_channels, base_planes, ngroups):
    return ResNet(in_channels, base_planes, ngroups, SEResNeXtBottleneck, [3, 4, 6, 3], cardinality=int(base_planes / 2))


def se_resneXt101(in_channels, base_planes, ngroups):
    return ResNet(in_channels, base_planes, ngroups, SEResNeXtBottleneck, [3, 4, 23, 3], cardinality=int(base_planes / 2))


MAKERS = dict(resnet50=R.resnet50, resneXt50=resneXt50, se_resnet50=se_resnet50, se_resneXt50=se_resneXt50,
              se_resneXt101=se_resneXt101)


def depth_space(size=256):
    return types.SimpleNamespace(spaces={"depth": types.SimpleNamespace(shape=(size, size, 1))})


def encoder(name, baseplanes=32, size=256):
    """The oracle's ResNetEncoder shell (avg_pool2d(2) -> backbone -> compression) around backbone `name`."""
    return R.ResNetEncoder(depth_space(size), baseplanes=baseplanes, ngroups=baseplanes // 2, make_backbone=MAKERS[name])
