"""ECAPA-TDNN speaker / style reference encoder (drop-in for reference msmctts/networks/vqgantts/tdnn.py:67-244): the
``global_encoder`` of ``MSMCVQGANEmb``.  Same classes, constructor arguments, sub-module names and ``state_dict`` keys (in the
reference's order, every BatchNorm buffer included).  Input ``[B, T, in_channels]`` as in the reference; inside, activations
stay channels-last ``[B, T, C]`` -- no transposes.

With ``use_hip = True`` (the default, an instance attribute of ``ECAPA_TDNN``):
  * every convolution (``layer1`` k = 5, the Res2 branches k = 3 at dilation 2 / 3 / 4, every 1x1, the pooling's two layers) is
    a ``plain=True`` layer of ONE ``ConvBank`` on the implicit-GEMM kernels;
  * ``bn(relu(conv(x)))`` is ``hip/tdnn.py relu_batch_norm``, the SE gate with the block's residual ``se_residual``, the pooling
    ``attentive_stats_pool`` behind ``msmc_tanh_*`` (csrc/tdnn.hip);
  * the Res2 branches work on CONTIGUOUS COPIES of their ``width`` channels (the convolution kernels take dense rows): the split,
    the running sum ``sp + spx[i]`` and the final concatenation are stock slicing / add / cat on ``[B, T, width]`` tensors;
    the concatenation of the three blocks' outputs is a stock ``cat`` too;
  * the tail ``bn1 -> linear -> bn2`` acts on ``[B, 6 channels]`` rows, B of them: stock operators, fp32.
``use_hip = False`` is the stock-operator form of the same modules; it exists so that tests have something to compare with.
There is no silent fallback: off the GPU (and without the kernel interpreter bound) the forward raises.

Sizes the kernels take: ``in_channels % 8 == 0`` and a Res2 branch width ``channels / scale`` that is a multiple of 8 (with the
default ``scale = 8``: ``channels % 64 == 0``) -- the convolution kernels' channel granularity.  Anything else is refused at
construction with ``NotImplementedError``.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...hip import norm as hipnorm
from ...hip import tdnn as hiptdnn
from ...hip.convnet import ConvBank, ConvLayer, hip_conv
from ..acoustic_models.transformer import _interpreter_bound


class _Hip(object):
    """what the sub-modules need to run on the kernels: the encoder's bank and its layer table"""

    def __init__(self, bank, layers):
        self.bank, self.layers = bank, layers

    def conv(self, module, x, out_slope=1.0):
        """``module`` (nn.Conv1d) on channels-last x [B, T, Cin]"""
        return hip_conv(self.bank, self.layers[id(module)], x.contiguous().unsqueeze(1), out_slope=out_slope).squeeze(1)


def _conv_stock(module, x):
    return module(x.transpose(1, 2)).transpose(1, 2)


def _relu_bn(bn, x, hip):
    if hip is not None:
        return hiptdnn.relu_batch_norm(x, bn)
    return bn(F.relu(x).transpose(1, 2)).transpose(1, 2)


class Res2Conv1dReluBn(nn.Module):
    """reference :69-103 (in_channels == out_channels == channels)"""

    def __init__(self, channels, kernel_size=1, stride=1, padding=0, dilation=1, bias=False, scale=4):
        super().__init__()
        assert channels % scale == 0, "{} % {} != 0".format(channels, scale)
        self.scale = scale
        self.width = channels // scale
        self.nums = scale if scale == 1 else scale - 1
        self.convs = nn.ModuleList([nn.Conv1d(self.width, self.width, kernel_size, stride, padding, dilation, bias=bias)
                                    for _ in range(self.nums)])
        self.bns = nn.ModuleList([nn.BatchNorm1d(self.width) for _ in range(self.nums)])

    def forward(self, x, hip=None):
        out = []
        spx = torch.split(x, self.width, -1)
        for i in range(self.nums):
            sp = spx[i] if i == 0 else sp + spx[i]
            sp = hip.conv(self.convs[i], sp) if hip is not None else _conv_stock(self.convs[i], sp)
            sp = _relu_bn(self.bns[i], sp, hip)                   # order: conv -> relu -> bn
            out.append(sp)
        if self.scale != 1:
            out.append(spx[self.nums])
        return torch.cat(out, dim=-1)


class Conv1dReluBn(nn.Module):
    """reference :109-116"""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, dilation=1, bias=False):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, stride, padding, dilation, bias=bias)
        self.bn = nn.BatchNorm1d(out_channels)

    def forward(self, x, hip=None):
        x = hip.conv(self.conv, x) if hip is not None else _conv_stock(self.conv, x)
        return _relu_bn(self.bn, x, hip)


class SE_Connect(nn.Module):
    """reference :122-134; ``res`` (the block's residual, reference :150-151) is added in the same pass"""

    def __init__(self, channels, s=2):
        super().__init__()
        assert channels % s == 0, "{} % {} != 0".format(channels, s)
        self.linear1 = nn.Linear(channels, channels // s)
        self.linear2 = nn.Linear(channels // s, channels)

    def forward(self, x, hip=None, res=None):
        if hip is not None:
            return hiptdnn.se_residual(x, torch.zeros_like(x) if res is None else res, self.linear1, self.linear2, holder=self)
        out = torch.sigmoid(self.linear2(F.relu(self.linear1(x.mean(dim=1)))))
        out = x * out.unsqueeze(1)
        return out if res is None else res + out


class SE_Res2Block(nn.Module):
    """reference :140-151"""

    def __init__(self, channels, kernel_size, stride, padding, dilation, scale):
        super().__init__()
        self.model = nn.Sequential(
            Conv1dReluBn(channels, channels, kernel_size=1, stride=1, padding=0),
            Res2Conv1dReluBn(channels, kernel_size, stride, padding, dilation, scale=scale),
            Conv1dReluBn(channels, channels, kernel_size=1, stride=1, padding=0),
            SE_Connect(channels))

    def forward(self, x, hip=None):
        h = self.model[2](self.model[1](self.model[0](x, hip), hip), hip)
        return self.model[3](h, hip, res=x)


class AttentiveStatsPool(nn.Module):
    """reference :156-170: attentive weighted mean and standard deviation over ALL frames (the reference passes no lengths)"""

    def __init__(self, in_dim, bottleneck_dim):
        super().__init__()
        self.linear1 = nn.Conv1d(in_dim, bottleneck_dim, kernel_size=1)
        self.linear2 = nn.Conv1d(bottleneck_dim, in_dim, kernel_size=1)

    def forward(self, x, hip=None):
        if hip is not None:
            a = hip.conv(self.linear2, hipnorm.tanh(hip.conv(self.linear1, x)))
            return hiptdnn.attentive_stats_pool(x.contiguous(), a, holder=self)
        alpha = torch.softmax(_conv_stock(self.linear2, torch.tanh(_conv_stock(self.linear1, x))), dim=1)
        mean = torch.sum(alpha * x, dim=1)
        residuals = torch.sum(alpha * x ** 2, dim=1) - mean ** 2
        return torch.cat([mean, torch.sqrt(residuals.clamp(min=1e-9))], dim=1)


class ECAPA_TDNN(nn.Module):
    """reference :180-244.  ``forward(x)``: x [B, T, in_channels] -> [B, embd_dim]; ``forward((x_list, alpha))``: the pooled
    statistics of several references mixed with weights alpha [B, n] -- linear in the mean, log-linear in the std (:215-244)."""

    def __init__(self, in_channels=80, embd_dim=192, channels=512, scale=8):
        super().__init__()
        if not (isinstance(channels, int) and channels > 0 and channels % scale == 0 and (channels // scale) % 8 == 0):
            raise NotImplementedError('ECAPA_TDNN: channels = %r with scale = %r gives Res2 branches of %s channels; the convolution '
                                      'kernels take multiples of 8 (scale 8: channels %% 64 == 0)'
                                      % (channels, scale, channels / scale if isinstance(channels, int) and scale else '?'))
        if not (isinstance(in_channels, int) and in_channels > 0 and in_channels % 8 == 0):
            raise NotImplementedError('ECAPA_TDNN: in_channels = %r; the convolution kernels take in_channels %% 8 == 0' % (in_channels,))
        self.in_channels = in_channels
        self.layer1 = Conv1dReluBn(in_channels, channels, kernel_size=5, padding=2)
        self.layer2 = SE_Res2Block(channels, kernel_size=3, stride=1, padding=2, dilation=2, scale=scale)
        self.layer3 = SE_Res2Block(channels, kernel_size=3, stride=1, padding=3, dilation=3, scale=scale)
        self.layer4 = SE_Res2Block(channels, kernel_size=3, stride=1, padding=4, dilation=4, scale=scale)
        cat_channels = channels * 3
        self.conv = nn.Conv1d(cat_channels, cat_channels, kernel_size=1)
        self.pooling = AttentiveStatsPool(cat_channels, 128)
        self.bn1 = nn.BatchNorm1d(cat_channels * 2)
        self.linear = nn.Linear(cat_channels * 2, embd_dim)
        self.bn2 = nn.BatchNorm1d(embd_dim)
        self.use_hip = True
        self.hip_dtype = torch.float32        # compute dtype of the frame passes (bf16 runs: torch.bfloat16)
        self._bank = None

    def _hip_ready(self, dev):
        """(build and) refresh the kernel-layout weights of every convolution: one call per forward"""
        if not self.use_hip:
            return None
        if not (dev.type == 'cuda' or _interpreter_bound()):
            raise RuntimeError('ECAPA_TDNN runs on the gfx950 kernels only: move the module to the GPU (tests: bind the interpreter '
                               'build, or set use_hip = False for the stock-operator comparison form)')
        if self._bank is None:
            self._layers = {id(m): ConvLayer(m, 'conv', (1, m.kernel_size[0]), (1, 1), (1, m.dilation[0]), (0, m.padding[0]),
                                             plain=True)
                            for m in self.modules() if isinstance(m, nn.Conv1d)}
            self._bank = ConvBank(list(self._layers.values()))
        self._bank.prepare(self.hip_dtype)
        return _Hip(self._bank, self._layers)

    def _pooled(self, x, hip):
        """[B, T, in_channels] -> (mean | std) [B, 6 channels] in fp32"""
        if hip is not None:
            x = x.to(self.hip_dtype).contiguous()
        out1 = self.layer1(x, hip)
        out2 = self.layer2(out1, hip)
        out3 = self.layer3(out2, hip)
        out4 = self.layer4(out3, hip)
        out = torch.cat([out2, out3, out4], dim=-1)
        if hip is not None:
            out = hip.conv(self.conv, out, out_slope=0.0)         # ReLU in the convolution's epilogue
        else:
            out = F.relu(_conv_stock(self.conv, out))
        return self.pooling(out, hip).float()

    def _tail(self, mean_std):
        return self.bn2(self.linear(self.bn1(mean_std)))

    def forward(self, x):
        if isinstance(x, (tuple, list)):
            return self.manipulate(x)
        return self._tail(self._pooled(x, self._hip_ready(x.device)))

    def manipulate(self, x):
        x, alpha = x
        hip = self._hip_ready(x[0].device)
        res = [self._pooled(seq, hip) for seq in x]
        means, stds = [], []
        for i in range(len(x)):
            mean, std = torch.chunk(res[i], 2, dim=1)
            means.append(mean * alpha[:, i])
            stds.append(std.log() * alpha[:, i])
        return self._tail(torch.cat((sum(means), sum(stds).exp()), dim=1))
