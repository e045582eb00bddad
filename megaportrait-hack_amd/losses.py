"""The VGG19 perceptual loss of the reference's training step on the project's kernels, forward and gradient.

`PerceptualLoss.compute_vgg19_loss` (model.py:1934-1937, 1981-2017) pushes the predicted and the target image through
`vgg19.features[0:30]`, adds `mean |p - t|` after layers 1, 6, 11, 20 and 29 and sends the gradient back to the predicted image;
train.py:221-223 repeats that per pyramid scale.  `VGG19FeatureLoss` is that expression as a module: the thirteen 3x3 convs run on the
matrix cores (ops.conv2d_stem, ops.conv2d, ops.conv2d_bwd_data), everything between them in csrc/feature_loss.hip, and the whole
stack is ONE autograd node, so the backward is one walk over the saved maps.  The weights are frozen: there is no
weight gradient, and a module whose weights ask for one takes `forward_reference`, the same expression in plain PyTorch.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops
from .autograd import _bwd, _fwd, conv2d_packs

VGG19_CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)   # torchvision's vgg19.features[0:30]: a ReLU follows each conv
VGG19_POOLS = (4, 9, 18, 27)                                     # MaxPool2d(2, 2)
_BLOCKS = (2, 2, 4, 4, 1)                                        # convs per width


def _pair(v) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(a) for a in v)


def _check_layout(seq) -> None:
    """Duck-typed check that `seq` has the 30-layer layout: raises TypeError naming what it expected."""
    try:
        layers = list(seq.children())
    except AttributeError:
        raise TypeError(f"VGG19FeatureLoss: expected an nn.Sequential with torchvision's vgg19.features[0:30] layout, got {type(seq).__name__}") from None
    if len(layers) != 30:
        raise TypeError(f"VGG19FeatureLoss: expected 30 layers (vgg19.features[0:30]), got {len(layers)}")
    ci = 3
    for i, m in enumerate(layers):
        if i in VGG19_CONVS:
            w, b = getattr(m, "weight", None), getattr(m, "bias", None)
            ok = (isinstance(w, torch.Tensor) and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and w.shape[1] == ci
                  and isinstance(b, torch.Tensor) and tuple(b.shape) == (w.shape[0],)
                  and _pair(getattr(m, "stride", 0)) == (1, 1) and _pair(getattr(m, "padding", 0)) == (1, 1)
                  and _pair(getattr(m, "dilation", 1)) == (1, 1) and getattr(m, "groups", 1) == 1
                  and getattr(m, "padding_mode", "zeros") == "zeros")
            if not ok:
                raise TypeError(f"VGG19FeatureLoss: layer {i} must be a Conv2d({ci}, Co, 3, stride=1, padding=1) with a bias, got {m!r}")
            ci = int(w.shape[0])
        elif i in VGG19_POOLS:
            ok = (hasattr(m, "kernel_size") and _pair(m.kernel_size) == (2, 2) and _pair(m.stride if m.stride is not None else m.kernel_size) == (2, 2)
                  and _pair(getattr(m, "padding", 0)) == (0, 0) and _pair(getattr(m, "dilation", 1)) == (1, 1)
                  and not getattr(m, "ceil_mode", False) and "max" in type(m).__name__.lower())
            if not ok:
                raise TypeError(f"VGG19FeatureLoss: layer {i} must be a MaxPool2d(2, 2) in floor mode, got {m!r}")
        elif not isinstance(m, nn.ReLU):
            raise TypeError(f"VGG19FeatureLoss: layer {i} must be a ReLU, got {m!r}")


class VGG19FeatureLossFn(torch.autograd.Function):
    """sum over taps of coeff_k * sum |f_k(predicted) - f_k(target)| through owner.vgg19 (frozen), one node for the whole stack.
    Forward: predicted and target as one batch of 2N (a conv launch reads its weights once).  Saved for backward, only when predicted
    needs a gradient: the post-ReLU map of every conv up to the deepest tap (it is the ReLU mask, the pool's argmax and the tap's sign
    at once).  Backward: per conv, deepest first, ops.feature_grad_assemble then ops.conv2d_bwd_data on the predicted half, ending in
    ops.conv2d_stem_bwd_data; the incoming gradient is folded into the tap coefficients on the device."""

    @staticmethod
    def _walk(owner, x, keep_all: bool):
        """the forward chain on x [2N,3,H,W]: (tap maps, post-ReLU map of every conv when keep_all)"""
        layers = list(owner.vgg19.children())
        taps, maps = [], []
        cur = x
        for i in range(owner._last_tap + 1):
            m = layers[i]
            if i == 0:
                cur = ops.conv2d_stem(cur, m.weight, m.bias, relu=True, pool=False, want_range=True)
            elif i in VGG19_CONVS:
                cur = ops.conv2d(cur, conv2d_packs(m, need_dx=False)[0], relu=True, want_range=True)
            elif i in VGG19_POOLS:
                cur = ops.maxpool2(cur, want_range=True)
            # (a ReLU: fused into the conv before it)
            if i in VGG19_CONVS and keep_all:
                maps.append(cur)
            if i in owner.taps:
                taps.append(cur)
        return taps, maps

    @staticmethod
    @_fwd
    def forward(ctx, predicted, target, owner):
        need = ctx.needs_input_grad[0]
        x = torch.cat([predicted, target]).contiguous()
        taps, maps = VGG19FeatureLossFn._walk(owner, x, need)
        parts = torch.empty(len(taps), dtype=torch.float32, device=x.device)
        counts = []
        for k, f in enumerate(taps):
            count = f.numel() // 2
            counts.append(float(count) if owner.reduction == "mean" else 1.0)
            ops.feature_l1(f, 1.0 / counts[-1], out=parts[k:k + 1])
        ctx.owner = owner
        if need:
            ctx.counts = torch.tensor(counts, dtype=torch.float64, device=x.device)
            ctx.save_for_backward(*maps)
        return parts.double().sum().float()   # (five fp32 values: their fp64 sum is exact for all practical magnitudes, so this rounds once)

    @staticmethod
    @once_differentiable  # no double backward (the reference's losses need none): asking for one raises instead of returning zeros
    @_bwd
    def backward(ctx, dloss):
        owner, maps = ctx.owner, ctx.saved_tensors
        layers = list(owner.vgg19.children())
        convs = [i for i in VGG19_CONVS if i <= owner._last_tap]
        coeffs = (dloss.reshape(1).double() / ctx.counts).float()   # d loss / d (sum |p - t|) of every tap, on the device
        tap_of = {t: k for k, t in enumerate(sorted(owner.taps))}
        upstream = None
        for k in range(len(convs) - 1, -1, -1):
            i = convs[k]
            j = tap_of.get(i + 1)
            g, scale = ops.feature_grad_assemble(maps[k], upstream, None if j is None else coeffs[j:j + 1])
            if i == 0:
                return ops.conv2d_stem_bwd_data(g, layers[0].weight), None, None
            upstream = ops.conv2d_bwd_data(g, conv2d_packs(layers[i], need_dx=True)[1], scale)
        raise AssertionError("unreachable: layer 0 is a conv")


class VGG19FeatureLoss(nn.Module):
    """loss(predicted, target) = sum over taps of mean |f_k(predicted) - f_k(target)|, f_k = vgg19[0 : tap_k + 1]: the reference's
    compute_perceptual_loss(vgg19, [1, 6, 11, 20, 29], ...) (model.py:1990-2017).  `self.vgg19` has torchvision's layout, so
    `loss.vgg19.load_state_dict(perceptual.vgg19.state_dict())` works; the constructor freezes its parameters.
    reduction="sum": the plain sum of |p - t| per tap.  normalize=True: the reference's normalize_input (model.py:2019-2022) first.
    fp32 CUDA inputs with frozen fp32 weights run on the HIP kernels (one VGG19FeatureLossFn node); anything else — CPU tensors, half
    modules, a weight that requires grad, widths off a multiple of 32, an image below 16 x 16, native(False) — is forward_reference."""

    def __init__(self, widths: Sequence[int] = (64, 128, 256, 512, 512), taps: Sequence[int] = (1, 6, 11, 20, 29), reduction: str = "mean",
                 normalize: bool = False):
        super().__init__()
        if len(widths) != 5:
            raise ValueError(f"VGG19FeatureLoss: five widths, got {tuple(widths)}")
        layers: List[nn.Module] = []
        ci = 3
        for b, (co, n) in enumerate(zip(widths, _BLOCKS)):
            if b:
                layers.append(nn.MaxPool2d(2, 2))
            for _ in range(n):
                layers += [nn.Conv2d(ci, int(co), 3, padding=1), nn.ReLU(inplace=True)]
                ci = int(co)
        self.vgg19 = nn.Sequential(*layers)
        self.vgg19.requires_grad_(False)
        self._setup(taps, reduction, normalize)

    @classmethod
    def from_sequential(cls, seq, taps: Sequence[int] = (1, 6, 11, 20, 29), reduction: str = "mean", normalize: bool = False):
        """Wraps an existing Sequential (the reference's `perceptual.vgg19`): its modules and Parameters are shared, not copied, and
        their requires_grad is left as it is (weights that require grad take forward_reference)."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.vgg19 = seq
        self._setup(taps, reduction, normalize)
        return self

    def _setup(self, taps, reduction, normalize):
        _check_layout(self.vgg19)
        taps = tuple(int(t) for t in taps)
        if not taps or len(set(taps)) != len(taps) or any(t - 1 not in VGG19_CONVS for t in taps):
            raise ValueError(f"VGG19FeatureLoss: taps must be distinct ReLU layers {tuple(c + 1 for c in VGG19_CONVS)}, got {taps}")
        if reduction not in ("mean", "sum"):
            raise ValueError(f"VGG19FeatureLoss: reduction = {reduction!r} (\"mean\" or \"sum\")")
        self.taps, self.reduction, self.normalize = taps, reduction, bool(normalize)
        self._last_tap = max(taps)
        self._native = True
        self.register_buffer("_mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), persistent=False)
        self.register_buffer("_std", torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1), persistent=False)

    def native(self, enabled: bool = True) -> "VGG19FeatureLoss":
        """native(False): every call takes forward_reference."""
        self._native = bool(enabled)
        return self

    def _convs(self):
        layers = list(self.vgg19.children())
        return [layers[i] for i in VGG19_CONVS]

    def native_ok(self, predicted: torch.Tensor, target: torch.Tensor) -> bool:
        """Do the HIP kernels take this call (the rules of the class docstring)?"""
        if not self._native or not (isinstance(predicted, torch.Tensor) and isinstance(target, torch.Tensor)):
            return False
        if not (predicted.is_cuda and target.is_cuda and predicted.device == target.device and predicted.is_floating_point()
                and target.is_floating_point() and predicted.dim() == 4 and predicted.shape == target.shape and predicted.shape[1] == 3):
            return False
        n, _, h, w = predicted.shape
        if n < 1 or h < 16 or w < 16:
            return False
        widest = 3
        for conv in self._convs():
            wt, b = conv.weight, conv.bias
            if (wt.dtype != torch.float32 or b.dtype != torch.float32 or wt.device != predicted.device or b.device != predicted.device
                    or wt.requires_grad or b.requires_grad or wt.shape[0] % 32):
                return False
            widest = max(widest, int(wt.shape[0]))
        return 2 * n * widest * h * w < 2 ** 31

    def _normalized(self, x: torch.Tensor) -> torch.Tensor:
        return (x - self._mean.to(x.dtype)) / self._std.to(x.dtype) if self.normalize else x

    def forward_reference(self, predicted: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """The same expression in plain PyTorch (model.py:1990-2017 with detach=False)."""
        p, t = self._normalized(predicted), self._normalized(target)
        loss = 0.0
        for i, layer in enumerate(self.vgg19.children()):
            p, t = layer(p), layer(t)
            if i in self.taps:
                d = torch.abs(p - t)
                loss = loss + (torch.mean(d) if self.reduction == "mean" else torch.sum(d))
            if i == self._last_tap:
                break
        return loss

    def forward(self, predicted: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not self.native_ok(predicted, target):
            return self.forward_reference(predicted, target)
        if target.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("VGG19FeatureLoss: target requires grad; the native path differentiates the predicted image only "
                               "(detach the target, or call native(False))")
        return VGG19FeatureLossFn.apply(self._normalized(predicted.float()), self._normalized(target.float()), self)

    @torch.no_grad()
    def features(self, predicted: torch.Tensor, target: torch.Tensor) -> List[torch.Tensor]:
        """The tap maps of the native path, each [2N, C, H, W]: predicted first, then target (for tests and measurements)."""
        if not self.native_ok(predicted, target):
            raise RuntimeError("VGG19FeatureLoss.features: the HIP kernels do not take this call (see native_ok)")
        x = torch.cat([self._normalized(predicted), self._normalized(target)]).float().contiguous()
        return VGG19FeatureLossFn._walk(self, x, False)[0]
