"""Host-side mirror of the reference's hot-path modules (johndpope/MegaPortrait-hack model.py).

Same class names, constructor signatures, parameter names/shapes (=> identical state-dict keys,
SURVEY.md Appendix C) and forward signatures as the reference, so its callers
(`train.py:194,283`, `inference.py:35`, `PairwiseTransferLoss` model.py:2192-2214) drop in; the
arithmetic runs in libmphip.so (hand-written HIP for gfx950) through the C ABI.  nn.Conv3d /
nn.GroupNorm objects are kept purely as parameter containers (names, shapes, default init,
.to()/.state_dict()); their own forward is never called.

Training: every module here is differentiable — under autograd the same HIP ops run as
torch.autograd Functions (autograd.py) whose backward kernels live in csrc/backward.hip, csrc/conv3d_bwd_f16x3.hip
and csrc/warp.hip (K9/K10); under torch.no_grad() the fused inference path runs.
"""
from __future__ import annotations

import logging
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import autograd as ag
from . import ops

COMPRESS_DIM = 512  # model.py:48
_C2D_EARLY = os.environ.get("MPHIP_C2D_EARLY", "0") == "1"  # dev switch, see GbaseHotSlice._run


def _f32(*tensors):
    """Inputs arrive in fp16/bf16 when an upstream PyTorch module ran under autocast (train.py:188): the HIP path
    computes in fp32, like the reference's fp32 parameters do outside autocast."""
    out = tuple(t.float() if isinstance(t, torch.Tensor) and t.is_floating_point() and t.dtype != torch.float32 else t
                for t in tensors)
    return out[0] if len(out) == 1 else out


def _autocast_policy(fn):
    """The reference runs its generator step under torch.cuda.amp.autocast() (train.py:145,188): conv3d then multiplies f16 operands
    with fp32 accumulation.  Inside such a region the F(2,3) conv launches of the wrapped forward do the same (ops.half_products); outside
    it — inference.py, the graded fp32 configurations — nothing changes.  Inputs are still promoted to fp32 at the boundary (_f32): the
    policy is about the conv arithmetic, activations stay fp32 between kernels."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        if not ops.autocast_half():
            return fn(*args, **kwargs)
        with ops.half_products(True):
            return fn(*args, **kwargs)

    return wrapped


# ------------------------------------------------------------------ model dtypes (INTEGRATION.md "Model dtypes")
# A hot module's model dtype is the dtype of its floating-point parameters.  A .half() / .bfloat16() module runs as its "fp32 twin": a
# copy whose parameters are fp32 shadows of the half ones (exact), under the single-product conv policy (ops.half_products), with the
# boundary tensors typed — inputs are read in their own dtype (K2, ops.cast_to_f32_range), outputs written in the model dtype (K3,
# ops.cast_from_f32).  Activations between kernels stay fp32.  The output is therefore bitwise the twin's fp32 output rounded once.
_HALF = (torch.float16, torch.bfloat16)
_dtype_generation = 0   # bumped by every dtype / device conversion of a hot module (_ModelDtype._apply): invalidates cached model dtypes
_TRAIN_HALF_MSG = ("{}: training a module whose parameters are {} is not supported — keep fp32 parameters and use torch.autocast "
                   "(the HIP path then runs the same single-product convs)")


class _ModelDtype:
    """Mixin of the hot modules: `.half()`, `.bfloat16()`, `.float()`, `.to()` reach every submodule's `_apply`; each call invalidates
    the cached model dtypes (recomputed on the next forward: the per-call check costs one dict lookup) and drops the fp32 twins of the
    converted modules (a module converted back to fp32 holds no dead copy; a half one builds its twin again on its next forward)."""

    def _apply(self, fn, *args, **kwargs):
        global _dtype_generation
        _dtype_generation += 1
        out = super()._apply(fn, *args, **kwargs)
        for m in self.modules():
            for k in _TWIN_SLOTS:
                m.__dict__.pop(k, None)
        return out


def model_dtype(module: nn.Module) -> torch.dtype:
    """The dtype of the module's floating-point parameters: float32, float16 or bfloat16.  Mixed dtypes raise RuntimeError."""
    hit = module.__dict__.get("_mphip_dtype")
    if hit is not None and hit[0] == _dtype_generation:
        return hit[1]
    dts = {p.dtype for p in module.parameters() if p.is_floating_point()}
    if len(dts) > 1:
        raise RuntimeError(f"{type(module).__name__}: parameters mix dtypes ({', '.join(sorted(str(d) for d in dts))}); a hot module runs in "
                           "ONE model dtype — convert it as a whole with .float(), .half() or .bfloat16()")
    dt = dts.pop() if dts else torch.float32
    if dt not in (torch.float32,) + _HALF:
        raise RuntimeError(f"{type(module).__name__}: parameters are {dt}; the HIP path runs float32, float16 or bfloat16 models")
    module.__dict__["_mphip_dtype"] = (_dtype_generation, dt)
    return dt


# per-module caches (packs, derived weights, plans, streams, ...): a twin starts without them
_TWIN_SLOTS = ("_mphip_twin", "_mphip_tail_twin")
_CACHE_ATTRS = ("_mphip_pack", "_mphip_bwd_pack", "_w_kn", "_w_head", "_fused", "_plans", "_side_streams", "_mphip_dtype") + _TWIN_SLOTS


def _fp32_copy(module: nn.Module) -> nn.Module:
    """Deep copy with every floating-point parameter / buffer as an fp32 tensor (no gradient) and the caches left behind."""
    import copy

    memo = {}
    for m in module.modules():
        for k in _CACHE_ATTRS:
            v = m.__dict__.get(k)
            if v is not None:
                memo[id(v)] = {} if isinstance(v, dict) else None
        for p in m._parameters.values():
            if p is not None:
                memo[id(p)] = nn.Parameter(p.detach().float() if p.is_floating_point() else p.detach().clone(), requires_grad=False)
        for b in m._buffers.values():
            if b is not None:
                memo[id(b)] = b.detach().float() if b.is_floating_point() else b.detach().clone()
    return copy.deepcopy(module, memo)


def _twin_key(pairs):
    return (ops.weight_epoch(),) + tuple((p.data_ptr(), p._version) for p, _ in pairs)


def _twin(module: nn.Module, build=None, slot: str = "_mphip_twin") -> nn.Module:
    """The module's fp32 twin, kept in step with the half parameters: a parameter that changed (in-place update, load_state_dict) is
    copied into its shadow, whose new version makes every cache of the twin (packs, plans) rebuild as it would for an fp32 module.
    The twin is built anew when there is none (a conversion of the module drops it: _ModelDtype._apply), after ops.invalidate_packs()
    (a Parameter object may have been replaced) and when a parameter changed device.  Whenever a twin is built or a parameter moved,
    the model dtype is checked afresh, uncached: a sub-module converted on its own (`.G3d.final_conv.float()`) never runs mixed."""
    src = module.__dict__.get(slot)
    if src is not None:
        twin, pairs, key = src
        now = _twin_key(pairs)
        if now == key:
            return twin
        module.__dict__.pop("_mphip_dtype", None)
        model_dtype(module)
        if now[0] == key[0] and all(p.device == q.device for p, q in pairs):
            with torch.no_grad():
                for (p, q), k_old, k_new in zip(pairs, key[1:], now[1:]):
                    if k_old != k_new:
                        q.copy_(p)
            module.__dict__[slot] = (twin, pairs, now)
            return twin
    module.__dict__.pop(slot, None)
    module.__dict__.pop("_mphip_dtype", None)
    model_dtype(module)
    if build is not None:
        twin, pairs = build()   # (twin, [(half parameter, its fp32 shadow), ...])
    else:
        twin = _fp32_copy(module)
        pairs = list(zip(module.parameters(), twin.parameters()))
    module.__dict__[slot] = (twin, pairs, _twin_key(pairs))
    return twin


def _refuse_half_training(module, dt, *tensors):
    if ag.needs_grad(module, *tensors):
        raise RuntimeError(_TRAIN_HALF_MSG.format(type(module).__name__, dt))


def _model_dtype_forward(cast_input: bool = False, volume_input: bool = False):
    """Decorator of a hot module's public forward: fp32 modules run it unchanged; a half module runs its fp32 twin's (see above) and
    returns the model dtype.  cast_input: the first argument feeds an f16x3 conv stack — a half input is widened together with its range
    descriptor in one pass (ops.cast_to_f32_range).  volume_input: a 4-D first argument is Eapp's [B,1536,H,W] map, viewed as the
    [B,96,16,H,W] volume before the cast (the descriptor rides on the tensor the stack reads)."""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrapped(self, *args, **kwargs):
            dt = model_dtype(self)
            if dt == torch.float32:
                return fn(self, *args, **kwargs)
            _refuse_half_training(self, dt, *args, *kwargs.values())
            twin = _twin(self, getattr(self, "_twin_build", None))
            if cast_input and args and isinstance(args[0], torch.Tensor) and args[0].dtype in _HALF:
                x = args[0]
                if volume_input and x.dim() == 4:
                    x = x.reshape(x.size(0), 96, 16, *x.shape[2:])
                args = (ops.cast_to_f32_range(x),) + args[1:]
            with ops.half_products(True):
                y = fn(twin, *args, **kwargs)   # (this class's forward on the twin, also when a subclass calls it: encoders2d.G2d)
            return ops.cast_from_f32(y, dt)

        return wrapped

    return deco


class _PackCache:
    """Packed conv weights, rebuilt when the parameter changes (in-place update, load_state_dict or .to()).
    The pack lives ON the conv module (not in a global table keyed by id()), so it dies with the module and
    can never be mistaken for another module's weights after id / address reuse."""

    @staticmethod
    def get(conv: nn.Module) -> ops.PackedConv:
        w, b = conv.weight, conv.bias
        key = ops._pack_cache_key(conv, "_mphip_pack")   # (data_ptr, _version, shape of the weight; the bias; device; epoch)
        hit = conv.__dict__.get("_mphip_pack")
        if not ops.pack_is_current(hit, key):
            hit = (key, ops.PackedConv(w, b))
            conv.__dict__["_mphip_pack"] = hit
        return hit[1]


_packs = _PackCache()


def compute_rt_warp(rotation, translation, invert=False, grid_size=64):
    """model.py:777-809 — rigid warp grid [B,3,G,G,G] (x,y,z channels)."""
    rotation, translation = _f32(rotation, translation)
    zero_em = torch.zeros((rotation.shape[0], 3, 1, 1, 1), dtype=torch.float32, device=rotation.device)
    if torch.is_grad_enabled() and (rotation.requires_grad or translation.requires_grad):
        # un-swapped reference code that calls this under autograd (the reference's own WarpGenerator*.forward, model.py:965,
        # 1016, when only integration.patch_functions ran): rt + resize(0) == rt exactly, with the gradient to R and t
        theta = ag.RtThetaFn.apply(rotation, translation, bool(invert))
        return ag.WarpFieldComposeFn.apply(theta, zero_em, grid_size)
    theta = ops.rt_theta(rotation, translation, invert)
    _, rt, _ = ops.warp_field_compose(theta, zero_em, grid_size, parts=True)
    return rt


def apply_warping_field(v, warp_field):
    """model.py:1028-1065 — same signature and result; one fused HIP kernel (K2); differentiable (autograd.WarpVolumeFn)."""
    v, warp_field = _f32(v, warp_field)
    if torch.is_grad_enabled() and (v.requires_grad or warp_field.requires_grad):
        return ag.WarpVolumeFn.apply(v, warp_field, False)
    return ops.warp_volume(v, warp_field)


def _upsample_trilinear(x, scale_factors):
    """F.interpolate(x, scale_factor=scale_factors, mode='trilinear', align_corners=False) on the HIP kernels."""
    if tuple(float(v) for v in scale_factors) == (1.0, 1.0, 1.0):
        return x
    if torch.is_grad_enabled() and x.requires_grad:
        return ag.UpsampleTrilinearFn.apply(x, tuple(scale_factors))
    return ops.upsample_trilinear(x, scale_factors)


class AdaptiveGroupNorm(nn.Module):
    """model.py:304-316."""

    def __init__(self, num_channels, num_groups=32):
        super().__init__()
        self.num_channels = num_channels
        self.num_groups = num_groups
        self.weight = nn.Parameter(torch.ones(1, num_channels, 1, 1, 1))
        self.bias = nn.Parameter(torch.zeros(1, num_channels, 1, 1, 1))
        self.group_norm = nn.GroupNorm(num_groups, num_channels)

    def forward(self, x):
        x = _f32(x)
        if ag.needs_grad(self, x):
            return ag.adaptive_groupnorm(x, self)
        st = ops.groupnorm_stats(x, self.num_groups, self.group_norm.eps)
        return ops.groupnorm_apply(x, st, self.group_norm.weight, self.group_norm.bias, self.num_groups,
                                   w2=self.weight, b2=self.bias)


class ResBlock3D_Adaptive(nn.Module):
    """model.py:369-408 (the `upsample` flag is never set on the hot path; kept for signature parity)."""

    def __init__(self, in_channels, out_channels, upsample=False, scale_factors=(1, 1, 1)):
        super().__init__()
        self.upsample = upsample
        self.scale_factors = scale_factors
        self.conv1 = nn.Conv3d(in_channels, out_channels, 3, padding=1)
        self.conv2 = nn.Conv3d(out_channels, out_channels, 3, padding=1)
        self.norm1 = AdaptiveGroupNorm(out_channels)
        self.norm2 = AdaptiveGroupNorm(out_channels)
        if in_channels != out_channels:
            self.residual_conv = nn.Conv3d(in_channels, out_channels, 1)
        else:
            self.residual_conv = nn.Identity()

    def forward(self, x, _up=(1, 1, 1)):
        """`_up`: nearest-upsample factors fused into the block's last elementwise pass (FlowField's nn.Upsample)."""
        out = self._forward(x, _up)
        if self.upsample:   # model.py:404-405 (no module of Gbase sets the flag): trilinear, align_corners=False
            out = _upsample_trilinear(out, self.scale_factors)
        return out

    def _forward(self, x, _up=(1, 1, 1)):
        x = _f32(x)
        if ag.needs_grad(self, x):  # differentiable path: the same ops, unfused, as autograd Functions (autograd.py)
            y = ag.conv3d(x, self.conv1, _packs.get(self.conv1))
            y = ag.adaptive_groupnorm(y, self.norm1, relu=True)
            y = ag.conv3d(y, self.conv2, _packs.get(self.conv2))
            res = x if isinstance(self.residual_conv, nn.Identity) else ag.conv3d(x, self.residual_conv, _packs.get(self.residual_conv))
            y = ag.adaptive_groupnorm(y, self.norm2, residual=res, relu=True)
            return y if tuple(_up) == (1, 1, 1) else ag.UpsampleNearestFn.apply(y, tuple(_up))
        n1, n2 = self.norm1, self.norm2
        res_conv = None if isinstance(self.residual_conv, nn.Identity) else self.residual_conv
        if res_conv is not None and ops.flowfield_conv_gn_ok(tuple(x.shape), self.conv1) and \
                ops.flowfield_conv_gn_ok(tuple(x.shape[:1]) + (self.conv2.weight.shape[1],) + tuple(x.shape[2:]), self.conv2, res_conv):
            # FlowField's four levels: each half of the block is ONE launch (csrc/flowfield.hip)
            a = ops.flowfield_conv_gn(x, self.conv1, n1, relu=True)
            return ops.flowfield_conv_gn(a, self.conv2, n2, res_x=x, res_conv=res_conv, relu=True, up=_up)
        # split-K slabs are summed by the GN kernels below; a direct launch carries the norm's statistics along
        y = ops.conv3d_split(x, _packs.get(self.conv1), gn_groups=n1.num_groups, gn_eps=n1.group_norm.eps)
        tiny = ops.groupnorm_fused_ok(y, n1.num_groups)  # FlowField: statistics + apply in one launch
        if tiny:
            a = ops.groupnorm_small(y, n1.group_norm.weight, n1.group_norm.bias, n1.num_groups, n1.group_norm.eps,
                                    w2=n1.weight, b2=n1.bias, relu=True)
            y = ops.conv3d_split(a, _packs.get(self.conv2))
        else:
            st = ops.groupnorm_stats(y, n1.num_groups, n1.group_norm.eps)
            pc2 = _packs.get(self.conv2)
            if y.splits == 1 and ops.gn_in_conv_ok(y.shape, pc2):  # Eapp's 3D tail: AGN1 + ReLU inside conv2's staging
                y2, st2 = ops.conv3d_gn_in(y.data, st, n1.group_norm.weight, n1.group_norm.bias, n1.num_groups, pc2,
                                           w2=n1.weight, b2=n1.bias, out_gn_groups=n2.num_groups, out_gn_eps=n2.group_norm.eps)
                y = ops.ConvOut(y2, 1, None, y.shape, st2, n2.num_groups)
            else:
                a = ops.groupnorm_apply(y, st, n1.group_norm.weight, n1.group_norm.bias, n1.num_groups, w2=n1.weight,
                                        b2=n1.bias, relu=True)
                y = ops.conv3d_split(a, pc2, gn_groups=n2.num_groups, gn_eps=n2.group_norm.eps)
        res = x if isinstance(self.residual_conv, nn.Identity) else ops.conv3d_split(x, _packs.get(self.residual_conv))
        if tiny:
            return ops.groupnorm_small(y, n2.group_norm.weight, n2.group_norm.bias, n2.num_groups, n2.group_norm.eps,
                                       w2=n2.weight, b2=n2.bias, residual=res, relu=True, up=_up)
        st = ops.groupnorm_stats(y, n2.num_groups, n2.group_norm.eps)
        return ops.groupnorm_apply(y, st, n2.group_norm.weight, n2.group_norm.bias, n2.num_groups, w2=n2.weight,
                                   b2=n2.bias, residual=res, relu=True, up=_up)


class FlowField(_ModelDtype, nn.Module):
    """model.py:415-471: [B,512,1,1] -> [B,3,16,16,16] in [0,1)."""

    _UPS = ((2, 2, 2), (2, 2, 2), (1, 2, 2), (1, 2, 2))

    def __init__(self):
        super().__init__()
        self.conv1x1 = nn.Conv2d(512, 2048, kernel_size=1)
        self.resblock1 = ResBlock3D_Adaptive(in_channels=512, out_channels=256)
        self.upsample1 = nn.Upsample(scale_factor=(2, 2, 2))
        self.resblock2 = ResBlock3D_Adaptive(in_channels=256, out_channels=128)
        self.upsample2 = nn.Upsample(scale_factor=(2, 2, 2))
        self.resblock3 = ResBlock3D_Adaptive(in_channels=128, out_channels=64)
        self.upsample3 = nn.Upsample(scale_factor=(1, 2, 2))
        self.resblock4 = ResBlock3D_Adaptive(in_channels=64, out_channels=32)
        self.upsample4 = nn.Upsample(scale_factor=(1, 2, 2))
        self.conv3x3x3 = nn.Conv3d(32, 3, kernel_size=3, padding=1)
        self.gn = nn.GroupNorm(1, 3)
        self.tanh = nn.Tanh()

    def _conv1x1_kn(self):
        """conv1x1.weight [2048,512,1,1] re-laid as [K=512][N=2048] (N contiguous) for the coalesced matmul kernel;
        rebuilt when the parameter changes."""
        w = self.conv1x1.weight
        key = (w.data_ptr(), w._version, str(w.device), ops.weight_epoch())
        hit = self.__dict__.get("_w_kn")
        if hit is None or hit[0] != key or ops.repacking():
            hit = (key, w.detach().reshape(2048, 512).t().contiguous())
            self.__dict__["_w_kn"] = hit
        return hit[1]

    def _head_kn(self, gamma):
        """(z+e) @ Gamma followed by the 1x1 conv on the 1x1 map (model.py:945-957 -> 446) is one linear map of (z+e):
        Gamma @ W^T, [512][2048], built once per weight version — one dense product per step instead of two dependent ones
        at the head of the latency-bound generator chain."""
        w = self.conv1x1.weight
        key = (w.data_ptr(), w._version, gamma.data_ptr(), gamma._version, str(w.device), ops.weight_epoch())
        hit = self.__dict__.get("_w_head")
        if hit is None or hit[0] != key or ops.repacking():
            hit = (key, ops.small_gemm(gamma.detach(), self._conv1x1_kn()))
            self.__dict__["_w_head"] = hit
        return hit[1]

    @_model_dtype_forward()
    def forward_from_codes(self, z, e, gamma):
        """Inference entry used by the warp generators: FlowField((z+e) @ Gamma) with the two dense products merged."""
        z, e = _f32(z, e)
        b = z.shape[0]
        x = ops.add_matmul(z.reshape(b, 512), e.reshape(b, 512), self._head_kn(gamma), self.conv1x1.bias)
        return self._tail(x.view(b, 512, 4, 1, 1), False)

    @_model_dtype_forward()
    def forward(self, zs, adaptive_gamma=0, adaptive_beta=0):  # last two ignored, as in the reference
        zs = _f32(zs)
        train = ag.needs_grad(self, zs)
        b = zs.shape[0]
        s = zs.reshape(b, 512)
        if train:
            x = ag.Conv1x1OnVectorFn.apply(s, self.conv1x1.weight, self.conv1x1.bias, self._conv1x1_kn())
        else:
            x = ops.add_matmul(s, None, self._conv1x1_kn(), self.conv1x1.bias)  # 1x1 conv on a 1x1 map == s @ W^T + b
        return self._tail(x.view(b, 512, 4, 1, 1), train)  # model.py:425: channel c*4+d -> (c,d)

    def _tail(self, x, train):
        for blk, up in zip((self.resblock1, self.resblock2, self.resblock3, self.resblock4), self._UPS):
            x = blk(x, _up=up)  # nn.Upsample (nearest, model.py:450-457) fused into the block's last pass
        if train:
            x = ag.conv3d(x, self.conv3x3x3, _packs.get(self.conv3x3x3))
            x = ag.groupnorm(x, self.gn, relu=True, tanh=True)
            assert x.shape[1] == 3, f"Expected 3 channels after conv3x3x3, got {x.shape[1]}"
            return x
        if ops.flowfield_out_ok(tuple(x.shape), self.conv3x3x3) and self.gn.num_groups == 1:
            return ops.flowfield_out(x, self.conv3x3x3, self.gn)   # direct 3-channel conv + one normalising pass (csrc/flowfield.hip)
        x = ops.conv3d_split(x, _packs.get(self.conv3x3x3))
        if ops.groupnorm_fused_ok(x, 1):
            x = ops.groupnorm_small(x, self.gn.weight, self.gn.bias, 1, self.gn.eps, relu=True, tanh=True)
        else:
            st = ops.groupnorm_stats(x, 1, self.gn.eps)
            x = ops.groupnorm_apply(x, st, self.gn.weight, self.gn.bias, 1, relu=True, tanh=True)
        assert x.shape[1] == 3, f"Expected 3 channels after conv3x3x3, got {x.shape[1]}"
        return x


class _WarpGenerator(_ModelDtype, nn.Module):
    _INVERT = False

    def __init__(self, num_channels):
        super().__init__()
        self.flowfield = FlowField()
        self.num_channels = COMPRESS_DIM
        # Registered parameters on every device (the reference's `nn.Parameter(...).to(device)` only
        # registers them on CPU hosts, model.py:934-935; load_gbase_state_dict() accepts both layouts).
        self.adaptive_matrix_gamma = nn.Parameter(torch.randn(self.num_channels, self.num_channels))
        self.adaptive_matrix_beta = nn.Parameter(torch.randn(self.num_channels, self.num_channels))

    @_model_dtype_forward()
    def forward(self, R, t, z, e):
        assert R.shape == (z.shape[0], 3), f"Expected R shape (batch_size, 3), got {R.shape}"
        assert t.shape == (z.shape[0], 3), f"Expected t shape (batch_size, 3), got {t.shape}"
        assert z.shape == e.shape, f"Expected z and e to have the same shape, got {z.shape} and {e.shape}"
        R, t, z, e = _f32(R, t, z, e)
        if ag.needs_grad(self, R, t, z, e):
            s = ag.AddMatmulFn.apply(z, e, self.adaptive_matrix_gamma)
            em = self.flowfield(s.unsqueeze(-1).unsqueeze(-1), 0, 0)
            theta = ag.RtThetaFn.apply(R, t, self._INVERT)
            return ag.WarpFieldComposeFn.apply(theta, em, 64)
        em = self.flowfield.forward_from_codes(z, e, self.adaptive_matrix_gamma)  # FlowField((z+e) @ Gamma), model.py:945-957
        theta = ops.rt_theta(R, t, self._INVERT)
        return ops.warp_field_compose(theta, em, 64)


class WarpGeneratorS2C(_WarpGenerator):
    """model.py:927-975 (rigid part inverted)."""
    _INVERT = True


class WarpGeneratorC2D(_WarpGenerator):
    """model.py:978-1024."""
    _INVERT = False


class ResBlock3D(nn.Module):
    """model.py:500-528."""

    def __init__(self, in_channels, out_channels, upsample=False, scale_factors=(1, 1, 1)):
        super().__init__()
        self.upsample = upsample
        self.scale_factors = scale_factors
        self.conv1 = nn.Conv3d(in_channels, out_channels, kernel_size=3, padding=1)
        self.gn1 = nn.GroupNorm(num_groups=32, num_channels=out_channels)
        self.conv2 = nn.Conv3d(out_channels, out_channels, kernel_size=3, padding=1)
        self.gn2 = nn.GroupNorm(num_groups=32, num_channels=out_channels)
        self.shortcut = nn.Conv3d(in_channels, out_channels, kernel_size=1) if in_channels != out_channels else nn.Identity()

    def _forward_train(self, x):
        """Differentiable path (scope row f2): the same ops, unfused, as torch.autograd Functions whose forward and
        backward both run in libmphip.so (autograd.py)."""
        identity = x if isinstance(self.shortcut, nn.Identity) else ag.conv3d(x, self.shortcut, _packs.get(self.shortcut))
        y = ag.conv3d(x, self.conv1, _packs.get(self.conv1))
        y = ag.groupnorm(y, self.gn1, relu=True)
        y = ag.conv3d(y, self.conv2, _packs.get(self.conv2))
        return ag.groupnorm(y, self.gn2, residual=identity, relu=True)

    def forward(self, x, _pool_after: bool = False, _after_conv1=None):
        """`_after_conv1`: host-side hook called right after conv1 has been launched (GbaseHotSlice issues the side-stream
        generator there, once the GPU has a long kernel queued)."""
        out = self._forward(x, _pool_after, _after_conv1)
        if self.upsample:   # model.py:525-526 (G3d never sets the flag): trilinear, align_corners=False
            out = _upsample_trilinear(out, self.scale_factors)
        return out

    def _forward(self, x, _pool_after: bool = False, _after_conv1=None):
        x = _f32(x)
        if ag.needs_grad(self, x):
            y = self._forward_train(x)
            if _after_conv1 is not None:
                _after_conv1()
            return ag.AvgPool2Fn.apply(y) if _pool_after else y
        pc2 = _packs.get(self.conv2)
        psc = None if isinstance(self.shortcut, nn.Identity) else _packs.get(self.shortcut)
        # a conv shortcut that can finish the block (GN2, residual add, ReLU, pool in the k = 1 kernel's epilogue) is launched LAST
        finish = psc is not None and ops.shortcut_finish_ok(x.shape, psc, _packs.get(self.conv1), pc2, _pool_after)
        identity = x if psc is None else None if finish else ops.conv3d_split(x, psc)
        y = ops.conv3d_split(x, _packs.get(self.conv1), gn_groups=32, gn_eps=self.gn1.eps)  # + GN1's statistics
        if _after_conv1 is not None:
            _after_conv1()
        st = ops.groupnorm_stats(y, 32, self.gn1.eps)
        if y.splits == 1 and ops.gn_in_conv_ok(y.shape, pc2):
            # GN1 + ReLU folded into conv2's input staging: the normalised tensor never touches HBM
            y2, st2 = ops.conv3d_gn_in(y.data, st, self.gn1.weight, self.gn1.bias, 32, pc2, out_gn_groups=32,
                                       out_gn_eps=self.gn2.eps)
            y = ops.ConvOut(y2, 1, None, y.shape, st2, 32)
        else:
            a = ops.groupnorm_apply(y, st, self.gn1.weight, self.gn1.bias, 32, relu=True)
            y = ops.conv3d_split(a, pc2, gn_groups=32, gn_eps=self.gn2.eps)
        st = ops.groupnorm_stats(y, 32, self.gn2.eps)
        if finish:
            return ops.conv3d_k1_gn_res(x, psc, y.data, st, self.gn2.weight, self.gn2.bias, 32, relu=True, pool2=_pool_after)
        return ops.groupnorm_apply(y, st, self.gn2.weight, self.gn2.bias, 32, residual=identity, relu=True,
                                   pool2=_pool_after)


class G3d(_ModelDtype, nn.Module):
    """model.py:571-597.  nn.Sequential indices give the reference's state-dict names."""

    def __init__(self, in_channels):
        super().__init__()
        self.downsampling = nn.Sequential(
            ResBlock3D(in_channels, 96), nn.AvgPool3d(kernel_size=2, stride=2),
            ResBlock3D(96, 192), nn.AvgPool3d(kernel_size=2, stride=2),
            ResBlock3D(192, 384), nn.AvgPool3d(kernel_size=2, stride=2),
            ResBlock3D(384, 768),
        )
        self.upsampling = nn.Sequential(
            ResBlock3D(768, 384), nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True),
            ResBlock3D(384, 192), nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True),
            ResBlock3D(192, 96), nn.Upsample(scale_factor=2, mode="trilinear", align_corners=True),
        )
        self.final_conv = nn.Conv3d(96, 96, kernel_size=3, padding=1)

    @_model_dtype_forward(cast_input=True)
    @_autocast_policy
    def forward(self, x, _after_first_conv=None, _final_roi=None):
        """`_final_roi`: sample boxes of the warp that is the ONLY reader of the result (GbaseHotSlice under autograd): final_conv
        is evaluated on the tiles they touch, the rest of the returned tensor is uninitialised (ops.conv3d_roi)."""
        x = _f32(x)
        train = ag.needs_grad(self, x)
        up = ag.UpsampleTrilinear2Fn.apply if train else ops.upsample_trilinear2
        d = self.downsampling
        x = d[0](x, _pool_after=True, _after_conv1=_after_first_conv)   # AvgPool3d fused into the block's last elementwise pass (inference)
        x = d[2](x, _pool_after=True)
        x = d[4](x, _pool_after=True)
        x = d[6](x)
        u = self.upsampling
        x = up(u[0](x))
        x = up(u[2](x))
        x = up(u[4](x))
        if train:
            return ag.conv3d(x, self.final_conv, _packs.get(self.final_conv), roi=_final_roi)
        return ops.conv3d(x, _packs.get(self.final_conv))


class Eapp3DTail(_ModelDtype, nn.Module):
    """Scope row f1: the 3D tail of Eapp, model.py:217-226 + 271-290.  Attribute names are
    the reference Eapp's, so `appearanceEncoder.resblock3D_*` checkpoint keys load into this module directly.
    The reference assigns `resblock3D_96_2` twice (model.py:218,225): five blocks exist, one is applied twice."""

    _ORDER = ("resblock3D_96", "resblock3D_96_2", "resblock3D_96_1", "resblock3D_96_1_2", "resblock3D_96_2",
              "resblock3D_96_2_2")
    max_frames_per_pass = 64

    def __init__(self):
        super().__init__()
        self.resblock3D_96 = ResBlock3D_Adaptive(in_channels=96, out_channels=96)
        self.resblock3D_96_1 = ResBlock3D_Adaptive(in_channels=96, out_channels=96)
        self.resblock3D_96_1_2 = ResBlock3D_Adaptive(in_channels=96, out_channels=96)
        self.resblock3D_96_2 = ResBlock3D_Adaptive(in_channels=96, out_channels=96)
        self.resblock3D_96_2_2 = ResBlock3D_Adaptive(in_channels=96, out_channels=96)

    @_model_dtype_forward(cast_input=True, volume_input=True)
    @_autocast_policy
    def forward(self, out):
        """out: Eapp's conv_1 output [B,1536,H,W] (model.py:268) or the reshaped volume [B,96,16,H,W]."""
        out = _f32(out)
        vs = out.view(out.size(0), 96, 16, *out.shape[2:]) if out.dim() == 4 else out  # model.py:271
        if vs.shape[0] > self.max_frames_per_pass and not ag.needs_grad(self, vs):
            # (the conv kernels' 2 GiB buffer resource: see _HotSliceRunner.max_frames_per_pass; frames are independent)
            step = int(self.max_frames_per_pass)
            return torch.cat([self.forward(vs[i:i + step]) for i in range(0, vs.shape[0], step)], dim=0)
        for name in self._ORDER:
            vs = getattr(self, name)(vs)
        return vs


def eapp_tail(owner: nn.Module, vs):
    """Eapp3DTail's block sequence on the `resblock3D_*` blocks of `owner` (an Eapp that holds them itself, encoders2d.Eapp), in their
    model dtype: fp32 blocks run as they are; fp16 / bf16 blocks run as an fp32 twin, the input widened with its range descriptor in one
    pass and the output rounded once — what Eapp3DTail does for a half module."""
    blocks = {name: getattr(owner, name) for name in Eapp3DTail._ORDER}
    dts = {p.dtype for b in blocks.values() for p in b.parameters()}
    if dts == {torch.float32}:
        owner.__dict__.pop("_mphip_tail_twin", None)   # (converted back to fp32 by a parent that is not a hot module)
        for name in Eapp3DTail._ORDER:
            vs = blocks[name](vs)
        return vs
    if len(dts) > 1:
        raise RuntimeError(f"{type(owner).__name__}: the 3-D tail's parameters mix dtypes ({', '.join(sorted(str(d) for d in dts))}); convert "
                           "the module as a whole with .float(), .half() or .bfloat16()")
    dt = dts.pop()
    _refuse_half_training(nn.ModuleList(blocks.values()), dt, vs)

    def build():
        twin = Eapp3DTail.__new__(Eapp3DTail)
        nn.Module.__init__(twin)
        pairs = []
        for name in dict.fromkeys(Eapp3DTail._ORDER):
            setattr(twin, name, _fp32_copy(blocks[name]))
            pairs += list(zip(blocks[name].parameters(), getattr(twin, name).parameters()))
        return twin, pairs

    twin = _twin(owner, build, "_mphip_tail_twin")
    x = ops.cast_to_f32_range(vs) if vs.dtype in _HALF else vs
    with ops.half_products(True):
        y = twin(x)
    return ops.cast_from_f32(y, dt)


class G2dHead(_ModelDtype, nn.Module):
    """Scope row f3: the entry of G2d, model.py:718-719 + 756-757 — `reshape` Conv2d(96,1536,1)
    followed directly by `conv1x1` Conv2d(1536,512,1).  There is no nonlinearity between them, so at inference the two
    collapse into ONE 96->512 product (W = W2 @ W1, b = W2 @ b1 + b2): 19x fewer FLOPs and the 25 MB/frame 1536-channel
    intermediate never exists.  Attribute names are G2d's, so `G2d.reshape.*` / `G2d.conv1x1.*` checkpoint keys load
    here.  Under autograd the two convs run separately (their parameters get their own gradients)."""

    def __init__(self):
        super().__init__()
        self.reshape = nn.Conv2d(96, 1536, kernel_size=1)
        self.conv1x1 = nn.Conv2d(1536, 512, kernel_size=1)

    def _twin_build(self):
        """The fp32 twin of the head alone (a subclass such as encoders2d.G2d carries a PyTorch body the head never runs)."""
        twin = G2dHead.__new__(G2dHead)
        nn.Module.__init__(twin)
        pairs = []
        for name in ("reshape", "conv1x1"):
            setattr(twin, name, _fp32_copy(getattr(self, name)))
            pairs += list(zip(getattr(self, name).parameters(), getattr(twin, name).parameters()))
        return twin, pairs

    def _fused_pack(self) -> ops.PackedConv:
        ps = (self.reshape.weight, self.reshape.bias, self.conv1x1.weight, self.conv1x1.bias)
        key = tuple((p.data_ptr(), p._version) for p in ps) + (str(ps[0].device), ops.weight_epoch())
        hit = self.__dict__.get("_fused")
        if hit is None or hit[0] != key or ops.repacking():
            w1, b1, w2, b2 = (p.detach() for p in ps)
            w = ops.small_gemm(w2.reshape(512, 1536), w1.reshape(1536, 96))                       # [512, 96]
            b = ops.small_gemm(b1.reshape(1, 1536), w2.reshape(512, 1536), trans_b=True, bias=b2)  # [1, 512]
            hit = (key, ops.PackedConv(w.view(512, 96, 1, 1, 1), b.view(512)))
            self.__dict__["_fused"] = hit
        return hit[1]

    @_model_dtype_forward(cast_input=True)
    def forward(self, x):
        """x: the hot slice's output [B,96,H,W] (model.py:1171) -> [B,512,H,W], the input of G2d's ResBlock2D stack."""
        x = _f32(x)
        b, c, h, w = x.shape
        x5 = x.reshape(b, c, 1, h, w)
        if ag.needs_grad(self, x):
            y = ag.conv3d(x5, self.reshape, _packs.get(self.reshape))
            y = ag.conv3d(y, self.conv1x1, _packs.get(self.conv1x1))
        else:
            y = ops.conv3d(x5, self._fused_pack())
        return y.reshape(b, 512, h, w)


class G2dFinalConv(_ModelDtype, nn.Sequential):
    """G2d's exit, model.py:747-752 + 762: `final_conv` = GroupNorm(32,64) -> ReLU -> Conv2d(64,3,3,padding=1) -> Sigmoid on the
    [B,64,H,W] map (the largest activation of the generator), as two HIP launches that read the map twice and write the image
    (csrc/g2d_final.hip) instead of five to six passes of stock kernels.  The children are the reference's four modules at indices
    0-3 — parameter containers, their own forward is never called — so the state-dict keys are `0.weight, 0.bias, 2.weight, 2.bias`
    and every checkpoint loads unchanged.  Opt-in: encoders2d.G2d.native_final_conv() / gbase.Gbase.native_final_conv() /
    integration.install(g2d_final=True) swap it in; nothing uses it otherwise.

    A .half() / .bfloat16() instance reads and writes the half dtype directly (no fp32 copy of the map); its output is bitwise its fp32
    twin's on the widened input, rounded once.  An fp32 instance fed a half map returns fp32.  The kernels read NCHW: a channels_last
    map is copied to NCHW first."""

    def __init__(self):
        super().__init__(nn.GroupNorm(32, 64), nn.ReLU(inplace=True), nn.Conv2d(64, 3, 3, padding=1), nn.Sigmoid())

    @staticmethod
    def matches(seq) -> bool:
        """Is `seq` the reference's final_conv (four modules of the expected kinds and shapes)?"""
        if not isinstance(seq, nn.Sequential) or len(seq) != 4:
            return False
        gn, act, conv, sig = seq[0], seq[1], seq[2], seq[3]
        return (isinstance(gn, nn.GroupNorm) and gn.num_groups == 32 and gn.num_channels == 64 and gn.affine
                and isinstance(act, nn.ReLU) and isinstance(sig, nn.Sigmoid) and isinstance(conv, nn.Conv2d)
                and tuple(conv.weight.shape) == (3, 64, 3, 3) and conv.bias is not None and conv.stride == (1, 1)
                and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros")

    @classmethod
    def from_sequential(cls, seq: nn.Sequential) -> "G2dFinalConv":
        """A G2dFinalConv over `seq`'s own four modules: the SAME Parameter objects (an optimizer built earlier stays valid), the same
        eps, device, dtype and train/eval mode."""
        if not cls.matches(seq):
            raise TypeError("G2dFinalConv.from_sequential: expected nn.Sequential(GroupNorm(32, 64), ReLU, Conv2d(64, 3, 3, padding=1), "
                            f"Sigmoid), got {seq}")
        new = cls.__new__(cls)
        nn.Sequential.__init__(new, seq[0], seq[1], seq[2], seq[3])
        new.train(seq.training)
        return new

    def forward(self, x):
        gn, conv = self[0], self[2]
        dt = model_dtype(self)
        if dt != torch.float32:
            _refuse_half_training(self, dt, x)
            twin = _twin(self)
            gn, conv = twin[0], twin[2]
            return ops.g2d_final(x, gn.weight, gn.bias, conv.weight, conv.bias, gn.eps, out_dtype=dt)
        if ag.needs_grad(self, x):
            return ag.G2dFinal.apply(x, gn.weight, gn.bias, conv.weight, conv.bias, gn.eps)
        return ops.g2d_final(x, gn.weight, gn.bias, conv.weight, conv.bias, gn.eps, out_dtype=torch.float32)


def native_final_conv(g2d: nn.Module, enable: bool = True) -> bool:
    """Swaps `g2d.final_conv` (this package's G2d or the reference's, model.py:747-752) for a G2dFinalConv over the same modules, or
    back to the very nn.Sequential object it replaced.  Returns whether anything changed.  Off by default everywhere."""
    cur = getattr(g2d, "final_conv", None)
    if enable:
        if isinstance(cur, G2dFinalConv):
            return False
        new = G2dFinalConv.from_sequential(cur)
        new.__dict__["_replaced"] = cur   # (not a registered child: the module tree and the state-dict keys stay as they were)
        g2d.final_conv = new
        return True
    if not isinstance(cur, G2dFinalConv):
        return False
    old = cur.__dict__.pop("_replaced", None)
    g2d.final_conv = old if old is not None else nn.Sequential(*cur.children())
    return True


def fold_batchnorm(conv: nn.Module, bn: nn.Module, dtype: Optional[torch.dtype] = None):
    """Eval-mode `bn(conv(x))` as one conv: s = gamma / sqrt(running_var + eps), w' = w * s[:, None, None, None],
    b' = (b - running_mean) * s + beta, in the parameters' own dtype (fp32 on the native path) -> (w', b').  dtype: the parameters and
    running statistics are cast to it first (fp32 for a half block: the fold of its fp32 twin).  A conv without bias (torchvision's
    BasicBlock) folds as one with a zero bias."""
    w, g, beta, mean, var = (t.detach() if dtype is None else t.detach().to(dtype)
                             for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var))
    b = torch.zeros_like(mean) if conv.bias is None else conv.bias.detach() if dtype is None else conv.bias.detach().to(dtype)
    s = g / torch.sqrt(var + bn.eps)
    return (w * s[:, None, None, None]).contiguous(), ((b - mean) * s + beta).contiguous()


def _half_mode(block: nn.Module, x, dt: torch.dtype):
    """For a fused 2-D block built with half_precision=True: the dtype the one-product path writes for this call, or None when the call
    takes the block's other paths.  dt: the block's parameter dtype.
      - a .half() / .bfloat16() block fed a map of its own dtype: that dtype;
      - an fp32 block inside torch.autocast('cuda', float16): float16, what the original block returns there;
      - an fp32 block while the calling thread's ops.half_products policy is on: float32 (the twin the two contracts are stated with).
    bf16 autocast regions are left alone."""
    if not block.__dict__.get("_mphip_half") or not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.numel() > 0):
        return None
    if dt in _HALF:
        return dt if x.dtype == dt else None
    if dt != torch.float32 or x.dtype not in (torch.float32,) + _HALF:
        return None
    if ops.autocast_half():
        return torch.float16
    return torch.float32 if ops.half_products_active() else None


def _set_half(block: nn.Module, half_precision: bool) -> bool:
    """Records the half_precision keyword on a fused block (nothing is stored when it is off) -> whether it changed."""
    if bool(block.__dict__.get("_mphip_half", False)) == bool(half_precision):
        return False
    if half_precision:
        block.__dict__["_mphip_half"] = True
    else:
        block.__dict__.pop("_mphip_half", None)
    return True


def _set_trainable(block: nn.Module, trainable: bool) -> bool:
    """Records the trainable keyword on a ResBlock2DFused (nothing is stored when it is off: the flag, the block's backward packs and
    the packs ag.conv2d_packs cached on conv1 and conv2 all go) -> whether it changed."""
    if bool(block.__dict__.get("_mphip_trainable", False)) == bool(trainable):
        return False
    if trainable:
        block.__dict__["_mphip_trainable"] = True
    else:
        block.__dict__.pop("_mphip_trainable", None)
        block.__dict__.pop("_mphip_fold_bwd", None)
        for conv in (getattr(block, "conv1", None), getattr(block, "conv2", None)):   # the train-mode packs ag.conv2d_packs left on the convs
            if conv is not None:
                conv.__dict__.pop("_mphip_pack2d", None)
                conv.__dict__.pop("_mphip_bwd_pack2d", None)
    return True


def fold_batchnorm_autograd(conv: nn.Module, bn: nn.Module):
    """fold_batchnorm's (w', b') with the same operations in the same order (the same bits), but as differentiable functions of
    conv.weight, conv.bias, bn.weight and bn.bias: the running statistics are constants (eval mode, the fine-tuning case)."""
    s = bn.weight / torch.sqrt(bn.running_var.detach() + bn.eps)
    return (conv.weight * s[:, None, None, None]).contiguous(), ((conv.bias - bn.running_mean.detach()) * s + bn.bias).contiguous()


class _FoldedConv:
    """What ag.Conv3dFn asks of its `conv` argument, for a folded 1x1 shortcut: the tensors and a __dict__ for the backward pack."""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias


def _is_conv2d(m, k: int) -> bool:
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (k, k) and m.stride == (1, 1) and m.padding == ((k - 1) // 2,) * 2
            and m.dilation == (1, 1) and m.groups == 1 and m.padding_mode == "zeros" and m.bias is not None)


def _is_bn2d(m, channels: int) -> bool:
    return (isinstance(m, nn.BatchNorm2d) and m.num_features == channels and m.affine and m.track_running_stats
            and m.running_mean is not None and m.running_var is not None)


class _FusedBlock2D(nn.Module):
    """What ResBlock2DFused and ResBlockCustomFused share: adopting the children of an existing block, the fold cache, the decision
    between the three paths of forward — the one-product path (half_precision=True), the native fp32 path, the original PyTorch
    expression — and the conditions of the first two.  A subclass says what it stands in for (`matches`, _CHILDREN, _EXPECTED, _adopt), how
    it folds (_fold_tensors, _fold), which calls it takes (_EVAL_ONLY, _CUDA_FLOAT_INPUT, _dtypes, _shape_ok: the [N,C,H,W] map fits) and what it
    computes (_reference in PyTorch, _launch on the matrix cores)."""

    _CHILDREN = ()               # the children taken over from the original block, by name
    _EXPECTED = ""               # from_block's TypeError: what `matches` accepts
    _EVAL_ONLY = False           # the native paths run in eval mode only
    _CUDA_FLOAT_INPUT = False    # the fp32 path asks for a floating-point CUDA map itself (else ops refuses what it cannot run)

    @classmethod
    def from_block(cls, block: nn.Module, half_precision: bool = False):
        if not cls.matches(block):
            raise TypeError(f"{cls.__name__}.from_block: expected {cls._EXPECTED}, got {block}")
        new = cls.__new__(cls)
        nn.Module.__init__(new)
        new._adopt(block)
        for name in cls._CHILDREN:
            setattr(new, name, getattr(block, name))
        new.training = block.training   # (the children keep their own flags: they are the block's)
        _set_half(new, half_precision)
        return new

    def _native_ok(self, x) -> bool:
        if (self._EVAL_ONLY and self.training) or ag.needs_grad(self, x) or self._dtypes(False) != {torch.float32}:
            return False
        if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.numel() > 0):
            return False
        if self._CUDA_FLOAT_INPUT and not (x.is_cuda and x.is_floating_point()):
            return False
        return self._shape_ok(x)

    def _folded(self):
        """The subclass's packs (_fold), folded in fp32 torch ops (a half block: the fold of its fp32 twin); cached until a parameter or
        a running buffer changes (their versions are the key)."""
        ts = self._fold_tensors()
        key = tuple((t.data_ptr(), t._version) for t in ts) + (str(ts[0].device), ops.weight_epoch())
        hit = self.__dict__.get("_mphip_fold")
        if hit is None or hit[0] != key or ops.repacking():
            with torch.no_grad():
                hit = (key, self._fold(torch.float32 if ts[0].dtype in _HALF else None))
            self.__dict__["_mphip_fold"] = hit
        return hit[1]

    def _half_out(self, x):
        """half_precision=True: the output dtype of the one-product path for this call (_half_mode), or None."""
        if "_mphip_half" not in self.__dict__ or (self._EVAL_ONLY and self.training):
            return None
        dts = self._dtypes(True)
        dt = _half_mode(self, x, dts.pop()) if len(dts) == 1 else None
        return dt if dt is not None and not ag.needs_grad(self, x) and self._shape_ok(x) else None

    def forward(self, x):
        half = self._half_out(x)
        if half is not None:
            packs = self._folded()
            with ops.half_products(True):
                return self._launch(x, packs, half, 0)
        if not self._native_ok(x):
            return self._reference(x)
        return self._launch(x, self._folded(), None, None)


class ResBlock2DFused(_FusedBlock2D):
    """G2d's ResBlock2D (model.py:600-640, `downsample` off) with an opt-in inference path on the matrix cores: BatchNorm folded into
    the convs, each 3x3 conv one launch of csrc/conv2d_f16x3.hip (f16x3 arithmetic: fp32-class accuracy) with bias, ReLU and the
    residual add in its epilogue.  The children are the original block's own `conv1, bn1, conv2, bn2, shortcut` — the same Parameter
    and buffer objects, the same state-dict keys — built over an existing block by `from_block`.

    The native path runs only in eval mode, without autograd (ag.needs_grad false), on an fp32 module and a supported shape (Ci % 16,
    Co % 32); otherwise forward evaluates the original block's expression in PyTorch, exactly encoders2d.ResBlock2D.forward.  Without
    `trainable=True` (below) training and fine-tuning take the PyTorch expression, and there is NO half-model path for this block:
    .half() / .bfloat16() instances take it too.  fp16 / bf16 inputs (torch.autocast upstream) are widened (model._f32) and the result is fp32; channels_last
    inputs are copied to NCHW once.  A 1x1 shortcut runs through the existing k = 1 conv with its BatchNorm folded.  Each conv leaves
    the range descriptor of its output on the tensor, so a fused block that directly follows does not scan its input again.

    `from_block(block, half_precision=True)` adds the half-precision form (csrc/conv2d_lp.hip; same conditions: eval mode, no autograd,
    a supported shape).  Inside torch.autocast('cuda', float16) an fp32 block then runs ONE f16 product per multiply in both 3x3
    launches, reads its input in the dtype it arrives in and returns float16, bitwise `.half()` of what it computes from `x.float()`
    under ops.half_products(True) outside the region.  A .half() / .bfloat16() block folds its BatchNorms in fp32 from the widened
    parameters, runs one product, reads input and residual and writes the output in the model dtype (y1 stays fp32): bitwise its fp32
    twin under ops.half_products(True), rounded once.  Everything else takes the paths above.

    `from_block(block, trainable=True)` (off by default; recorded on the block and removed again when off) trains through the block on
    the matrix cores: a call that ag.needs_grad sends to the PyTorch expression takes ag.Conv2dFn instead (csrc/conv2d_bwd_f16x3.hip:
    the backward-weight kernel; backward-data is the forward kernel on the flipped, transposed pack).  fp32 modules and fp32 CUDA maps
    outside autocast only, where ops.conv2d_bwd_supported takes both convs; every other call keeps its path.
      eval mode (frozen statistics, fine-tuning): each BatchNorm is folded into its conv by differentiable torch ops on every call
        and the inference path's two launches run, with bias, ReLU and the residual in the epilogue: the output carries the bits of
        the inference path, and the gradients reach conv.weight, conv.bias, bn.weight and bn.bias through the fold.  A 1x1 shortcut
        is folded the same way and runs the inference path's k = 1 launch with ag.Conv3dFn's backward kernels.
      train mode (batch statistics): conv1 and conv2 go through ag.Conv2dFn with their own bias, the block's bn1 / bn2 modules run
        as they are (running statistics update as before), ReLU, the add and the whole shortcut (1x1 conv + BatchNorm) stay in PyTorch.
    Half, bf16 and one-product training are not built: inside torch.autocast and on a half block the keyword changes nothing."""

    _CHILDREN = ("conv1", "bn1", "conv2", "bn2", "shortcut")
    _EXPECTED = ("a ResBlock2D without downsampling (3x3 stride-1 convs with bias, BatchNorm2d with running statistics, Identity or "
                 "Conv2d 1x1 + BatchNorm2d shortcut)")
    _EVAL_ONLY = True

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.downsample = False
        self.conv1 = nn.Conv2d(in_channels, out_channels, 3, stride=1, padding=1)
        self.bn1 = nn.BatchNorm2d(out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, 3, stride=1, padding=1)
        self.bn2 = nn.BatchNorm2d(out_channels)
        if in_channels != out_channels:
            self.shortcut = nn.Sequential(nn.Conv2d(in_channels, out_channels, 1, stride=1), nn.BatchNorm2d(out_channels))
        else:
            self.shortcut = nn.Identity()

    @staticmethod
    def matches(block) -> bool:
        """Duck-typed: is `block` a ResBlock2D (this package's or the reference's) the fused path can stand in for?"""
        if isinstance(block, ResBlock2DFused):
            return False
        conv1, bn1, conv2, bn2 = (getattr(block, n, None) for n in ("conv1", "bn1", "conv2", "bn2"))
        sc = getattr(block, "shortcut", None)
        if getattr(block, "downsample", True) is not False or not (_is_conv2d(conv1, 3) and _is_conv2d(conv2, 3)):
            return False
        co = conv1.out_channels
        if conv2.in_channels != co or conv2.out_channels != co or not (_is_bn2d(bn1, co) and _is_bn2d(bn2, co)):
            return False
        if isinstance(sc, nn.Identity):
            return conv1.in_channels == co
        return (isinstance(sc, nn.Sequential) and len(sc) == 2 and _is_conv2d(sc[0], 1) and sc[0].in_channels == conv1.in_channels
                and sc[0].out_channels == co and _is_bn2d(sc[1], co))

    def _adopt(self, block):
        self.downsample = False

    def _shape_ok(self, x) -> bool:
        (n, ci, h, w), co = x.shape, self.conv1.out_channels
        return ci == self.conv1.in_channels and ops.conv2d_supported(n, ci, co, h, w) and ops.conv2d_supported(n, co, co, h, w)

    def _dtypes(self, half_path: bool):
        dt = self.conv1.weight.dtype   # (what the paths look at: conv1 alone, but every parameter and buffer of a half block)
        return {t.dtype for t in self.state_dict().values() if t.is_floating_point()} if half_path and dt in _HALF else {dt}

    def _fold_pairs(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)] + ([tuple(self.shortcut)] if isinstance(self.shortcut, nn.Sequential) else [])

    def _fold_tensors(self):
        return [t for conv, bn in self._fold_pairs() for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]

    def _fold(self, wide):
        """(conv1', conv2', shortcut' or None): BatchNorm folded and packed."""
        pairs = self._fold_pairs()
        p1, p2 = (ops.PackedConv2d(*fold_batchnorm(conv, bn, wide)) for conv, bn in pairs[:2])
        ps = None
        if len(pairs) > 2:
            ws, bs = fold_batchnorm(*pairs[2], wide)
            ps = ops.PackedConv(ws.view(ws.shape[0], ws.shape[1], 1, 1, 1), bs)
        return p1, p2, ps

    def _reference(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return F.relu(y + self.shortcut(x))

    @classmethod
    def from_block(cls, block: nn.Module, half_precision: bool = False, trainable: bool = False):
        new = super().from_block(block, half_precision)
        _set_trainable(new, trainable)
        return new

    def _trainable_ok(self, x) -> bool:
        """trainable=True: does this call take ag.Conv2dFn?  Under autograd only (every other call keeps the paths it has), an fp32
        module and an fp32 CUDA map outside autocast, and shapes whose forward, backward-weight and (where dx is wanted) backward-data
        launches the library takes."""
        if "_mphip_trainable" not in self.__dict__ or not ag.needs_grad(self, x) or self._dtypes(False) != {torch.float32}:
            return False
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
            return False
        if torch.is_autocast_enabled() or ops.half_products_active():
            return False
        (n, ci, h, w), co = x.shape, self.conv1.out_channels
        if not (ci == self.conv1.in_channels and ops.conv2d_bwd_supported(n, ci, co, h, w, bool(x.requires_grad))
                and ops.conv2d_bwd_supported(n, co, co, h, w, True)):
            return False
        if self.training or not isinstance(self.shortcut, nn.Sequential):
            return True
        # eval mode runs the 1x1 shortcut through ag.Conv3dFn (k = 1), which raises where the library has no kernel: ask first.  (Where
        # the f16x3 kernels do not take a shape the exact fp32 ones do, so this holds wherever the 3x3 rules above hold.)
        lib = ops._lib.load()
        return bool(lib.mphip_conv3d_supported(n, ci, co, 1, h, w, 1, 0) and lib.mphip_conv3d_supported(n, co, ci, 1, h, w, 1, 0)
                    and lib.mphip_conv3d_bwd_weight_workspace_bytes(n, ci, co, 1, h, w, 1, 0) and lib.mphip_packed_weight_bytes(ci, co, 1, 0))

    def _folded_bwd(self):
        """(conv1', conv2', shortcut') backward-data packs of the folded weights (None where the transposed pack's rule refuses the
        channels, and for an identity shortcut), cached like _folded.  The shortcut's is ag.Conv3dFn's transposed k = 1 PackedConv."""
        ts = self._fold_tensors()
        key = tuple((t.data_ptr(), t._version) for t in ts) + (str(ts[0].device), ops.weight_epoch())
        hit = self.__dict__.get("_mphip_fold_bwd")
        if hit is None or hit[0] != key or ops.repacking():
            with torch.no_grad():
                ws = [fold_batchnorm(conv, bn)[0] for conv, bn in self._fold_pairs()]
            t3 = ops.PackedConv(ws[2].view(ws[2].shape[0], ws[2].shape[1], 1, 1, 1), None, transposed=True) if len(ws) > 2 else None
            hit = (key, tuple(ops.PackedConv2d(w, None, transposed=True) if w.shape[0] % 16 == 0 and w.shape[1] % 32 == 0 else None
                              for w in ws[:2]) + (t3,))
            self.__dict__["_mphip_fold_bwd"] = hit
        return hit[1]

    def _train_forward(self, x):
        """The two paths of trainable=True (class docstring)."""
        xc = x.contiguous()
        if self.training:   # batch statistics: the block's own BatchNorm modules run as they are; ReLU, add and shortcut stay in torch
            f1, b1 = ag.conv2d_packs(self.conv1, bool(x.requires_grad))
            y = F.relu(self.bn1(ag.conv2d(xc, self.conv1.weight, self.conv1.bias, f1, b1)))
            f2, b2 = ag.conv2d_packs(self.conv2, True)
            y = self.bn2(ag.conv2d(y, self.conv2.weight, self.conv2.bias, f2, b2))
            return F.relu(y + self.shortcut(x))
        # frozen statistics: the inference path's two launches, on weights folded by differentiable torch ops (the same bits as the
        # cached fold the packs were made from), so the gradients reach conv.weight, conv.bias, bn.weight and bn.bias through the fold
        p1, p2, ps = self._folded()
        t1, t2, ts_ = self._folded_bwd()
        pairs = self._fold_pairs()
        (w1, c1), (w2, c2) = (fold_batchnorm_autograd(conv, bn) for conv, bn in pairs[:2])
        idt = xc
        if ps is not None:   # the 1x1 shortcut: the inference path's k = 1 launch, with ag.Conv3dFn's backward kernels
            ws, cs = fold_batchnorm_autograd(*pairs[2])
            n, c, h, w = xc.shape
            folded = _FoldedConv(ws.view(ws.shape[0], ws.shape[1], 1, 1, 1), cs)
            if not ops.repacking():   # the cached backward pack, under the key ag.Conv3dFn's backward looks it up with
                folded.__dict__["_mphip_bwd_pack"] = (ops._pack_cache_key(folded, "_mphip_bwd_pack"), ts_)
            idt = ag.conv3d(xc.reshape(n, c, 1, h, w), folded, ps).reshape(n, ps.co, h, w)
        y1 = ag.conv2d(xc, w1, c1, p1, t1 if x.requires_grad else None, relu=True)
        return ag.conv2d(y1, w2, c2, p2, t2, residual=idt, relu=True)

    def forward(self, x):
        if self._trainable_ok(x):
            return self._train_forward(x)
        return super().forward(x)

    def _launch(self, x, packs, out_dtype, products):
        """Both 3x3 launches and the 1x1 shortcut.  products None: the fp32 path (a half input is widened, the fp32 entry); 0: the
        one-product path, which reads x in its own dtype and writes out_dtype."""
        p1, p2, ps = packs
        half = products is not None
        if not half:
            x = _f32(x)
        elif x.dtype in _HALF and x.dtype != out_dtype:   # (a bf16 map inside a float16 region: one half dtype per launch)
            x = x.float()
        xc = x.contiguous()   # (the kernels read NCHW: a channels_last map is copied once)
        if half and ps is not None:   # the 1x1 shortcut reads fp32: one widening pass, which also delivers the descriptor conv1 needs
            xc = ops.cast_to_f32_range(xc)

        def shortcut():
            if ps is None:
                return xc
            n, c, h, w = xc.shape
            return ops.conv3d(xc.reshape(n, c, 1, h, w), ps, x_range=ops.current_range(xc)).reshape(n, ps.co, h, w)

        # (the shortcut is launched before conv1 on the one-product path and after it on the fp32 path)
        idt = shortcut() if half else None
        y1 = ops.conv2d(xc, p1, relu=True, want_range=True, products=products)
        if not half:
            idt = shortcut()
        return ops.conv2d(y1, p2, residual=idt, relu=True, want_range=True, out_dtype=out_dtype, products=products)


def _up2_axis(l: int, device):
    """Rows (or columns) of up2 for a map with l of them -> (i0, i1 int64 [2l], lambda fp32 [2l]): num = i (l - 1), den = 2l - 1 (l == 1:
    num = 0, den = 1), i0 = num div den, lambda = float(num mod den) / float(den) (one fp32 division, on the host: IEEE), i1 = min(i0 + 1, l - 1)."""
    i = torch.arange(2 * l, dtype=torch.int64)
    num, den = i * (l - 1), 2 * l - 1
    i0 = num // den
    lam = (num % den).to(torch.float32) / torch.tensor(den, dtype=torch.float32)
    return i0.to(device), torch.clamp(i0 + 1, max=l - 1).to(device), lam.to(device)


def up2_reference(x: torch.Tensor) -> torch.Tensor:
    """nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True) of x [N,C,h,w] -> [N,C,2h,2w] as the kernels of
    csrc/conv2d_up2_f16x3.hip compute it: exact integer coordinates (_up2_axis), horizontal first,
        top = x[i0,j0] (1 - mu) + x[i0,j1] mu,   bot = x[i1,j0] (1 - mu) + x[i1,j1] mu,   u = top (1 - lambda) + bot lambda,
    every product, sum and 1 - . a torch operation of its own (`*`, `+`, `-`: nothing that may fuse), so each is rounded to fp32 once.
    ops.conv2d_up2 / ops.conv2d_resup2 reproduce conv2d(up2_reference(x)) / conv2d(x, residual=up2_reference(r)) bit for bit."""
    if x.dim() != 4 or not x.is_floating_point():
        raise RuntimeError(f"up2_reference: expected a floating-point [N,C,h,w] map, got {tuple(x.shape)} {x.dtype}")
    h, w = x.shape[2:]
    i0, i1, lam = _up2_axis(h, x.device)
    j0, j1, mu = _up2_axis(w, x.device)
    lam, mu = lam.to(x.dtype)[:, None], mu.to(x.dtype)
    ol, om = torch.ones_like(lam) - lam, torch.ones_like(mu) - mu
    r0, r1 = x[:, :, i0], x[:, :, i1]
    top = r0[:, :, :, j0] * om + r0[:, :, :, j1] * mu
    bot = r1[:, :, :, j0] * om + r1[:, :, :, j1] * mu
    return top * ol + bot * lam


def _is_up2(m) -> bool:
    """Exactly nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)?"""
    if not isinstance(m, nn.Upsample) or m.size is not None or m.mode != "bilinear" or m.align_corners is not True:
        return False
    if getattr(m, "recompute_scale_factor", None):
        return False
    sf = m.scale_factor
    return sf is not None and all(float(s) == 2.0 for s in (sf if isinstance(sf, (tuple, list)) else (sf, sf))) and (
        not isinstance(sf, (tuple, list)) or len(sf) == 2)


class Up2ResBlock2DFused(nn.Sequential):
    """A whole `nn.Sequential(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True), ResBlock2D)` stage of G2d with the
    up-sample folded into the block's convs (csrc/conv2d_up2_f16x3.hip): the up-sampled map is never written.  Positions 0 and 1 hold
    the very Upsample object and the block (a ResBlock2DFused over the original block's children, whose fold cache and conditions this
    class uses): every state-dict key, module name and Parameter object stays.

    Native path (eval mode, no autograd, an fp32 block with a 1x1 shortcut, a supported shape):
        s   = shortcut'(x)                       at LOW resolution, through the k = 1 conv: a 1x1 conv and a bilinear resample commute
        y1  = ops.conv2d_up2(x, conv1', relu)    conv1 reads up2(x), blended while it is staged
        out = ops.conv2d_resup2(y1, conv2', s, relu)     conv2 adds up2(s), blended in its epilogue
    with x's own range descriptor as the bound of up2(x).  The commuted shortcut changes the rounding order: against the unfused stage
    this is an accuracy contract (fp32-class, like the block's), not a bitwise one.  Everything else — train mode, autograd, a half
    model, a block built with half_precision=True — evaluates exactly the two modules in order."""

    @staticmethod
    def matches(seq) -> bool:
        if not isinstance(seq, nn.Sequential) or isinstance(seq, Up2ResBlock2DFused) or len(seq) != 2 or not _is_up2(seq[0]):
            return False
        blk = seq[1]
        return (isinstance(blk, ResBlock2DFused) or ResBlock2DFused.matches(blk)) and isinstance(blk.shortcut, nn.Sequential)

    @classmethod
    def from_sequential(cls, seq: nn.Sequential) -> "Up2ResBlock2DFused":
        if not cls.matches(seq):
            raise TypeError(f"{cls.__name__}.from_sequential: expected Sequential(Upsample(scale_factor=2, bilinear, align_corners=True), "
                            f"a ResBlock2D with a 1x1 shortcut), got {seq}")
        blk = seq[1] if isinstance(seq[1], ResBlock2DFused) else ResBlock2DFused.from_block(seq[1])
        new = cls(seq[0], blk)
        new.training = seq.training
        return new

    def _native_ok(self, x) -> bool:
        blk = self[1]
        if not isinstance(blk, ResBlock2DFused) or "_mphip_half" in blk.__dict__ or not isinstance(blk.shortcut, nn.Sequential):
            return False
        if blk.training or ag.needs_grad(blk, x) or blk._dtypes(False) != {torch.float32}:
            return False
        if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.numel() > 0 and x.is_floating_point()):
            return False
        (n, ci, h, w), co = x.shape, blk.conv1.out_channels
        return ci == blk.conv1.in_channels and ops.conv2d_up2_supported(n, ci, co, h, w) and ops.conv2d_up2_supported(n, co, co, h, w)

    def forward(self, x):
        if not self._native_ok(x):
            return self[1](self[0](x))
        p1, p2, ps = self[1]._folded()
        xc = _f32(x).contiguous()   # (the kernels read NCHW: a channels_last map is copied once)
        n, c, h, w = xc.shape
        xr = ops.current_range(xc)
        if xr is None:
            xr = ops.absmax_range(xc)   # one scan of the LOW-resolution map serves the shortcut and conv1: a bound of up2(x)
        s = ops.conv3d(xc.reshape(n, c, 1, h, w), ps, x_range=xr).reshape(n, ps.co, h, w)
        y1 = ops.conv2d_up2(xc, p1, relu=True, x_range=xr, want_range=True)
        return ops.conv2d_resup2(y1, p2, s, relu=True, want_range=True)


def _is_conv2d_at(m, k: int, stride: int) -> bool:
    """_is_conv2d at a given stride, and with or without a bias (BasicBlockFused's convs)."""
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (k, k) and m.stride == (stride, stride) and m.padding == ((k - 1) // 2,) * 2
            and m.dilation == (1, 1) and m.groups == 1 and m.padding_mode == "zeros")


class BasicBlockFused(_FusedBlock2D):
    """A torchvision-style ResNet BasicBlock — encoders2d._BasicBlock, the reference's resnet.BasicBlock: 3x3 conv, BatchNorm, ReLU,
    3x3 conv, BatchNorm, add, ReLU; `downsample` is None or Sequential(1x1 conv at conv1's stride, BatchNorm) — with an opt-in inference
    path on the matrix cores, as ResBlock2DFused has it: BatchNorm folded into the (bias-less) convs, each 3x3 conv one launch with bias,
    ReLU and the residual add in its epilogue, f16x3 arithmetic (fp32-class accuracy).  A stride-1 block is ResBlock2DFused's two launches
    of csrc/conv2d_f16x3.hip.  A stride-2 block runs conv1 on csrc/conv2d_s2_f16x3.hip; its 1x1 stride-2 `downsample` reads a
    quarter-size torch copy x[:, :, ::2, ::2] through the existing k = 1 conv with the BatchNorm folded (not fused into the stride-2
    launch).  The children are the original block's own `conv1, bn1, relu, conv2, bn2, downsample`: the same Parameter and buffer
    objects, the same state-dict keys.

    The native path runs only in eval mode, without autograd, on an fp32 module and a supported shape (Ci % 16, Co % 32); otherwise
    forward evaluates the original block's expression in PyTorch.  There are NO backward kernels, NO half-model path and NO
    half_precision form: training and .half() / .bfloat16() instances take the PyTorch expression.  fp16 / bf16 inputs are widened and
    the result is fp32; channels_last inputs are copied to NCHW once.  Each block leaves the range descriptor of its output on the
    tensor, so only the first block of a net scans its input."""

    _CHILDREN = ("conv1", "bn1", "relu", "conv2", "bn2", "downsample")
    _EXPECTED = ("a ResNet BasicBlock (3x3 convs with or without bias, the first at stride 1 or 2, BatchNorm2d with running statistics, "
                 "downsample None or Conv2d 1x1 at that stride + BatchNorm2d, no `shortcut`)")
    _EVAL_ONLY = True
    split_small_maps = False   # set: the stride-1 launches pass splits="auto" (the split-K form where ops.conv2d_splits recommends it)

    def __init__(self, inplanes: int, planes: int, stride: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride=stride, bias=False), nn.BatchNorm2d(planes))

    @classmethod
    def from_block(cls, block: nn.Module, half_precision: bool = False):
        if half_precision:
            raise TypeError("BasicBlockFused has no half_precision form")
        return super().from_block(block, False)

    @staticmethod
    def matches(block) -> bool:
        """Duck-typed: is `block` a BasicBlock the fused path can stand in for?  (Not a ResBlock2D: that one has a `shortcut`.)"""
        if isinstance(block, _FusedBlock2D) or not isinstance(block, nn.Module) or hasattr(block, "shortcut"):
            return False
        conv1, bn1, relu, conv2, bn2 = (getattr(block, n, None) for n in ("conv1", "bn1", "relu", "conv2", "bn2"))
        if not isinstance(relu, nn.ReLU) or not hasattr(block, "downsample"):
            return False
        stride = 2 if isinstance(conv1, nn.Conv2d) and conv1.stride == (2, 2) else 1
        if not (_is_conv2d_at(conv1, 3, stride) and _is_conv2d_at(conv2, 3, 1)):
            return False
        ci, co = conv1.in_channels, conv1.out_channels
        if conv2.in_channels != co or conv2.out_channels != co or not (_is_bn2d(bn1, co) and _is_bn2d(bn2, co)):
            return False
        ds = block.downsample
        if ds is None:
            return stride == 1 and ci == co
        return (isinstance(ds, nn.Sequential) and len(ds) == 2 and _is_conv2d_at(ds[0], 1, stride) and ds[0].in_channels == ci
                and ds[0].out_channels == co and _is_bn2d(ds[1], co))

    def _adopt(self, block):
        pass

    def _stride(self) -> int:
        return self.conv1.stride[0]

    def _shape_ok(self, x) -> bool:
        (n, ci, h, w), co, s = x.shape, self.conv1.out_channels, self._stride()
        if ci != self.conv1.in_channels:
            return False
        if s == 1:
            return ops.conv2d_supported(n, ci, co, h, w) and ops.conv2d_supported(n, co, co, h, w)
        return ops.conv2d_s2_supported(n, ci, co, h, w) and ops.conv2d_supported(n, co, co, (h + 1) // 2, (w + 1) // 2)

    def _dtypes(self, half_path: bool):
        return {self.conv1.weight.dtype}

    def _fold_pairs(self):
        return [(self.conv1, self.bn1), (self.conv2, self.bn2)] + ([tuple(self.downsample)] if self.downsample is not None else [])

    def _fold_tensors(self):
        return [t for conv, bn in self._fold_pairs() for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
                if t is not None]

    _fold = ResBlock2DFused._fold   # (conv1', conv2', downsample' or None): BatchNorm folded and packed

    def _reference(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        return self.relu(self.bn2(self.conv2(y)) + idt)

    def _launch(self, x, packs, out_dtype, products):
        """Stride 1: ResBlock2DFused's launches.  Stride 2: the stride-2 conv, the 1x1 conv on the even sub-sample, the second conv."""
        p1, p2, ps = packs
        xc = _f32(x).contiguous()   # (the kernels read NCHW: a channels_last map is copied once)
        s2 = self._stride() == 2
        split = {"splits": "auto"} if self.split_small_maps else {}   # (stride 1 only: there is no split form of the stride-2 kernel)
        y1 = ops.conv2d_s2(xc, p1, relu=True, want_range=True) if s2 else ops.conv2d(xc, p1, relu=True, want_range=True, **split)
        idt = xc
        if ps is not None:
            xr = ops.current_range(xc)   # (of the whole map: a valid bound of its sub-sample)
            xs = xc[:, :, ::2, ::2].contiguous() if s2 else xc
            n, c, h, w = xs.shape
            idt = ops.conv3d(xs.reshape(n, c, 1, h, w), ps, x_range=xr).reshape(n, ps.co, h, w)
        return ops.conv2d(y1, p2, residual=idt, relu=True, want_range=True, **split)


class BottleneckFused(_FusedBlock2D):
    """A torchvision-layout ResNet bottleneck — encoders2d._Bottleneck, torchvision's Bottleneck: 1x1 conv, BatchNorm, ReLU, 3x3 conv (the
    block's stride is here), BatchNorm, ReLU, 1x1 conv, BatchNorm, add, ReLU; `downsample` is None or Sequential(1x1 conv at conv2's
    stride, BatchNorm) — with an opt-in inference path on the matrix cores, as BasicBlockFused has it: BatchNorm folded into the
    (bias-less) convs, every conv one launch with bias, ReLU and the residual add in its epilogue, f16x3 arithmetic (fp32-class accuracy):
        y1  = conv2d_pw(x,  conv1', relu)
        y2  = conv2d(y1, conv2', relu)                       stride 2: conv2d_s2
        idt = x                                              or conv2d_pw(x, downsample', stride = conv2's)
        out = conv2d_pw(y2, conv3', residual = idt, relu)
    — three launches, four with a `downsample`.  The 1x1 convs run on csrc/conv2d_pw_f16x3.hip; a stride-2 `downsample` sub-samples in
    the kernel's loads (no copy of x).  The children are the original block's own `conv1, bn1, conv2, bn2, conv3, bn3, relu, downsample`:
    the same Parameter and buffer objects, the same state-dict keys.

    The native path runs only in eval mode, without autograd, on an fp32 module and a supported shape (channels % 16 in, % 32 out);
    otherwise forward evaluates the original block's expression in PyTorch.  There are NO backward kernels, NO half-model path and NO
    half_precision form.  fp16 / bf16 inputs are widened and the result is fp32; channels_last inputs are copied to NCHW once.  Every
    launch leaves the range descriptor of its output on the tensor, so only the first block of a net scans its input (once: conv1 and
    the downsample share the descriptor, which bounds the sub-sample as well)."""

    _CHILDREN = ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "relu", "downsample")
    _EXPECTED = ("a torchvision-layout ResNet bottleneck (conv1 and conv3 1x1 at stride 1, conv2 3x3 with padding 1 at stride 1 or 2, no "
                 "groups or dilation, BatchNorm2d with running statistics, downsample None or Conv2d 1x1 at conv2's stride + BatchNorm2d, no "
                 "`shortcut`)")
    _EVAL_ONLY = True
    _CUDA_FLOAT_INPUT = True   # a CPU map takes the original expression

    def __init__(self, inplanes: int, planes: int, stride: int = 1, expansion: int = 4):
        super().__init__()
        out = planes * expansion
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, out, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or inplanes != out:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, out, 1, stride=stride, bias=False), nn.BatchNorm2d(out))

    @classmethod
    def from_block(cls, block: nn.Module, half_precision: bool = False):
        if half_precision:
            raise TypeError("BottleneckFused has no half_precision form")
        return super().from_block(block, False)

    @staticmethod
    def matches(block) -> bool:
        """Duck-typed: is `block` a bottleneck the fused path can stand in for?  (The v1 layout, with the stride on conv1, is not.)"""
        if isinstance(block, _FusedBlock2D) or not isinstance(block, nn.Module) or hasattr(block, "shortcut"):
            return False
        conv1, bn1, conv2, bn2, conv3, bn3, relu = (getattr(block, n, None) for n in ("conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "relu"))
        if not isinstance(relu, nn.ReLU) or not hasattr(block, "downsample"):
            return False
        stride = 2 if isinstance(conv2, nn.Conv2d) and conv2.stride == (2, 2) else 1
        if not (_is_conv2d_at(conv1, 1, 1) and _is_conv2d_at(conv2, 3, stride) and _is_conv2d_at(conv3, 1, 1)):
            return False
        ci, mid, co = conv1.in_channels, conv1.out_channels, conv3.out_channels
        if (conv2.in_channels, conv2.out_channels, conv3.in_channels) != (mid, mid, mid):
            return False
        if not (_is_bn2d(bn1, mid) and _is_bn2d(bn2, mid) and _is_bn2d(bn3, co)):
            return False
        ds = block.downsample
        if ds is None:
            return stride == 1 and ci == co
        return (isinstance(ds, nn.Sequential) and len(ds) == 2 and _is_conv2d_at(ds[0], 1, stride) and ds[0].in_channels == ci
                and ds[0].out_channels == co and _is_bn2d(ds[1], co))

    def _adopt(self, block):
        pass

    def _stride(self) -> int:
        return self.conv2.stride[0]

    def _shape_ok(self, x) -> bool:
        (n, ci, h, w), mid, co, s = x.shape, self.conv1.out_channels, self.conv3.out_channels, self._stride()
        if ci != self.conv1.in_channels:
            return False
        ho, wo = (h + s - 1) // s, (w + s - 1) // s
        mid_ok = ops.conv2d_supported(n, mid, mid, h, w) if s == 1 else ops.conv2d_s2_supported(n, mid, mid, h, w)
        return (mid_ok and ops.conv2d_pw_supported(n, ci, mid, h, w, 1) and ops.conv2d_pw_supported(n, mid, co, ho, wo, 1)
                and (self.downsample is None or ops.conv2d_pw_supported(n, ci, co, h, w, s)))

    def _dtypes(self, half_path: bool):
        return {self.conv1.weight.dtype}

    def _fold_pairs(self):
        return ([(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]
                + ([tuple(self.downsample)] if self.downsample is not None else []))

    _fold_tensors = BasicBlockFused._fold_tensors

    def _fold(self, wide):
        """(conv1', conv2', conv3', downsample' or None): BatchNorm folded and packed (a 1x1 weight makes a pointwise pack)."""
        packs = [ops.PackedConv2d(*fold_batchnorm(conv, bn, wide)) for conv, bn in self._fold_pairs()]
        return tuple(packs) if len(packs) == 4 else (*packs, None)

    def _reference(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        return self.relu(self.bn3(self.conv3(y)) + idt)

    def _launch(self, x, packs, out_dtype, products):
        p1, p2, p3, pd = packs
        xc = _f32(x).contiguous()   # (the kernels read NCHW: a channels_last map is copied once)
        s = self._stride()
        # two launches read x: one descriptor serves both (of the whole map: a valid bound of its sub-sample); else the library scans
        xr = ops._range_for(xc) if pd is not None else None
        y1 = ops.conv2d_pw(xc, p1, relu=True, x_range=xr, want_range=True)
        y2 = ops.conv2d_s2(y1, p2, relu=True, want_range=True) if s == 2 else ops.conv2d(y1, p2, relu=True, want_range=True)
        idt = xc if pd is None else ops.conv2d_pw(xc, pd, stride=s, x_range=xr)
        return ops.conv2d_pw(y2, p3, residual=idt, relu=True, want_range=True)


def _swap_slot(cls, cur, enable: bool, half_precision: bool, trainable=None):
    """One slot of native_g2d_body / native_eapp_trunk -> (the module the slot holds now, whether anything changed): a matching block
    becomes a `cls` over the same children, a fused one takes the keywords' values, or (enable off) the very object it replaced comes
    back.  trainable: None for a class without the keyword, else ResBlock2DFused's."""
    if enable and isinstance(cur, cls):
        did = _set_half(cur, half_precision)
        return cur, (_set_trainable(cur, trainable) or did) if trainable is not None else did
    if enable and cls.matches(cur):
        new = cls.from_block(cur, half_precision) if trainable is None else cls.from_block(cur, half_precision, trainable=trainable)
        new.__dict__["_replaced"] = cur   # (not a registered child: the module tree and the state-dict keys stay as they were)
        return new, True
    if not enable and isinstance(cur, cls) and "_replaced" in cur.__dict__:
        if trainable is not None:
            _set_trainable(cur, False)   # (the packs it cached on the children, which the original block shares)
        return cur.__dict__.pop("_replaced"), True
    return cur, False


_G2D_BODY_SLOTS = (("upsample1", 1), ("upsample2", 1), ("upsample3", 1))


def native_g2d_body(g2d: nn.Module, enable: bool = True, half_precision: bool = False, fuse_upsample: bool = False,
                    trainable: bool = False) -> bool:
    """Swaps every matching ResBlock2D of `g2d.res_blocks`, `g2d.upsample1[1]`, `upsample2[1]`, `upsample3[1]` (this package's G2d or
    the reference's, model.py:720-746) for a ResBlock2DFused over the same children, or puts the very objects it replaced back.
    Returns whether anything changed.  Off by default everywhere.  half_precision: the blocks' half-precision form (ResBlock2DFused);
    blocks that are fused already take the keyword's value.
    fuse_upsample (off by default): each matching `Sequential(Upsample x2 bilinear align_corners, block)` of `upsample1/2/3` also becomes
    an Up2ResBlock2DFused over the same two objects, which folds the up-sample into the block's convs; without the keyword (or with
    enable off) the very Sequential objects come back.  With half_precision=True the three stages keep the materialised up-sample:
    there is no typed or one-product form of the up2 kernels.
    trainable (off by default): under autograd the fused blocks run ag.Conv2dFn, forward and backward on the matrix cores
    (ResBlock2DFused); blocks that are fused already take the keyword's value.  Up2ResBlock2DFused is not touched: under autograd a
    stage evaluates its two modules in order as before, the nn.Upsample in PyTorch and then the block, which takes its own path."""
    fuse = bool(enable and fuse_upsample and not half_precision)
    changed = False
    if not fuse:   # (first: the slots below are looked up in the Sequentials that hold them)
        for name, _ in _G2D_BODY_SLOTS:
            cur = getattr(g2d, name, None)
            if isinstance(cur, Up2ResBlock2DFused) and "_replaced" in cur.__dict__:
                setattr(g2d, name, cur.__dict__.pop("_replaced"))
                changed = True
    seqs = [(getattr(g2d, "res_blocks", None), None)] + [(getattr(g2d, name, None), idx) for name, idx in _G2D_BODY_SLOTS]
    for seq, only in seqs:
        if not isinstance(seq, nn.Sequential):
            continue
        for i in (range(len(seq)) if only is None else [only] if len(seq) > only else []):
            new, did = _swap_slot(ResBlock2DFused, seq[i], enable, half_precision, bool(trainable))
            if new is not seq[i]:
                seq[i] = new
            changed |= did
    if fuse:
        for name, _ in _G2D_BODY_SLOTS:
            cur = getattr(g2d, name, None)
            if Up2ResBlock2DFused.matches(cur) and isinstance(cur[1], ResBlock2DFused):
                new = Up2ResBlock2DFused.from_sequential(cur)
                new.__dict__["_replaced"] = cur   # (not a registered child: the module tree and the state-dict keys stay as they were)
                setattr(g2d, name, new)
                changed = True
    return changed


def _set_split(block, on: bool) -> bool:
    """`split_small_maps` of a BasicBlockFused / RepVGGBlockFused -> whether it changed (off: the class's default, no instance attribute)."""
    if bool(block.split_small_maps) == on:
        return False
    if on:
        block.split_small_maps = True
    else:
        block.__dict__.pop("split_small_maps", None)
    return True


def native_emtn_resnets(emtn: nn.Module, enable: bool = True, split_small_maps: bool = False) -> bool:
    """Swaps every matching BasicBlock in every nn.Sequential stage of `emtn.head_pose_net` and `emtn.expression_net` (this package's Emtn
    or the reference's, model.py:869-907; the stages are found by type: `layer1..4` in the first, positional children in the second)
    for a BasicBlockFused over the same children, or puts the very objects it replaced back.  Returns whether anything changed.  Off by
    default everywhere; opt-in, inference only.  What stays on PyTorch: each net's 3->64 stem conv + BatchNorm + ReLU + max-pool (Ci = 3
    does not fit the kernel; native_emtn_stems fuses it on its own), the pools and the `fc`s.  The third net, the 6DRepNet
    `rotation_net` (not an nn.Module of Gbase), has a switch of its own: native_rotation_net.
    split_small_maps (off by default): the fused blocks' stride-1 convs ask ops.conv2d_splits for a split-K launch
    (csrc/conv2d_splitk_f16x3.hip); without the keyword every fused block is back on the unsplit kernels."""
    changed = False
    for net in (getattr(emtn, "head_pose_net", None), getattr(emtn, "expression_net", None)):
        if not isinstance(net, nn.Module):
            continue
        for stage in net.children():
            if not isinstance(stage, nn.Sequential):
                continue
            for i in range(len(stage)):
                new, did = _swap_slot(BasicBlockFused, stage[i], enable, False)
                if new is not stage[i]:
                    stage[i] = new
                if isinstance(new, BasicBlockFused):
                    did |= _set_split(new, bool(enable and split_small_maps))
                changed |= did
    return changed


class _StemSlot(nn.Module):
    """One of the four stand-ins StemFused.swap puts into the stem slots `conv1, bn1, relu, maxpool` of a ResNet.  It registers the
    Parameters and buffers of the module it replaces under their own names — the same objects, so the state-dict keys, their order and
    `parameters()` stay as they were — and keeps that module itself out of the module tree, in `__dict__` (`named_modules()` keeps its
    names).  `train()` / `eval()` reach the original through it, and `.to()` / `.half()` hand the converted buffers on to it."""

    def _take(self, orig: nn.Module, head: "StemFused"):
        self.__dict__["_orig"], self.__dict__["_head"] = orig, head
        for name, param in orig._parameters.items():
            self.register_parameter(name, param)
        for name, buf in orig._buffers.items():
            self.register_buffer(name, buf, persistent=name not in orig._non_persistent_buffers_set)
        self.training = orig.training
        self._version = orig._version   # (state_dict()'s metadata records it per module: BatchNorm's is 2)
        return self

    def train(self, mode: bool = True):
        self._orig.train(mode)
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self._orig._parameters.update(self._parameters)   # (torch converts Parameters in place, and replaces buffer objects)
        self._orig._buffers.update(self._buffers)
        return self

    def extra_repr(self) -> str:
        return f"stands in for {self._orig}"


class _StemPass(_StemSlot):
    """The `bn1`, `relu` and `maxpool` slots of a fused stem: a tensor that carries the mark of this stem's StemFused has been through all
    four modules already and is returned as it is — the same object, untouched (the in-place ReLU would bump its version and drop its
    range descriptor); the last slot takes the mark off.  Anything else goes through the original module."""

    def __init__(self, orig: nn.Module, head: "StemFused", last: bool):
        super().__init__()
        self._take(orig, head)
        self.__dict__["_last"] = last

    def forward(self, x):
        if isinstance(x, torch.Tensor) and x.__dict__.get("_mphip_stem") is self._head:
            if self._last:
                del x._mphip_stem
            return x
        return self._orig(x)


class StemFused(_StemSlot):
    """The stem `conv1 (3 -> Co, 3x3, stride 1, padding 1) -> bn1 -> relu -> maxpool(3, stride 2, padding 1)` of a torchvision-style
    ResNet with a CIFAR stem — encoders2d.CifarResNet18 (Emtn's `head_pose_net`, whose forward calls the four attributes in turn), the
    first four positions of the nn.Sequential `expression_net`, the reference's resnet.py — as ONE launch of csrc/conv2d_stem.hip: the
    BatchNorm folded into the conv (fold_batchnorm), bias, ReLU and the max-pool in the kernel, exact fp32 FMA arithmetic, the full-size
    64-channel map never written.  Opt-in, inference only; `StemFused.swap(net)` puts a StemFused into the `conv1` slot and pass-through
    stand-ins (_StemPass) into the other three, `swap(net, False)` puts the very objects back.  State-dict keys, `named_modules()` names and
    the Parameter and buffer objects are the net's own.

    The native path runs in eval mode, without autograd (ag.needs_grad false), on an fp32 module, a CUDA image and a supported shape
    (ops.conv2d_stem_supported); an fp16 / bf16 image is widened, a channels_last one copied once, the result is fp32 and carries the
    range descriptor of its exact max|y|, so the first fused BasicBlock of `layer1` does not scan it.  Otherwise this slot runs the
    original conv and returns an unmarked tensor, so the originals of the other three slots run: the original expression, bit for bit,
    on the CPU, in train mode, under autograd and on half modules.  A net whose forward does not call the four slots in turn on one
    tensor is not one this class stands in for."""

    _SLOTS = ("conv1", "bn1", "relu", "maxpool")

    def __init__(self, conv: nn.Module, bn: nn.Module, relu: nn.Module, pool: nn.Module):
        super().__init__()
        self._take(conv, self)
        self.__dict__["_bn"], self.__dict__["_relu"], self.__dict__["_pool"] = bn, relu, pool

    @classmethod
    def _find(cls, net):
        """The four slots of `net` -> (keys, modules): positions 0-3 of an nn.Sequential, else the attributes _SLOTS; None without them."""
        if isinstance(net, nn.Sequential):
            return (list(range(4)), [net[i] for i in range(4)]) if len(net) >= 4 else None
        mods = [getattr(net, name, None) for name in cls._SLOTS] if isinstance(net, nn.Module) else [None]
        return (list(cls._SLOTS), mods) if all(isinstance(m, nn.Module) for m in mods) else None

    @classmethod
    def matches(cls, net) -> bool:
        """Duck-typed: does `net` begin with a stem this class can stand in for (and is it not fused already)?"""
        from torch.nn.modules.utils import _pair

        found = cls._find(net)
        if found is None or any(isinstance(m, _StemSlot) for m in found[1]):
            return False
        conv, bn, relu, pool = found[1]
        if not (_is_conv2d_at(conv, 3, 1) and conv.in_channels == 3 and _is_bn2d(bn, conv.out_channels) and isinstance(relu, nn.ReLU)):
            return False
        return (isinstance(pool, nn.MaxPool2d) and _pair(pool.kernel_size) == (3, 3) and _pair(pool.stride) == (2, 2)
                and _pair(pool.padding) == (1, 1) and _pair(pool.dilation) == (1, 1) and not pool.ceil_mode and not pool.return_indices)

    @classmethod
    def swap(cls, net, enable: bool = True) -> bool:
        """Fuses the stem of `net` (matches) or, enable off, puts the four original modules back -> whether anything changed."""
        found = cls._find(net)
        if found is None:
            return False
        keys, mods = found
        put = net.__setitem__ if isinstance(net, nn.Sequential) else (lambda key, m: setattr(net, key, m))
        if enable:
            if not cls.matches(net):
                return False
            head = cls(*mods)
            for i, (key, m) in enumerate(zip(keys, mods)):
                put(key, head if i == 0 else _StemPass(m, head, last=i == 3))
            return True
        changed = False
        for key, m in zip(keys, mods):
            if isinstance(m, _StemSlot):
                put(key, m._orig)
                changed = True
        return changed

    def _fold_tensors(self):
        conv, bn = self._orig, self._bn
        return [t for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]

    def _native_ok(self, x) -> bool:
        if self.training or self._bn.training or ag.needs_grad(self, x) or ag.needs_grad(self._bn):
            return False
        ts = self._fold_tensors()
        if {t.dtype for t in ts} != {torch.float32}:
            return False
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_floating_point() and x.dim() == 4 and x.numel() > 0):
            return False
        n, ci, h, w = x.shape
        return ci == 3 and all(t.device == x.device for t in ts) and ops.conv2d_stem_supported(n, ci, self._orig.out_channels, h, w, True)

    def _folded(self):
        """(w', b') of fold_batchnorm(conv1, bn1), cached until a parameter or a running buffer changes (_FusedBlock2D._folded's key)."""
        ts = self._fold_tensors()
        key = tuple((t.data_ptr(), t._version) for t in ts) + (str(ts[0].device), ops.weight_epoch())
        hit = self.__dict__.get("_mphip_fold")
        if hit is None or hit[0] != key or ops.repacking():
            with torch.no_grad():
                hit = (key, fold_batchnorm(self._orig, self._bn))
            self.__dict__["_mphip_fold"] = hit
        return hit[1]

    def forward(self, x):
        if not self._native_ok(x):
            return self._orig(x)   # unmarked: bn1, relu and maxpool run as the modules they are
        w, b = self._folded()
        y = ops.conv2d_stem(_f32(x), w, b, relu=True, pool=True, want_range=True)
        y._mphip_stem = self   # bn1, relu and maxpool hand it through; maxpool takes the mark off
        return y


def native_emtn_stems(emtn: nn.Module, enable: bool = True) -> bool:
    """Swaps the stem `conv1, bn1, relu, maxpool` of `emtn.head_pose_net` (attributes) and of `emtn.expression_net` (positions 0-3) for a
    StemFused and its three pass-through stand-ins, or puts the very objects it replaced back.  Returns whether anything changed.  Off
    by default everywhere; opt-in, inference only.  What stays on PyTorch: the pools after `layer4` and the `fc`s (the 6DRepNet
    `rotation_net` has a switch of its own: native_rotation_net)."""
    changed = False
    for net in (getattr(emtn, "head_pose_net", None), getattr(emtn, "expression_net", None)):
        if isinstance(net, nn.Module):
            changed |= StemFused.swap(net, enable)
    return changed


def _is_repvgg_conv(m) -> bool:
    """The re-parameterised conv of a deploy-form RepVGG block: 3x3, padding 1, stride 1 or 2, any group count, with a bias."""
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride in ((1, 1), (2, 2)) and m.padding == (1, 1)
            and m.dilation == (1, 1) and m.padding_mode == "zeros" and m.bias is not None)


class RepVGGBlockFused(_FusedBlock2D):
    """A RepVGG block in deploy form — encoders2d._RepVGGDeployBlock, the reference's RepVGGBlock(deploy=True): `rbr_reparam`, one 3x3
    conv with a bias at stride 1 or 2, then ReLU (where the block has them, `se` is an nn.Identity and `nonlinearity` an nn.ReLU) — with an
    opt-in inference path on the matrix cores: ONE launch with bias and ReLU in its epilogue, f16x3 arithmetic (fp32-class accuracy):
    csrc/conv2d_s2_f16x3.hip at stride 2 (groups == 1 only), csrc/conv2d_f16x3.hip at groups == 1, csrc/conv2d_grp_f16x3.hip otherwise.
    The children are the original block's own, under their own names and in their own order: the same Parameter objects, the same
    state-dict keys, the same `named_modules()` names.  A block that still has its training branches (`rbr_dense`) is not matched.

    The native path runs only in eval mode, without autograd, on an fp32 module, a CUDA floating-point map and a supported shape
    (ops.conv2d_grouped_supported / conv2d_supported / conv2d_s2_supported); otherwise forward evaluates the original expression through
    the block's own children: on the CPU, in train mode, under autograd, on a .half() / .bfloat16() module and on a shape the kernels
    do not take (four groups at width 128: 32 output channels per group).  There are NO backward kernels and NO half_precision form.
    fp16 / bf16 inputs are widened and the result is fp32; a channels_last map is copied to NCHW once.  Each launch leaves the range
    descriptor of its output on the tensor, so only the first fused block of a net scans its input."""

    _EXPECTED = ("a deploy-form RepVGG block (`rbr_reparam`: Conv2d 3x3, padding 1, stride 1 or 2 (groups == 1 there), with a bias; `se` an "
                 "Identity and `nonlinearity` a ReLU where present; no `rbr_dense`; in_channels % 16 == 0)")
    _EVAL_ONLY = True
    _CUDA_FLOAT_INPUT = True
    split_small_maps = False   # set: the stride-1 launches pass splits="auto" (the split-K form where ops.conv2d_splits recommends it)

    def __init__(self, in_channels: int, out_channels: int, stride: int = 1, groups: int = 1):
        super().__init__()
        self.rbr_reparam = nn.Conv2d(in_channels, out_channels, 3, stride=stride, padding=1, groups=groups, bias=True)

    @classmethod
    def from_block(cls, block: nn.Module, half_precision: bool = False):
        if half_precision:
            raise TypeError("RepVGGBlockFused has no half_precision form")
        if not cls.matches(block):
            raise TypeError(f"{cls.__name__}.from_block: expected {cls._EXPECTED}, got {block}")
        new = cls.__new__(cls)
        nn.Module.__init__(new)
        for name, child in block._modules.items():   # (every child, in the block's order: named_modules() and state_dict() keep theirs)
            setattr(new, name, child)
        new.training = block.training
        return new

    @staticmethod
    def matches(block) -> bool:
        """Duck-typed: is `block` a deploy-form RepVGG block the fused path can stand in for?"""
        if isinstance(block, _FusedBlock2D) or not isinstance(block, nn.Module) or hasattr(block, "rbr_dense"):
            return False
        conv = getattr(block, "rbr_reparam", None)
        if not _is_repvgg_conv(conv) or (conv.stride == (2, 2) and conv.groups != 1):
            return False
        if conv.in_channels % 16:   # (no shape of such a block fits a kernel: layer0's 3 -> 64 conv stays the module it is)
            return False
        if set(block._modules) - {"rbr_reparam", "se", "nonlinearity"}:
            return False
        if hasattr(block, "se") and not isinstance(block.se, nn.Identity):
            return False
        return not hasattr(block, "nonlinearity") or isinstance(block.nonlinearity, nn.ReLU)

    def _shape_ok(self, x) -> bool:
        conv = self.rbr_reparam
        (n, ci, h, w), co, g = x.shape, conv.out_channels, conv.groups
        if ci != conv.in_channels or conv.weight.device != x.device:
            return False
        if conv.stride == (2, 2):
            return g == 1 and ops.conv2d_s2_supported(n, ci, co, h, w)
        return ops.conv2d_grouped_supported(n, ci, co, h, w, g)

    def _dtypes(self, half_path: bool):
        return {self.rbr_reparam.weight.dtype, self.rbr_reparam.bias.dtype}

    def _fold_tensors(self):
        return [self.rbr_reparam.weight, self.rbr_reparam.bias]

    def _fold(self, wide):
        return ops.PackedConv2d(self.rbr_reparam.weight, self.rbr_reparam.bias, self.rbr_reparam.groups)

    def _reference(self, x):
        y = self.rbr_reparam(x)
        if "nonlinearity" not in self._modules:
            return F.relu(y)   # encoders2d._RepVGGDeployBlock.forward
        return self.nonlinearity(self.se(y) if "se" in self._modules else y)

    def _launch(self, x, pack, out_dtype, products):
        xc = _f32(x).contiguous()   # (the kernels read NCHW: a channels_last map is copied once)
        if self.rbr_reparam.stride == (2, 2):
            return ops.conv2d_s2(xc, pack, relu=True, want_range=True)
        split = {"splits": "auto"} if self.split_small_maps else {}
        if pack.groups == 1:
            return ops.conv2d(xc, pack, relu=True, want_range=True, **split)
        return ops.conv2d_grouped(xc, pack, relu=True, want_range=True, **split)


def native_rotation_net(target, enable: bool = True, split_small_maps: bool = False) -> bool:
    """Swaps every matching deploy-form RepVGG block of the 6DRepNet backbone — `layer0` and the nn.Sequential stages `layer1..layer4` —
    for a RepVGGBlockFused over the same children, or puts the very objects it replaced back.  `target` is an Emtn (its `rotation_net`
    is looked up), a detector object with a `.model` (encoders2d.SixDRepNet_Detector, the reference's) or the backbone module itself.
    Returns whether anything changed.  Off by default everywhere; opt-in, inference only.  With RepVGG-B1g2 the 27 blocks of
    `layer1..layer4` are swapped; what stays on PyTorch: `layer0` (3 -> 64 at stride 2: Ci = 3 fits neither f16x3 kernel, so the block does not
    match and is left as it is), the global average pool, `linear_reg` and the Gram-Schmidt step.
    split_small_maps (off by default): the fused blocks' stride-1 plain and grouped convs ask ops.conv2d_splits for a split-K launch
    (csrc/conv2d_splitk_f16x3.hip); without the keyword every fused block is back on the unsplit kernels."""
    split = bool(enable and split_small_maps)
    net = getattr(target, "rotation_net", target)   # Emtn -> detector
    if not hasattr(net, "layer1"):
        net = getattr(net, "model", net)            # detector -> backbone
    if not isinstance(net, nn.Module):
        return False
    changed = False
    if isinstance(getattr(net, "layer0", None), nn.Module):
        new, changed = _swap_slot(RepVGGBlockFused, net.layer0, enable, False)
        if new is not net.layer0:
            net.layer0 = new
        if isinstance(new, RepVGGBlockFused):
            changed |= _set_split(new, split)
    for name in ("layer1", "layer2", "layer3", "layer4"):
        stage = getattr(net, name, None)
        if not isinstance(stage, nn.Sequential):
            continue
        for i in range(len(stage)):
            new, did = _swap_slot(RepVGGBlockFused, stage[i], enable, False)
            if new is not stage[i]:
                stage[i] = new
            if isinstance(new, RepVGGBlockFused):
                did |= _set_split(new, split)
            changed |= did
    return changed


def standardise_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv2d_WS.forward's weight (model.py:61-67): per output filter, minus its mean over dims 1-3, over (unbiased std + 1e-5)."""
    w = w - w.mean(dim=(1, 2, 3), keepdim=True)
    return w / (w.flatten(1).std(dim=1).view(-1, 1, 1, 1) + 1e-5)


def fold_resblock_custom(conv_res: nn.Module, conv_ws: nn.Module, conv: nn.Module, dtype: Optional[torch.dtype] = None):
    """ResBlock_Custom as two convs -> ((w_ws', b_ws), (w_cat, b_cat)) in the parameters' own dtype: conv_ws with its weight
    standardised, and conv(a) + conv_res(x) as ONE conv over the channel concatenation [a ; x]: w_cat = [W_conv | W_res] along dim 1,
    b_cat = b_conv + b_res.  dtype: the parameters are cast to it first (fp32 for a half block: the fold of its fp32 twin)."""
    cast = (lambda t: t.detach()) if dtype is None else (lambda t: t.detach().to(dtype))
    w_ws = standardise_weight(cast(conv_ws.weight)).contiguous()
    w_cat = torch.cat([cast(conv.weight), cast(conv_res.weight)], dim=1).contiguous()
    return (w_ws, cast(conv_ws.bias).contiguous()), (w_cat, (cast(conv.bias) + cast(conv_res.bias)).contiguous())


class ResBlockCustomFused(_FusedBlock2D):
    """Eapp's 2-D ResBlock_Custom (model.py:88-130)
        out = conv(relu(GN32(conv_ws(relu(GN32(x)))))) + conv_res(x)          GN32 = F.group_norm(., 32), no parameters
    with an opt-in path on the matrix cores: two launches of csrc/conv2d_gn_f16x3.hip (f16x3 arithmetic: fp32-class accuracy), each
    normalising its input while it stages it, the second one reading x as a second source so that the skip conv and the add cost no
    launch and no pass over memory (fold_resblock_custom).  The children are the original block's own `conv_res, conv_ws, conv` — the
    same Parameter objects, the same state-dict keys — built over an existing block by `from_block`.

    The native path runs without autograd (ag.needs_grad false) on an fp32 module, a CUDA input and a supported shape, in train and in
    eval mode alike (the block has no mode-dependent layer); otherwise forward evaluates the original block's expression in PyTorch.
    There are NO backward kernels and NO half-model path: training, fine-tuning and .half() / .bfloat16() instances take the PyTorch
    expression.  fp16 / bf16 inputs are widened (model._f32) and the result is fp32; channels_last inputs are copied to NCHW once.

    `from_block(block, half_precision=True)` adds the half-precision form (csrc/conv2d_lp.hip), with the contracts stated on
    ResBlock2DFused: inside torch.autocast('cuda', float16) an fp32 block runs one f16 product per multiply in both launches and returns
    float16; a .half() / .bfloat16() block folds its weights in fp32 from the widened parameters, runs one product and writes the
    model dtype.  A typed input is widened once (ops.cast_to_f32_range: the pass also delivers the descriptor of x the second launch
    needs); GroupNorm statistics and tables are taken on fp32 maps by their existing kernels, and `t` stays fp32."""

    _CHILDREN = ("conv_res", "conv_ws", "conv")
    _EXPECTED = "a 2-D ResBlock_Custom (conv_res, conv_ws (Conv2d_WS), conv: 3x3 stride-1 padding-1 convs with bias)"
    _CUDA_FLOAT_INPUT = True

    def __init__(self, dimension: int, in_channels: int, out_channels: int):
        super().__init__()
        from .encoders2d import Conv2d_WS

        if dimension != 2:
            raise NotImplementedError("ResBlockCustomFused: the 2-D block only")
        self.dimension, self.in_channels, self.out_channels = dimension, in_channels, out_channels
        self.conv_res = nn.Conv2d(in_channels, out_channels, 3, padding=1)
        self.conv_ws = Conv2d_WS(in_channels, out_channels, 3, padding=1)
        self.conv = nn.Conv2d(out_channels, out_channels, 3, padding=1)

    @staticmethod
    def matches(block) -> bool:
        """Duck-typed: is `block` a 2-D ResBlock_Custom (this package's or the reference's) the fused path can stand in for?"""
        if isinstance(block, ResBlockCustomFused) or getattr(block, "dimension", None) != 2:
            return False
        res, ws, conv = (getattr(block, n, None) for n in ("conv_res", "conv_ws", "conv"))
        if not (_is_conv2d(res, 3) and _is_conv2d(ws, 3) and _is_conv2d(conv, 3)) or type(ws).__name__ != "Conv2d_WS":
            return False
        ci, co = res.in_channels, res.out_channels
        return (ws.in_channels, ws.out_channels, conv.in_channels, conv.out_channels) == (ci, co, co, co)

    def _adopt(self, block):
        self.dimension, self.in_channels, self.out_channels = 2, block.conv_res.in_channels, block.conv_res.out_channels

    def _shape_ok(self, x) -> bool:
        (n, ci, h, w), co = x.shape, self.out_channels
        return ci == self.in_channels and ops.conv2d_cat_supported(n, ci, 0, co, h, w) and ops.conv2d_cat_supported(n, co, ci, co, h, w)

    def _dtypes(self, half_path: bool):
        return {p.dtype for p in self.parameters()}

    def _fold_tensors(self):
        return [t for m in (self.conv_res, self.conv_ws, self.conv) for t in (m.weight, m.bias)]

    def _fold(self, wide):
        """(conv_ws', [conv | conv_res]) packed."""
        ws, cat = fold_resblock_custom(self.conv_res, self.conv_ws, self.conv, wide)
        return ops.PackedConv2d(*ws), ops.PackedConv2d(*cat)

    def _reference(self, x):
        skip = self.conv_res(x)
        y = self.conv_ws(F.relu(F.group_norm(x, 32)))
        y = self.conv(F.relu(F.group_norm(y, 32)))
        return y + skip

    def _launch(self, x, packs, out_dtype, products):
        """Both launches, with the GroupNorm tables they stage through.  products None: the fp32 path; 0: the one-product path, whose
        typed input is widened by the pass that also delivers its descriptor."""
        p_ws, p_cat = packs
        # (NCHW: a channels_last map is copied once; an fp32 map is returned as it is by either)
        xc = _f32(x).contiguous() if products is None else ops.cast_to_f32_range(x.contiguous())
        tab, rng = ops.gn_relu_table2d(xc)
        t = ops.conv2d_cat(xc, p_ws, affine1=tab, relu1=True, x1_range=rng, products=products)
        tab, rng = ops.gn_relu_table2d(t)
        return ops.conv2d_cat(t, p_cat, x2=xc, affine1=tab, relu1=True, x1_range=rng, want_range=True, out_dtype=out_dtype, products=products)


_EAPP_TRUNK_SLOTS = ("resblock_128", "resblock_256", "resblock_512")


def native_eapp_trunk(eapp: nn.Module, enable: bool = True, half_precision: bool = False) -> bool:
    """Swaps every matching ResBlock_Custom among `eapp.resblock_128 / _256 / _512` (this package's Eapp or the reference's,
    model.py:210-212) for a ResBlockCustomFused over the same children, or puts the very objects it replaced back.  Returns whether
    anything changed.  Off by default everywhere.  half_precision: the blocks' half-precision form (ResBlockCustomFused); blocks that
    are fused already take the keyword's value."""
    changed = False
    for name in _EAPP_TRUNK_SLOTS:
        cur = getattr(eapp, name, None)
        new, did = _swap_slot(ResBlockCustomFused, cur, enable, half_precision)
        if new is not cur:
            setattr(eapp, name, new)
        changed |= did
    return changed


_RESNET50_STAGES = ("layer1", "layer2", "layer3")


def native_eapp_resnet50(eapp: nn.Module, enable: bool = True) -> bool:
    """Swaps every matching bottleneck of `eapp.custom_resnet50.layer1 / layer2 / layer3` (this package's Eapp or the reference's,
    model.py:136-173: thirteen blocks) for a BottleneckFused over the same children, or puts the very objects it replaced back.
    Returns whether anything changed.  Off by default everywhere; opt-in, inference only.  What stays on PyTorch: the adaptive pool,
    `conv_reduce` and Eapp's `fc`; the 7x7 stride-2 stem with its BatchNorm, ReLU and max-pool has a switch of its own
    (native_eapp_stems)."""
    net = getattr(eapp, "custom_resnet50", None)
    changed = False
    for name in _RESNET50_STAGES:
        stage = getattr(net, name, None)
        if not isinstance(stage, nn.Sequential):
            continue
        for i in range(len(stage)):
            new, did = _swap_slot(BottleneckFused, stage[i], enable, False)
            if new is not stage[i]:
                stage[i] = new
            changed |= did
    return changed


def _is_stem7_conv(m, stride: int) -> bool:
    """Conv2d(3, Co, 7, stride, padding=3) with Co a multiple of 16 up to 64: what csrc/conv2d_stem7_f16x3.hip computes."""
    return _is_conv2d_at(m, 7, stride) and m.in_channels == 3 and m.out_channels % 16 == 0 and 16 <= m.out_channels <= 64


def _stem7_input_ok(x, tensors, co: int, stride: int, pool: bool) -> bool:
    """The call conditions the two 7x7 stems share: fp32 parameters, a CUDA floating-point [N, 3, H, W] image on their device, a shape
    the kernel takes."""
    if {t.dtype for t in tensors} != {torch.float32}:
        return False
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_floating_point() and x.dim() == 4 and x.numel() > 0):
        return False
    n, ci, h, w = x.shape
    return ci == 3 and all(t.device == x.device for t in tensors) and ops.conv2d_stem7_supported(n, ci, co, h, w, stride, pool)


class ConvStem7Fused(_StemSlot):
    """`Eapp.conv`, Conv2d(3, 64, 7, stride=1, padding=3) with a bias at full resolution (model.py:209), as ONE launch of
    csrc/conv2d_stem7_f16x3.hip on the matrix cores (f16x3 arithmetic: fp32-class accuracy).  The result carries the range descriptor of
    its exact max|y|: ResBlockCustomFused's second launch, which reads this map as its second source, finds one (ops.current_range) and
    does not scan 64 channels at full resolution; the scan of the 3-channel image stays on the image, so Eapp's other stem does not repeat
    it.  Opt-in, inference only.  The Parameters are the conv's own, registered under their own names (_StemSlot): the same state-dict
    keys, the same `named_modules()` name; `native_eapp_stems(eapp, False)` puts the very conv back.

    The native path runs in eval mode, without autograd, on an fp32 conv, a CUDA image and a supported shape; an fp16 / bf16 image is
    widened, a channels_last one copied once, the result is fp32.  Otherwise the original conv runs: bit for bit on the CPU, in train
    mode, under autograd and on half modules."""

    def __init__(self, conv: nn.Module):
        super().__init__()
        self._take(conv, self)

    @staticmethod
    def matches(conv) -> bool:
        return _is_stem7_conv(conv, 1) and conv.bias is not None

    def _native_ok(self, x) -> bool:
        if self.training or ag.needs_grad(self, x):
            return False
        return _stem7_input_ok(x, [self._orig.weight, self._orig.bias], self._orig.out_channels, 1, False)

    def _pack(self):
        w, b = self._orig.weight, self._orig.bias
        hit = self.__dict__.get("_mphip_pack")
        if hit is None or hit.key != ops.PackedConv2dStem7.key_of(w, b) or ops.repacking():
            hit = self.__dict__["_mphip_pack"] = ops.PackedConv2dStem7(w, b)
        return hit

    def forward(self, x):
        if not self._native_ok(x):
            return self._orig(x)
        return ops.conv2d_stem7(_f32(x), self._pack(), stride=1, relu=False, pool=False, want_range=True)


class _Stem7Pass(_StemSlot):
    """The `bn1` and `maxpool` slots of a fused 7x7 stem.  Between them CustomResNet50.forward calls F.relu, not a module, so no mark on
    the tensor survives; the shape does.  Stem7Fused returns its pooled map as a 5-D view [1, N, C, Hp, Wp] carrying its mark: `bn1`
    hands a marked 5-D tensor through, F.relu keeps shape and bits (the map is >= +0 or NaN already), and `maxpool` turns a 5-D tensor
    with a leading 1 back into the 4-D view and puts the descriptor the head kept for a map of that shape on it.  nn.MaxPool2d raises
    on a 5-D input, so nothing else reaches that branch.  No tensor contents are compared and the device is not synchronised.  A 4-D
    tensor goes through the original module."""

    def __init__(self, orig: nn.Module, head: "Stem7Fused", last: bool):
        super().__init__()
        self._take(orig, head)
        self.__dict__["_last"] = last

    def forward(self, x):
        if isinstance(x, torch.Tensor) and x.dim() == 5 and x.shape[0] == 1:
            if not self._last:
                if x.__dict__.get("_mphip_stem7") is self._head:
                    return x
            else:
                kept = self._head.__dict__.pop("_mphip_kept", None)   # (used once: the descriptor of the launch this map came from)
                y = x[0]
                if kept is not None and kept[1] == tuple(y.shape) and kept[2] == y.device:
                    ops.tag_range(y, kept[0])
                return y
        return self._orig(x)


class Stem7Fused(_StemSlot):
    """The stem of Eapp's `custom_resnet50` (model.py:140-160): `conv1` (3 -> 64, 7x7, stride 2, padding 3, no bias) -> `bn1` -> F.relu ->
    `maxpool` (3, stride 2, padding 1), as ONE launch of csrc/conv2d_stem7_f16x3.hip: the BatchNorm folded into the conv (fold_batchnorm),
    bias, ReLU and the max-pool in the kernel's epilogue, the 64-channel half-resolution map never written.  `Stem7Fused.swap(net)` puts a
    Stem7Fused into the `conv1` slot and _Stem7Pass stand-ins into `bn1` and `maxpool`; `swap(net, False)` puts the very objects back.
    State-dict keys and their order, `named_modules()` names and the Parameter and buffer objects are the net's own; the net's forward is
    not touched.  The functional ReLU between `bn1` and `maxpool` still runs, over the pooled map (a sixteenth of the conv's map).

    The native path runs in eval mode, without autograd, on an fp32 module, a CUDA image and a supported shape; an fp16 / bf16 image is
    widened, a channels_last one copied once; the map entering `layer1` is fp32, 4-D and carries the range descriptor of its exact
    max|y|.  Otherwise this slot runs the original conv and returns a 4-D tensor, so the originals of the other slots run: the original
    expression, bit for bit."""

    _SLOTS = ("conv1", "bn1", "maxpool")

    def __init__(self, conv: nn.Module, bn: nn.Module, pool: nn.Module):
        super().__init__()
        self._take(conv, self)
        self.__dict__["_bn"], self.__dict__["_pool"] = bn, pool

    @classmethod
    def _find(cls, net):
        mods = [getattr(net, name, None) for name in cls._SLOTS] if isinstance(net, nn.Module) else [None]
        return mods if all(isinstance(m, nn.Module) for m in mods) else None

    @classmethod
    def matches(cls, net) -> bool:
        from torch.nn.modules.utils import _pair

        mods = cls._find(net)
        if mods is None or any(isinstance(m, _StemSlot) for m in mods):
            return False
        conv, bn, pool = mods
        if not (_is_stem7_conv(conv, 2) and _is_bn2d(bn, conv.out_channels)):
            return False
        return (isinstance(pool, nn.MaxPool2d) and _pair(pool.kernel_size) == (3, 3) and _pair(pool.stride) == (2, 2)
                and _pair(pool.padding) == (1, 1) and _pair(pool.dilation) == (1, 1) and not pool.ceil_mode and not pool.return_indices)

    @classmethod
    def swap(cls, net, enable: bool = True) -> bool:
        """Fuses the stem of `net` (matches) or, enable off, puts the three original modules back -> whether anything changed."""
        mods = cls._find(net)
        if mods is None:
            return False
        if enable:
            if not cls.matches(net):
                return False
            head = cls(*mods)
            for i, (name, m) in enumerate(zip(cls._SLOTS, mods)):
                setattr(net, name, head if i == 0 else _Stem7Pass(m, head, last=i == 2))
            return True
        changed = False
        for name, m in zip(cls._SLOTS, mods):
            if isinstance(m, (Stem7Fused, _Stem7Pass)):
                setattr(net, name, m._orig)
                changed = True
        return changed

    _fold_tensors = StemFused._fold_tensors

    def _native_ok(self, x) -> bool:
        if self.training or self._bn.training or ag.needs_grad(self, x) or ag.needs_grad(self._bn):
            return False
        return _stem7_input_ok(x, self._fold_tensors(), self._orig.out_channels, 2, True)

    def _pack(self):
        """The pack of fold_batchnorm(conv1, bn1), cached until a parameter or a running buffer changes (StemFused._folded's key)."""
        ts = self._fold_tensors()
        key = tuple((t.data_ptr(), t._version) for t in ts) + (str(ts[0].device), ops.weight_epoch())
        hit = self.__dict__.get("_mphip_fold")
        if hit is None or hit[0] != key or ops.repacking():
            with torch.no_grad():
                hit = (key, ops.PackedConv2dStem7(*fold_batchnorm(self._orig, self._bn)))
            self.__dict__["_mphip_fold"] = hit
        return hit[1]

    def forward(self, x):
        if not self._native_ok(x):
            return self._orig(x)   # 4-D: bn1 and maxpool run as the modules they are
        y = ops.conv2d_stem7(_f32(x), self._pack(), stride=2, relu=True, pool=True, want_range=True)
        self.__dict__["_mphip_kept"] = (ops.tensor_range(y), tuple(y.shape), y.device)
        y5 = y.unsqueeze(0)
        y5._mphip_stem7 = self   # bn1 hands it through; F.relu drops the mark and keeps the shape, which maxpool recognises
        return y5


def native_eapp_stems(eapp: nn.Module, enable: bool = True) -> bool:
    """Swaps the two 7x7 convs that read Eapp's source image (this package's Eapp or the reference's, model.py:209 and 140-160) for their
    matrix-core forms, or puts the very objects it replaced back: `eapp.conv` becomes a ConvStem7Fused, and the stem `conv1, bn1, maxpool`
    of `eapp.custom_resnet50` a Stem7Fused with its two stand-ins.  Returns whether anything changed.  Off by default everywhere; opt-in,
    inference only; independent of native_eapp_trunk and native_eapp_resnet50.  What stays on PyTorch in Eapp's 2-D part: the average and
    adaptive pools, `conv_1`, `conv_reduce`, `fc`, and the functional ReLU over the pooled stem map."""
    changed = False
    conv = getattr(eapp, "conv", None)
    if enable and ConvStem7Fused.matches(conv):
        eapp.conv = ConvStem7Fused(conv)
        changed = True
    elif not enable and isinstance(conv, ConvStem7Fused):
        eapp.conv = conv._orig
        changed = True
    net = getattr(eapp, "custom_resnet50", None)
    if isinstance(net, nn.Module):
        changed |= Stem7Fused.swap(net, enable)
    return changed


class _HotSliceRunner(_ModelDtype):
    """model.py:1151-1171 over `self.warp_generator_s2c`, `self.warp_generator_c2d`, `self.G3d` — shared by
    GbaseHotSlice (the slice alone) and gbase.Gbase (the orchestrator)."""

    # The C2D generator depends only on (Rd, td, zd, es): its ~25 small, latency-bound launches run on
    # a second HIP stream underneath G3d's MFMA-bound kernels instead of in front of the last warp.
    overlap_generators = True
    # Frames per pass of the slice: the conv kernels address their input through one 2 GiB buffer resource (a [B,96,16,64,64]
    # volume is 25 MB per frame: 85 frames); larger batches run as consecutive passes of this many frames (frames are
    # independent: same results).  Under autograd the batch is not split (a training batch of that size does not fit anyway).
    max_frames_per_pass = 64

    def _side_stream(self, main):
        """One helper stream per caller stream (callers may keep several batches in flight on their own streams)."""
        table = self.__dict__.setdefault("_side_streams", {})
        key = (main.device, main.cuda_stream)
        st = table.get(key)
        if st is None:
            st = table[key] = torch.cuda.Stream(device=main.device)
        return st

    # Inference goes through the C-side plan (csrc/plan.hip, include/mphip.h "one-call entries"): ONE ctypes call per step
    # issues the same launches in the same order as `_run_python` below (bitwise identical results, tests/test_gpu_plan.py);
    # a single frame is launch-bound and the ~135 Python/ctypes round trips cost more than the kernels.  MPHIP_C_PLAN=0 or
    # `use_c_plan = False` selects the per-op schedule (also taken under autograd and when a measurement hook is installed).
    use_c_plan = os.environ.get("MPHIP_C_PLAN", "1") != "0"
    # G3d's last upsample + conv only where the final warp reads them (MPHIP_FULL_FINAL_CONV=1: everywhere; same output bits)
    full_final_conv = os.environ.get("MPHIP_FULL_FINAL_CONV", "0") == "1"

    def _plan_for(self, vs):
        from . import plan as _plan

        # one plan per caller stream: a plan owns ONE side stream and one fork/join event pair, so callers that keep several batches in
        # flight on several streams get independent generator lanes (and their own packed weights: ~230 MB per plan)
        shape_key = (tuple(vs.shape[1:]), vs.device, bool(self.overlap_generators), bool(self.full_final_conv))
        key = shape_key + (torch.cuda.current_stream(vs.device).cuda_stream,)
        table = self.__dict__.setdefault("_plans", {})
        if torch.cuda.is_current_stream_capturing():
            # torch.cuda.graph() switches to its own capture stream: a plan made HERE would hipMalloc, copy tables synchronously and pack
            # weights inside the capture (illegal, or recorded into every replay).  Take the plan that was warmed up for this shape —
            # its launches go to whatever stream is current — and refuse to build one while capturing.  
            for k in reversed(list(table)):
                if k[:len(shape_key)] == shape_key:
                    return table[k]
            raise RuntimeError("GbaseHotSlice: no warmed-up plan for this shape while a stream is capturing — run one forward of the same "
                               "shape before torch.cuda.graph() (model.GraphedHotSlice does)")
        pl = table.pop(key, None)
        if pl is None:
            pl = _plan.HotSlicePlan(self, dims=tuple(vs.shape[1:]), single_stream=not self.overlap_generators,
                                    full_final_conv=self.full_final_conv)
        table[key] = pl   # (most recently used last)
        while len(table) > self._MAX_PLANS:   # a caller that keeps making new streams must not keep every plan's packed weights
            torch.cuda.synchronize(vs.device)
            table.pop(next(iter(table))).close()
        return pl

    _MAX_PLANS = 6

    _HOT_CHILDREN = ("warp_generator_s2c", "warp_generator_c2d", "G3d")
    _TWIN_FLAGS = ("use_c_plan", "overlap_generators", "full_final_conv", "max_frames_per_pass")

    def _run(self, vs, es, Rs, ts, zs, Rd, td, zd, check_shape: bool):
        dt = model_dtype(self)
        if dt != torch.float32:
            return self._run_typed(dt, vs, es, Rs, ts, zs, Rd, td, zd, check_shape)
        return self._run_f32(vs, es, Rs, ts, zs, Rd, td, zd, check_shape)

    def _hot_twin(self):
        """fp32 twin of the hot slice alone (gbase.Gbase's 2-D modules are not copied): a bare GbaseHotSlice over fp32 copies."""
        twin = GbaseHotSlice.__new__(GbaseHotSlice)
        nn.Module.__init__(twin)
        pairs = []
        for name in self._HOT_CHILDREN:
            src = getattr(self, name)
            setattr(twin, name, _fp32_copy(src))
            pairs += list(zip(src.parameters(), getattr(twin, name).parameters()))
        return twin, pairs

    def _run_typed(self, dt, vs, es, Rs, ts, zs, Rd, td, zd, check_shape: bool):
        """A half model (see model_dtype): the fp32 twin under the single-product conv policy; K2 reads vs in its own dtype, K3 writes the
        projection in the model dtype."""
        _refuse_half_training(self, dt, vs, es, Rs, ts, zs, Rd, td, zd)
        twin = _twin(self, self._hot_twin)
        for k in self._TWIN_FLAGS:
            twin.__dict__[k] = getattr(self, k)
        with ops.half_products(True):
            return twin._run_f32(vs, es, Rs, ts, zs, Rd, td, zd, check_shape, out_dtype=dt)

    @_autocast_policy
    def _run_f32(self, vs, es, Rs, ts, zs, Rd, td, zd, check_shape: bool, out_dtype=None):
        """out_dtype (a half model's twin): vs may stay fp16/bf16 — K2 reads it directly — and the result is written in out_dtype."""
        typed = out_dtype is not None and isinstance(vs, torch.Tensor) and vs.dtype in _HALF
        es, Rs, ts, zs, Rd, td, zd = _f32(es, Rs, ts, zs, Rd, td, zd)
        vs = vs if typed else _f32(vs)
        if (self.use_c_plan and vs.shape[0] > 0 and vs.dim() == 5 and vs.shape[1] == 96 and ops._conv_hook is None
                and ops._GNIN_ENABLED and ops._GN_SMALL_ENABLED and ops._RANGES_ENABLED   # (dev A/B switches act on the per-op path)
                and not ag.needs_grad(self, vs, es, Rs, ts, zs, Rd, td, zd)
                and all(v % 8 == 0 for v in vs.shape[2:])):
            if check_shape:
                assert vs.shape[1:] == (96, 16, 64, 64), f"Expected vc shape (_, 96, 16, 64, 64), got {vs.shape}"
            if out_dtype is not None:
                return self._plan_for(vs).forward(vs, es, Rs, ts, zs, Rd, td, zd, out_dtype=out_dtype)
            return self._plan_for(vs).forward(vs, es, Rs, ts, zs, Rd, td, zd)
        return self._run_python(vs, es, Rs, ts, zs, Rd, td, zd, check_shape, out_dtype)

    def _run_python(self, vs, es, Rs, ts, zs, Rd, td, zd, check_shape: bool, out_dtype=None):
        typed = out_dtype is not None and isinstance(vs, torch.Tensor) and vs.dtype in _HALF
        es, Rs, ts, zs, Rd, td, zd = _f32(es, Rs, ts, zs, Rd, td, zd)
        vs = vs if typed else _f32(vs)
        if vs.shape[0] == 0:  # an empty frame shard (dp.shard_inputs with more ranks than frames): nothing to launch
            out = vs.new_zeros((0, vs.shape[1]) + tuple(vs.shape[3:]), dtype=out_dtype or torch.float32)
            if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                # training: stay connected to the parameters (zero gradients), so this rank's loss.backward() runs and it
                # enters the gradient all-reduce with the others instead of leaving them blocked in the collective
                # (multiply-free: `p.sum() * 0` would turn one Inf/NaN weight into a NaN loss on this rank and, through the
                #  all-reduce, on every rank; an empty slice sums to an exact 0 with zero gradients and launches no reduction)
                out = out + sum(p.reshape(-1)[:0].sum() for p in self.parameters() if p.requires_grad)
            return out
        train = ag.needs_grad(self, vs, es, Rs, ts, zs, Rd, td, zd)
        if not train and vs.shape[0] > self.max_frames_per_pass:
            step = int(self.max_frames_per_pass)
            return torch.cat([self._run_python(*(t[i:i + step] for t in (vs, es, Rs, ts, zs, Rd, td, zd)), check_shape, out_dtype)
                              for i in range(0, vs.shape[0], step)], dim=0)
        main = torch.cuda.current_stream(vs.device)
        # training: one stream (autograd replays each op's backward on its forward stream; the overlap is an inference trick)
        side = self._side_stream(main) if (self.overlap_generators and not train) else None
        if side is not None:
            side.wait_stream(main)  # inputs produced on the main stream are visible
        # Critical path first, in HOST order too: S2C, warp #1 and G3d's first (0.6 ms) conv are launched before the host
        # spends its ~0.3 ms issuing the C2D generator's ~25 launches on the side stream.  Issued earlier, they leave the
        # main stream idle between S2C and warp #1 whenever the host is not running ahead (first step, profiled runs);
        # in the steady-state throughput loop the host is ahead anyway and the order is worth +0.3 % only.
        w_s2c = self.warp_generator_s2c(Rs, ts, zs, es)
        c2d = {}

        def issue_c2d():
            with torch.cuda.stream(side):
                c2d["w"] = self.warp_generator_c2d(Rd, td, zd, es)

        early = side is not None and _C2D_EARLY  # dev switch: the old issue order, for same-box A/B runs
        if early:
            issue_c2d()
        vc = ops.warp_volume(vs, w_s2c) if typed else apply_warping_field(vs, w_s2c)   # (typed: K2 reads the half volume)
        if check_shape:
            assert vc.shape[1:] == (96, 16, 64, 64), f"Expected vc shape (_, 96, 16, 64, 64), got {vc.shape}"
        roi = None
        if train and not self.full_final_conv and isinstance(self.G3d, G3d):
            # training: the final warp reads (and sends gradient to) only the voxels inside its sample boxes — final_conv's
            # forward is evaluated there (the C-side plan does the same at inference); backward kernels unchanged
            c2d["w"] = self.warp_generator_c2d(Rd, td, zd, es)
            with torch.no_grad():
                roi = ops.warp_sample_box(ops.warp_coords(c2d["w"].detach(), *vc.shape[2:]))
        vc2d = self.G3d(vc, _after_first_conv=issue_c2d if (side is not None and not early) else None, **({"_final_roi": roi} if roi is not None else {}))
        if side is not None:
            w_c2d = c2d["w"]
            main.wait_stream(side)
            w_c2d.record_stream(main)
        elif "w" in c2d:
            w_c2d = c2d["w"]
        else:
            w_c2d = self.warp_generator_c2d(Rd, td, zd, es)
        # apply_warping_field + torch.sum(dim=2) (model.py:1167-1171) in one kernel (K3)
        if train:
            return ag.WarpVolumeFn.apply(vc2d, w_c2d, True)
        if out_dtype is not None:
            return ops.warp_volume_dsum(vc2d, w_c2d, out_dtype=out_dtype)
        return ops.warp_volume_dsum(vc2d, w_c2d)



class GbaseHotSlice(_HotSliceRunner, nn.Module):
    """The slice of Gbase.forward between the 2D encoders and G2d (model.py:1151-1171), with the
    reference's attribute names so a Gbase checkpoint's `warp_generator_s2c.*`,
    `warp_generator_c2d.*` and `G3d.*` keys load unchanged."""

    def __init__(self):
        super().__init__()
        self.warp_generator_s2c = WarpGeneratorS2C(num_channels=512)
        self.warp_generator_c2d = WarpGeneratorC2D(num_channels=512)
        self.G3d = G3d(in_channels=96)

    def forward(self, vs, es, Rs, ts, zs, Rd, td, zd):
        return self._run(vs, es, Rs, ts, zs, Rd, td, zd, True)

    def forward_any_size(self, vs, es, Rs, ts, zs, Rd, td, zd):
        """Same graph without the 512^2-only shape assert (small parity cases)."""
        return self._run(vs, es, Rs, ts, zs, Rd, td, zd, False)


class GraphedHotSlice:
    """Replays the hot slice as one hipGraph: the ~130 stream-ordered launches of a step (two streams) are
    captured once for fixed input shapes and re-launched with a single hipGraphLaunch, which removes the
    per-launch host cost (Python + ctypes + hipLaunchKernel ~ 15 us each) from the critical path.
    Inputs are copied into static buffers; the output tensor is reused between calls."""

    def __init__(self, hot: "GbaseHotSlice", example_inputs: dict, any_size: bool = False, warmup: int = 2):
        self.hot = hot
        self.static_in = {k: v.clone() for k, v in example_inputs.items()}
        fn = hot.forward_any_size if any_size else hot.forward
        with torch.no_grad():
            side = torch.cuda.Stream(device=next(iter(example_inputs.values())).device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):       # warm up off the default stream (packs weights, fills caches)
                for _ in range(warmup):
                    fn(**self.static_in)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph(keep_graph=True)
            ops.begin_capture()   # range descriptors measured on the warm-up batch are not frozen into the graph
            with torch.cuda.graph(self.graph):
                self.static_out = fn(**self.static_in)
            self.memset_nodes_replaced = ops.finish_graph_capture(self.graph)   # (memset nodes -> kernel nodes, then instantiate)

    def __call__(self, **inputs):
        for k, v in inputs.items():
            if v.data_ptr() != self.static_in[k].data_ptr():
                self.static_in[k].copy_(v)
        self.graph.replay()
        return self.static_out


def load_hot_state_dict(module: nn.Module, state_dict, strict: bool = True):
    """Loads a (sub)set of a reference Gbase state-dict.  Reference checkpoints built on a GPU host
    lack `adaptive_matrix_gamma/beta` (model.py:934-935 quirk): those keys are then left at their
    current values and reported."""
    own = module.state_dict()
    filtered = {k: v for k, v in state_dict.items() if k in own}
    missing = [k for k in own if k not in filtered]
    tolerated = [k for k in missing if "adaptive_matrix_" in k]
    hard_missing = [k for k in missing if k not in tolerated]
    if strict and hard_missing:
        raise KeyError(f"missing keys: {hard_missing[:8]}{'...' if len(hard_missing) > 8 else ''}")
    module.load_state_dict(filtered, strict=False)
    if tolerated:
        logging.warning("checkpoint has no %s (GPU-built reference model); kept current values", tolerated)
    return hard_missing, tolerated
