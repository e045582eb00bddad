"""`Gbase` — the orchestrator at the drop-in boundary (reference model.py:1127-1180).

Same attribute names as the reference (`appearanceEncoder, motionEncoder, warp_generator_s2c, warp_generator_c2d, G3d,
G2d, image_pyramid` — model.py:1130-1137) and therefore the same state-dict keys; `forward(xs, xd)` returns
`(xhat_base [B,3,512,512], {'prediction_0.5': ..., 'prediction_0.25': ...})` like model.py:1180, so `train.py:194,283`
(`pred, pyramids = Gbase(src, drv)`), `PairwiseTransferLoss` (model.py:2192-2214: sub-module calls) and a fixed
`inference.py` drop in.

Hot path (model.py:1151-1171) = the HIP kernels, through model._HotSliceRunner; Eapp's 3D tail and G2d's entry are the
HIP rows f1/f3; everything else is PyTorch-ROCm (encoders2d.py, or whatever modules the caller injects).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import encoders2d as E
from . import model as M


class Gbase(M._HotSliceRunner, nn.Module):
    """model.py:1127-1180.  `Gbase()` (no arguments, like the reference) builds this repo's own 2D modules with random
    init — the reference's constructor downloads weights and calls `.cuda(0)`.  Pass
    `appearanceEncoder` / `motionEncoder` / `G2d` / `image_pyramid` to inject other modules (any nn.Module with the
    reference's forward signature)."""

    def __init__(self, appearanceEncoder: Optional[nn.Module] = None, motionEncoder: Optional[nn.Module] = None,
                 G2d: Optional[nn.Module] = None, image_pyramid: Optional[nn.Module] = None):
        super().__init__()
        self.appearanceEncoder = appearanceEncoder if appearanceEncoder is not None else E.Eapp()
        self.motionEncoder = motionEncoder if motionEncoder is not None else E.Emtn()
        self.warp_generator_s2c = M.WarpGeneratorS2C(num_channels=512)
        self.warp_generator_c2d = M.WarpGeneratorC2D(num_channels=512)
        self.G3d = M.G3d(in_channels=96)
        self.G2d = G2d if G2d is not None else E.G2d(in_channels=96)
        self.image_pyramid = image_pyramid if image_pyramid is not None else E.ImagePyramide(scales=[0.5, 0.25], num_channels=3)

    def channels_last_2d(self, enable: bool = True) -> "Gbase":
        """Memory format of the PyTorch-ROCm 2D modules on the driver-side path: `motionEncoder` and `G2d` in
        torch.channels_last (MIOpen's NHWC kernels: 73 -> 62 ms per 8 frames under autocast-fp16, 147 -> 142 ms in fp32 on
        MI355X — with MIOpen's find mode, `torch.backends.cudnn.benchmark = True`; in immediate mode NHWC measures SLOWER
        (101 vs 110 frames/s), so set that flag with it.  Eapp's trunk measures slower in NHWC and is left alone).  A layout
        choice only: same parameters, same state-dict keys, results equal up to MIOpen's kernel selection."""
        self._cl2d = bool(enable)
        fmt = torch.channels_last if enable else torch.contiguous_format
        for m in (self.motionEncoder, self.G2d):
            for t in list(m.parameters()) + list(m.buffers()):
                if t.dim() == 4:
                    t.data = t.data.contiguous(memory_format=fmt)
        return self

    def native_final_conv(self, enable: bool = True) -> "Gbase":
        """Opt-in (off by default): `G2d.final_conv` — GroupNorm-ReLU-conv-sigmoid on the [B,64,512,512] map — as the fused HIP
        kernels of model.G2dFinalConv; `enable=False` restores the original nn.Sequential.  Same parameters and state-dict keys.
        With channels_last_2d() the map reaches the kernels in NHWC and is copied to NCHW first."""
        M.native_final_conv(self.G2d, enable)
        return self

    def native_body(self, enable: bool = True, half_precision: bool = False, fuse_upsample: bool = False, trainable: bool = False) -> "Gbase":
        """Opt-in (off by default; inference, and training with trainable=True): G2d's ResBlock2D body as model.ResBlock2DFused — BatchNorm folded, 3x3 convs on the
        matrix cores (model.native_g2d_body); `enable=False` restores the original blocks.  Same parameters and state-dict keys.
        half_precision (off by default): the blocks' one-product form for autocast(float16) regions and half models.
        fuse_upsample (off by default): the three up-sampling stages fold their bilinear x2 up-sample into the block's convs
        (model.Up2ResBlock2DFused); with half_precision=True they keep the materialised up-sample.
        trainable (off by default): under autograd the fused blocks run forward and backward on the matrix cores (ag.Conv2dFn), fp32
        outside autocast only; with fuse_upsample an up-sampling stage under autograd runs its nn.Upsample in PyTorch, then the block."""
        M.native_g2d_body(self.G2d, enable, half_precision, fuse_upsample, trainable)
        return self

    def native_trunk(self, enable: bool = True, half_precision: bool = False) -> "Gbase":
        """Opt-in (off by default), inference only: the three ResBlock_Custom of the appearance encoder's 2-D trunk as
        model.ResBlockCustomFused — GroupNorm, ReLU and the skip conv folded into two matrix-core conv launches per block
        (model.native_eapp_trunk); `enable=False` restores the original blocks.  Same parameters and state-dict keys.
        half_precision (off by default): the blocks' one-product form for autocast(float16) regions and half models."""
        M.native_eapp_trunk(self.appearanceEncoder, enable, half_precision)
        return self

    def native_resnet50(self, enable: bool = True) -> "Gbase":
        """Opt-in, inference only: run the thirteen bottlenecks of the appearance encoder's `custom_resnet50` (the identity descriptor
        `es`) on the matrix cores (model.native_eapp_resnet50); `enable=False` restores the original blocks.  Same parameters and
        state-dict keys."""
        M.native_eapp_resnet50(self.appearanceEncoder, enable)
        return self

    def native_stems(self, enable: bool = True) -> "Gbase":
        """Opt-in, inference only: run the appearance encoder's two 7x7 stems (`conv`, and `custom_resnet50`'s conv1-bn1-relu-maxpool)
        on the matrix cores, one launch each (model.native_eapp_stems); `enable=False` restores the original modules.  Same parameters
        and state-dict keys."""
        M.native_eapp_stems(self.appearanceEncoder, enable)
        return self

    def native_motion_encoder(self, enable: bool = True, fuse_stem: bool = False, rotation_net: bool = False,
                              split_small_maps: bool = False) -> "Gbase":
        """Opt-in (off by default), inference only: the BasicBlocks of the motion encoder's two ResNet-18s (`head_pose_net`,
        `expression_net`) as model.BasicBlockFused — BatchNorm folded, 3x3 convs on the matrix cores, the stride-2 ones included
        (model.native_emtn_resnets); `enable=False` restores the original blocks.  Same parameters and state-dict keys.
        fuse_stem (off by default): each net's 3->64 stem (conv, BatchNorm, ReLU, max-pool) as one exact-fp32 launch (model.StemFused;
        model.native_emtn_stems); without it, or with enable off, the four original modules are back.
        rotation_net (off by default): the 27 deploy-form RepVGG blocks of the frozen 6DRepNet's `layer1..layer4` as one matrix-core
        launch each, the groups = 2 ones on the grouped kernel (model.RepVGGBlockFused; model.native_rotation_net); without it, or
        with enable off, the original blocks are back.  The pools, the `fc`s, and of the 6DRepNet `layer0`, the pool and `linear_reg`
        stay on PyTorch.  With channels_last_2d() the image and a block's input map are copied to NCHW once.
        split_small_maps (off by default): the stride-1 convs of every block fused here take the split-K launch where the library
        recommends one (ops.conv2d_splits; csrc/conv2d_splitk_f16x3.hip); without it they are back on the unsplit kernels."""
        M.native_emtn_resnets(self.motionEncoder, enable, split_small_maps)
        M.native_emtn_stems(self.motionEncoder, bool(enable and fuse_stem))
        M.native_rotation_net(self.motionEncoder, bool(enable and rotation_net), split_small_maps)
        return self

    def _nhwc(self, x):
        return x.contiguous(memory_format=torch.channels_last) if getattr(self, "_cl2d", False) and x.dim() == 4 else x

    def hot_slice(self, vs, es, Rs, ts, zs, Rd, td, zd, check_shape: bool = True):
        """model.py:1151-1171 on already-encoded inputs -> projected features [B,96,H,W] (what GbaseHotSlice computes)."""
        return self._run(vs, es, Rs, ts, zs, Rd, td, zd, check_shape)

    def encode(self, xs, xd):
        """model.py:1141-1145: (vs, es, Rs, ts, zs, Rd, td, zd)."""
        vs, es = self.appearanceEncoder(xs)
        Rs, ts, zs = self.motionEncoder(self._nhwc(xs))
        Rd, td, zd = self.motionEncoder(self._nhwc(xd))
        return vs, es, Rs, ts, zs, Rd, td, zd

    def forward(self, xs, xd):
        vs, es, Rs, ts, zs, Rd, td, zd = self.encode(xs, xd)
        vc2d_projected = self._run(vs, es, Rs, ts, zs, Rd, td, zd, True)   # asserts the 96x16x64x64 volume (model.py:1157,1168)
        xhat_base = self.G2d(self._nhwc(vc2d_projected))
        return xhat_base, self.image_pyramid(xhat_base)

    def forward_any_size(self, xs, xd):
        """Same graph without the 512^2-only asserts (BASELINE config 1: 256x256 frames; small parity cases)."""
        vs, es, Rs, ts, zs, Rd, td, zd = self.encode(xs, xd)
        xhat_base = self.G2d(self._nhwc(self._run(vs, es, Rs, ts, zs, Rd, td, zd, False)))
        return xhat_base, self.image_pyramid(xhat_base)

    @torch.no_grad()
    def reenact(self, xs, xd, chunk: int = 16, rank: int = 0, world: int = 1, fp16: bool = False):
        """BASELINE config 5: ONE source image x N driver frames -> images [n_local,3,H,W] of this rank's driver shard.
        The source-side half (Eapp, Emtn(xs), S2C field, warp #1, G3d: model.py:1141-1160) runs once; per driver chunk
        only Emtn(xd), the C2D field, the fused warp + depth sum and G2d run (model.py:1145,1163-1174).  Results equal
        calling forward() on every (source, driver) pair.

        fp16 (config 5's "fp16"): the reference's own reduced-precision policy is `torch.cuda.amp.autocast()` around the
        generator (train.py:188).  Here that region covers the PyTorch-ROCm 2D modules (Emtn and G2d's body are the whole
        per-driver cost: G3d runs once per SOURCE).  The HIP kernels take fp32 at the boundary (model._f32) and keep fp32 between
        kernels; inside the region G3d's F(2,3) convs follow the reference's autocast arithmetic — one f16 product per multiply, fp32
        accumulation (model._autocast_policy) — everything else on the HIP side computes as without it."""
        from . import dp, ops

        if xs.shape[0] != 1:
            raise ValueError("reenact expects a single source image [1,3,H,W]")
        import contextlib

        # a half model (model.model_dtype): the hot slice runs on its fp32 twin with typed boundaries, exactly as forward() does it
        dt = M.model_dtype(self)
        hot = self if dt == torch.float32 else M._twin(self, self._hot_twin)
        policy = ops.half_products(True) if dt != torch.float32 else contextlib.nullcontext()
        with torch.autocast(device_type="cuda", dtype=torch.float16, enabled=bool(fp16)), policy:
            vs, es = self.appearanceEncoder(xs)
            Rs, ts, zs = self.motionEncoder(self._nhwc(xs))
            w_s2c = hot.warp_generator_s2c(Rs, ts, zs, es)
            vc2d = hot.G3d(ops.warp_volume(vs, w_s2c) if dt != torch.float32 else M.apply_warping_field(vs, w_s2c))
            b, e = dp.shard_range(xd.shape[0], rank, world)
            outs = []
            for i in range(b, e, chunk):
                j = min(e, i + chunk)
                Rd, td, zd = self.motionEncoder(self._nhwc(xd[i:j]))
                w_c2d = hot.warp_generator_c2d(Rd, td, zd, es.float().expand(j - i, -1).contiguous())
                proj = ops.warp_volume_dsum(vc2d, w_c2d) if dt == torch.float32 else ops.warp_volume_dsum(vc2d, w_c2d, out_dtype=dt)
                outs.append(self.G2d(self._nhwc(proj)).float().contiguous())
        return torch.cat(outs, dim=0) if outs else xs.new_zeros((0,) + tuple(xs.shape[1:]))
