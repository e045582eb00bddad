"""In-place installation of the HIP hot path into an existing reference model (the drop-in boundary).

The reference's `Gbase.forward` (model.py:1140-1180) reaches the hot path through three sub-modules
(`warp_generator_s2c`, `warp_generator_c2d`, `G3d`), the module-level function `apply_warping_field`, and — row f1 —
the `resblock3D_*` blocks of `appearanceEncoder` (model.py:217-226).  `install(gbase, model_module)` swaps exactly
those for the classes of `megaportrait_hack_amd.model` (same names, state-dict keys and forward signatures), carrying
over parameters, device and train/eval mode; everything else (Eapp's 2D trunk, Emtn, G2d, losses, the training loop)
stays the reference's own PyTorch code, as north_star prescribes.  Nothing here computes: it is module plumbing.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from . import model as M

_EAPP_TAIL_BLOCKS = ("resblock3D_96", "resblock3D_96_1", "resblock3D_96_1_2", "resblock3D_96_2", "resblock3D_96_2_2")


def _carry_over(old: nn.Module, new: nn.Module) -> nn.Module:
    own = new.state_dict()
    src = {k: v for k, v in old.state_dict().items() if k in own}
    # a GPU-built reference generator holds adaptive_matrix_* as plain tensors (model.py:934-935: Parameter(...).to(device)
    # is not a Parameter), so they are missing from its state_dict but present as attributes
    for name in ("adaptive_matrix_gamma", "adaptive_matrix_beta"):
        if name in own and name not in src and isinstance(getattr(old, name, None), torch.Tensor):
            src[name] = getattr(old, name).detach()
    missing = [k for k in own if k not in src]
    if missing:
        raise KeyError(f"{type(old).__name__} does not provide {missing[:4]}{'...' if len(missing) > 4 else ''}")
    new.load_state_dict(src, strict=True)
    ref = next(iter(old.parameters()), None)
    if ref is not None:
        new.to(ref.device)
    new.train(old.training)
    return new


def swap_hot_path(gbase: nn.Module, eapp_tail: bool = True) -> List[str]:
    """Replaces, in place, gbase.warp_generator_s2c / warp_generator_c2d / G3d (and, with eapp_tail, the five
    ResBlock3D_Adaptive(96,96) blocks of gbase.appearanceEncoder) by their HIP-backed equivalents.  Returns the
    attribute paths that were swapped.  Optimizers created before the swap hold the OLD parameters: build them after."""
    done = []
    for name, ctor in (("warp_generator_s2c", lambda: M.WarpGeneratorS2C(num_channels=512)),
                       ("warp_generator_c2d", lambda: M.WarpGeneratorC2D(num_channels=512)),
                       ("G3d", lambda: M.G3d(in_channels=96))):
        old = getattr(gbase, name, None)
        if old is None:
            raise AttributeError(f"{type(gbase).__name__} has no attribute {name!r} (expected a reference Gbase, model.py:1127-1137)")
        if isinstance(old, (M.WarpGeneratorS2C, M.WarpGeneratorC2D, M.G3d)):
            continue  # already installed
        setattr(gbase, name, _carry_over(old, ctor()))
        done.append(name)
    enc = getattr(gbase, "appearanceEncoder", None)
    if eapp_tail and enc is not None:
        for name in _EAPP_TAIL_BLOCKS:
            old = getattr(enc, name, None)
            if old is None or isinstance(old, M.ResBlock3D_Adaptive):
                continue
            setattr(enc, name, _carry_over(old, M.ResBlock3D_Adaptive(in_channels=96, out_channels=96)))
            done.append("appearanceEncoder." + name)
    return done


def patch_functions(model_module) -> List[str]:
    """Points the reference module's hot-path functions (looked up as globals by Gbase.forward and
    PairwiseTransferLoss, model.py:1155,1167,2203) at the HIP implementations."""
    done = []
    for name in ("apply_warping_field", "compute_rt_warp"):
        if hasattr(model_module, name):
            setattr(model_module, name, getattr(M, name))
            done.append(name)
    return done


def install(gbase: nn.Module, model_module: Optional[object] = None, eapp_tail: bool = True, g2d_final: bool = False,
            g2d_body: bool = False, eapp_trunk: bool = False, half_precision: bool = False, fuse_upsample: bool = False,
            motion_encoder: bool = False, fuse_stem: bool = False, rotation_net: bool = False,
            split_small_maps: bool = False, eapp_stems: bool = False) -> List[str]:
    """swap_hot_path + patch_functions.  `model_module` is the imported reference `model` module (the one that defines
    Gbase); pass it so the two `apply_warping_field` call sites inside Gbase.forward use the HIP kernel too.
    g2d_final (off by default): also swap `gbase.G2d.final_conv` (model.py:747-752) for model.G2dFinalConv, which shares the
    Sequential's own modules and Parameters — optimizers built before stay valid for it.
    g2d_body (off by default): also swap G2d's ResBlock2D blocks for model.ResBlock2DFused (inference only; model.native_g2d_body).
    eapp_trunk (off by default): also swap `gbase.appearanceEncoder.resblock_128 / _256 / _512` (model.py:210-212) for
    model.ResBlockCustomFused (inference only; model.native_eapp_trunk).
    half_precision (off by default): g2d_body / eapp_trunk blocks get their half-precision form — one f16 product per multiply and half
    outputs inside torch.autocast(float16) and as .half() / .bfloat16() modules (model.ResBlock2DFused).
    fuse_upsample (off by default): with g2d_body, G2d's three `Sequential(Upsample, ResBlock2D)` stages become model.Up2ResBlock2DFused,
    the bilinear x2 up-sample folded into the block's convs; with half_precision=True they keep the materialised up-sample.
    motion_encoder (off by default): also swap the BasicBlocks of `gbase.motionEncoder`'s two ResNet-18s for model.BasicBlockFused
    (inference only; model.native_emtn_resnets).
    fuse_stem (off by default): with motion_encoder, each of the two nets' 3->64 stems (conv, BatchNorm, ReLU, max-pool) becomes one launch
    (model.StemFused; model.native_emtn_stems).  Without motion_encoder it is a ValueError: the keyword belongs to that switch, as
    Emtn.native_resnets has it (fuse_upsample without g2d_body is ignored silently; a new keyword does not repeat that).
    rotation_net (off by default): with motion_encoder, the 27 deploy-form RepVGG blocks of the frozen 6DRepNet
    (`gbase.motionEncoder.rotation_net`) become model.RepVGGBlockFused, one matrix-core launch each (inference only;
    model.native_rotation_net).  Without motion_encoder it is a ValueError, like fuse_stem.
    split_small_maps (off by default): with motion_encoder, the stride-1 convs of the blocks fused there take the split-K launch where the
    library recommends one (ops.conv2d_splits).  Without motion_encoder it is a ValueError, like fuse_stem.
    eapp_stems (off by default): also swap the two 7x7 stems of `gbase.appearanceEncoder` (`conv`, and `custom_resnet50`'s
    conv1-bn1-relu-maxpool) for their one-launch matrix-core forms (inference only; model.native_eapp_stems).  Independent of eapp_trunk."""
    if split_small_maps and not motion_encoder:
        raise ValueError("install: split_small_maps=True needs motion_encoder=True")
    if fuse_stem and not motion_encoder:
        raise ValueError("install: fuse_stem=True needs motion_encoder=True")
    if rotation_net and not motion_encoder:
        raise ValueError("install: rotation_net=True needs motion_encoder=True")
    done = swap_hot_path(gbase, eapp_tail=eapp_tail)
    if g2d_final and M.native_final_conv(gbase.G2d, True):
        done.append("G2d.final_conv")
    if g2d_body and M.native_g2d_body(gbase.G2d, True, half_precision, fuse_upsample):
        done.append("G2d.body")
    if eapp_trunk and M.native_eapp_trunk(getattr(gbase, "appearanceEncoder", None), True, half_precision):
        done.append("Eapp.trunk2d")
    if eapp_stems and M.native_eapp_stems(getattr(gbase, "appearanceEncoder", None), True):
        done.append("Eapp.stems")
    emtn = getattr(gbase, "motionEncoder", None)
    if motion_encoder and M.native_emtn_resnets(emtn, True, split_small_maps):
        done.append("Emtn.resnets")
    if motion_encoder and fuse_stem and M.native_emtn_stems(emtn, True):
        done.append("Emtn.stems")
    if motion_encoder and rotation_net and M.native_rotation_net(emtn, True, split_small_maps):
        done.append("Emtn.rotation_net")
    if model_module is not None:
        done += [f"{getattr(model_module, '__name__', 'model')}.{n}" for n in patch_functions(model_module)]
    return done


def install_vgg19_loss(perceptual) -> List[str]:
    """Binds the VGG19 terms of the reference's `PerceptualLoss` (model.py:1928-2017: an object with `.vgg19` and `.vgg19_layers`) to
    losses.VGG19FeatureLoss.from_sequential(perceptual.vgg19): `compute_vgg19_loss(predicted, target)` and
    `compute_feature_matching_loss(predicted, target)` (the same sum with the target detached) become instance attributes that run the
    loss, forward and gradient, on the HIP kernels.  The Sequential's modules and Parameters are shared and their requires_grad is left
    alone: torchvision's weights come with requires_grad=True, and such weights take the module's plain-PyTorch path, so call
    `perceptual.vgg19.requires_grad_(False)` (the reference's optimizers never hold them).  Returns the names it replaced.  `install`
    itself does not call this."""
    from .losses import VGG19FeatureLoss

    loss = VGG19FeatureLoss.from_sequential(perceptual.vgg19, taps=tuple(perceptual.vgg19_layers))
    # (kept off the Module's registry: the loss shares perceptual.vgg19, a second registration would double its state-dict keys)
    perceptual.__dict__["_mphip_vgg19_loss"] = loss
    perceptual.compute_vgg19_loss = lambda predicted, target: loss(predicted, target)
    perceptual.compute_feature_matching_loss = lambda predicted, target: loss(predicted, target.detach())
    return ["compute_vgg19_loss", "compute_feature_matching_loss"]
