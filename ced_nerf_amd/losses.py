"""The reference's training regularisers (train_real.py:371-409, flags of opt.py:46-72):

  -d   distortion loss          `distortion` (drop-in for cednerf/losses.py:4-11), `distortion_from_density` (fused)
  -ae  accumulated-opacity entropy  `acc_entropy_loss`
  -o   opacity loss              `opacity_loss`
  -wr  weighted per-sample colour loss  `weighted_rgb_loss`

The distortion loss runs on the HIP kernels of csrc/losses.hip in both directions; the other three are a few element-wise
torch operations on tensors the renderer already returns.  None of them carries the reference's 1e-3 factor:
`train.train_step(loss_weights=...)` applies it.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import ops
from .nerfacc_api import _packed_info_from


def _require_cuda(*tensors: Tensor) -> None:
    for t in tensors:
        if not t.is_cuda:
            raise NotImplementedError(f"the distortion loss runs on the HIP kernels only (got a tensor on {t.device}); "
                                      "ced_nerf_amd has no CPU fallback")


class _DistortionFn(torch.autograd.Function):
    """ced_distortion_loss: the loss and the unscaled dL/dw come from one kernel pass; the backward only scales the
    gradient by grad_out / n_norm (n_norm read on the device: no host synchronisation in either direction)."""

    @staticmethod
    def forward(ctx, weights, t_starts, t_ends, packed):
        loss, inv_norm, _, grad = ops.distortion_loss(packed, weights.detach().contiguous(), t_starts, t_ends,
                                                      want_grad=ctx.needs_input_grad[0])
        if grad is not None:
            ctx.save_for_backward(grad, inv_norm)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        grad, inv_norm = ctx.saved_tensors
        return grad * (grad_out * inv_norm), None, None, None


class _DistortionDensityFn(torch.autograd.Function):
    """ced_distortion_loss_density: weights recomputed from the densities (the bits of ced_render_weights), loss and the
    unscaled dL/dsigma in one kernel pass; no weights tensor, no autograd node for them."""

    @staticmethod
    def forward(ctx, sigmas, t_starts, t_ends, packed):
        loss, inv_norm, _, d_sig = ops.distortion_loss_density(packed, sigmas.detach().contiguous(), t_starts, t_ends,
                                                               want_grad=ctx.needs_input_grad[0])
        if d_sig is not None:
            ctx.save_for_backward(d_sig, inv_norm)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        d_sig, inv_norm = ctx.saved_tensors
        return d_sig * (grad_out * inv_norm), None, None, None


def _flat_f32(t: Tensor) -> Tensor:
    return t.reshape(-1).float().contiguous()


def distortion(ray_ids: Tensor, weights: Tensor, t_starts: Tensor, t_ends: Tensor) -> Tensor:
    """Drop-in for cednerf/losses.py:distortion (= torch_efficient_distloss.flatten_eff_distloss(w, m, s, ray_ids)).
    Shapes [S] or [S,1]; returns a scalar with a gradient to `weights` only.  Contract:
        loss = sum_rays [ sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i s_i w_i^2 ] / (ray_ids.max() + 1),
    with m = (t_starts + t_ends) / 2 and s = t_ends - t_starts.  Precondition (met by every sampler of this package):
    samples are grouped by ray in increasing ray index, and t_starts does not decrease within a ray; they are not sorted
    here.  The per-ray offsets come from `_packed_info_from` (a bincount: one host synchronisation for the ray count)."""
    _require_cuda(ray_ids, weights, t_starts, t_ends)
    w = weights.reshape(-1)
    if w.dtype != torch.float32:
        w = w.float()
    packed = _packed_info_from(ray_ids.reshape(-1).long(), 0)
    loss = _DistortionFn.apply(w, _flat_f32(t_starts), _flat_f32(t_ends), packed)
    return loss


def distortion_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Tensor) -> Tensor:
    """The distortion loss of the weights render_weight_from_density(t_starts, t_ends, sigmas, packed_info) would give,
    with the gradient going straight to `sigmas` (the fused route of `train.train_step`).  Same contract and precondition
    as `distortion`, with n_norm = 1 + the largest ray index of packed_info that has a sample.  No host synchronisation."""
    _require_cuda(t_starts, t_ends, sigmas, packed_info)
    sig = sigmas.reshape(-1)
    if sig.dtype != torch.float32:
        sig = sig.float()
    return _DistortionDensityFn.apply(sig, _flat_f32(t_starts), _flat_f32(t_ends), packed_info.long().contiguous())


def opacity_loss(acc: Tensor) -> Tensor:
    """`-o`, train_real.py:373-374 without its 1e-3: mean(-acc log acc).  One divergence: it is computed with xlogy, so
    acc = 0 contributes 0 where the reference's acc * log(acc) gives NaN."""
    return (-torch.xlogy(acc, acc)).mean()


def acc_entropy_loss(acc: Tensor) -> Tensor:
    """`-ae`, train_real.py:388-392 without its 1e-3: the binary entropy of the remaining transmittance 1 - acc,
    clamped to [1e-6, 1 - 1e-6]."""
    T_last = (1 - acc).clamp(1e-6, 1 - 1e-6)
    return -(T_last * torch.log(T_last) + (1 - T_last) * torch.log(1 - T_last)).mean()


def weighted_rgb_loss(rgbs: Tensor, pixels: Tensor, ray_indices: Tensor, weights: Tensor) -> Tensor:
    """`-wr`, train_real.py:394-396 without its 1e-3: sum_i w_i |rgb_i - pixel_ray(i)|^2 / n_rays, the weights detached
    (only the per-sample colours get a gradient)."""
    rgbper = (rgbs - pixels[ray_indices]).pow(2).sum(dim=-1)
    return (rgbper * weights.detach().reshape(rgbper.shape)).sum() / pixels.shape[0]
