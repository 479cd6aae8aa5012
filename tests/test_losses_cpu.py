"""The reference's training regularisers (ced_nerf_amd.losses) and train_step's loss switches, without a GPU: the
element-wise terms against the literal expressions of train_real.py:369-396, the distortion loss's refusal of CPU
tensors (no fallback), and train_step's new keyword arguments with today's defaults."""
import inspect

import pytest
import torch
import torch.nn.functional as F


def _acc(n=257, seed=0):
    g = torch.Generator().manual_seed(seed)
    acc = torch.rand(n, 1, generator=g)
    acc[:4, 0] = torch.tensor([1.0, 1e-8, 0.5, 1.0 - 1e-8])
    return acc


def test_opacity_loss_is_the_reference_expression_and_zero_at_zero():
    from ced_nerf_amd import losses
    acc = _acc()
    want = (-acc * torch.log(acc)).mean()                       # train_real.py:373-374 (without its 1e-3)
    assert torch.equal(losses.opacity_loss(acc), want)
    assert losses.opacity_loss(torch.zeros(3, 1)).item() == 0.0  # xlogy: 0 log 0 = 0 (the reference gives NaN)
    a = torch.tensor([[0.0], [0.25]])
    assert losses.opacity_loss(a).item() == pytest.approx((-0.25 * torch.log(torch.tensor(0.25))).item() / 2, rel=1e-6)


def test_acc_entropy_loss_is_the_reference_expression():
    from ced_nerf_amd import losses
    acc = _acc(seed=1)
    acc[4:8, 0] = torch.tensor([0.0, 1.0, 0.0, 1.0])            # the clamp at both ends
    T_last = 1 - acc                                            # train_real.py:388-392
    T_last = T_last.clamp(1e-6, 1 - 1e-6)
    want = -(T_last * torch.log(T_last) + (1 - T_last) * torch.log(1 - T_last)).mean()
    got = losses.acc_entropy_loss(acc)
    assert torch.equal(got, want) and torch.isfinite(got)


def test_weighted_rgb_loss_is_the_reference_expression_with_detached_weights():
    from ced_nerf_amd import losses
    g = torch.Generator().manual_seed(2)
    n_rays, S = 13, 101
    pixels = torch.rand(n_rays, 3, generator=g)
    ray_indices = torch.sort(torch.randint(0, n_rays, (S,), generator=g)).values
    rgbs = torch.rand(S, 3, generator=g).requires_grad_()
    weights = torch.rand(S, generator=g).requires_grad_()
    rgbper = (rgbs - pixels[ray_indices]).pow(2).sum(dim=-1)    # train_real.py:394-396
    want = (rgbper * weights.detach()).sum() / pixels.shape[0]
    got = losses.weighted_rgb_loss(rgbs, pixels, ray_indices, weights)
    assert torch.equal(got, want)
    got.backward()
    assert rgbs.grad is not None and weights.grad is None         # only the colours get a gradient


def test_distortion_refuses_cpu_tensors():
    from ced_nerf_amd import losses
    ray_ids = torch.tensor([0, 0, 1])
    w = torch.tensor([0.2, 0.3, 0.5])
    t0 = torch.tensor([0.1, 0.2, 0.1]); t1 = t0 + 0.1
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        losses.distortion(ray_ids, w, t0, t1)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        losses.distortion_from_density(t0, t1, w, torch.tensor([[0, 2], [2, 1]]))


def test_colour_loss_mse_is_torch_mse_and_the_default_is_smooth_l1():
    from ced_nerf_amd.train import colour_loss
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(64, 3, generator=g), torch.rand(64, 3, generator=g) * 3
    assert torch.equal(colour_loss(a, b, "mse"), F.mse_loss(a, b))
    assert torch.equal(colour_loss(a, b), F.smooth_l1_loss(a, b))
    with pytest.raises(ValueError, match="rgb_loss"):
        colour_loss(a, b, "l1")


def test_train_step_loss_switches_default_to_todays_behaviour():
    from ced_nerf_amd.train import train_step
    p = inspect.signature(train_step).parameters
    want = dict(rgb_loss="smooth_l1", distortion_loss=False, acc_entropy_loss=False, opacity_loss=False,
                weight_rgbper=False, loss_weights=None)
    for name, default in want.items():
        assert p[name].default == default, (name, p[name].default)
    with pytest.raises(ValueError, match="rgb_loss"):          # refused before anything touches a device
        train_step(None, None, None, torch.zeros(1, 3), torch.zeros(1, 3), torch.zeros(1), torch.zeros(1, 3), 5e-3,
                   rgb_loss="l2")
    with pytest.raises(ValueError, match="loss_weights"):
        train_step(None, None, None, torch.zeros(1, 3), torch.zeros(1, 3), torch.zeros(1), torch.zeros(1, 3), 5e-3,
                   loss_weights={"distorsion": 1e-2})


def test_rendering_train_want_weights_defaults_off():
    from ced_nerf_amd.render import rendering_train
    p = inspect.signature(rendering_train).parameters
    assert p["want_weights"].default is False and p["packed_info"].default is None
