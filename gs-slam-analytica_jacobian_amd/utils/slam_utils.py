"""Losses that seed the backward of the render path, with the reference's names and semantics
(utils/slam_utils.py:56-128 get_loss_tracking* / get_loss_mapping*; compute_loss of
Jacobian_test.py:155-196), get_median_depth (:131-142) and the image-gradient helpers (:4-53 image_gradient,
image_gradient_mask, depth_reg).  Device-agnostic restatement; get_median_depth hands device tensors to the kernels of
gsaj.seeding.  The gradient helpers are plain torch on the input's device: the product's gradient mask is gsaj.grad_mask
(Camera.compute_grad_mask), these are the module's surface and what tools time it against."""
import torch
import torch.nn.functional as F

_SCHARR = ((3.0, 10.0, 3.0), (0.0, 0.0, 0.0), (-3.0, -10.0, -3.0))  # rows above minus rows below; transposed: left minus right


def _reflect_padded(image):
    return F.pad(image[None], (1, 1, 1, 1), mode="reflect")


def image_gradient(image):
    """Scharr gradients of a [C,H,W] image, each channel on its own, normalised by the filter's absolute sum (32), on the image
    reflect-padded by one pixel -> (vertical [C,H,W], horizontal [C,H,W]).  Reference :4-21."""
    c = image.shape[0]
    kv = torch.tensor(_SCHARR, dtype=torch.float32, device=image.device)
    norm = 1.0 / kv.abs().sum()
    p = _reflect_padded(image)
    gv = F.conv2d(p, kv.expand(c, 1, 3, 3).contiguous(), groups=c)
    gh = F.conv2d(p, kv.t().expand(c, 1, 3, 3).contiguous(), groups=c)
    return (norm * gv)[0], (norm * gh)[0]


def image_gradient_mask(image, eps=0.01):
    """Where all nine reflect-padded neighbours have |value| > eps -> the same bool [C,H,W] twice (the reference computes it once
    per filter).  Reference :24-38."""
    small = (torch.abs(_reflect_padded(image)) > eps).logical_not().float()
    valid = (F.max_pool2d(small, 3, stride=1) == 0)[0]
    return valid, valid.clone()


def depth_reg(depth, gt_image, huber_eps=0.1, mask=None):
    """Edge-aware depth smoothness (reference :41-53; the reference never calls it, huber_eps and mask are unused there too): the
    depth gradients weighted by exp(-10 gray_gradient^2), averaged over the pixels whose depth neighbourhood is valid."""
    valid_v, valid_h = image_gradient_mask(depth)
    gray_v, gray_h = image_gradient(gt_image.mean(dim=0, keepdim=True))
    depth_v, depth_h = image_gradient(depth)
    term_v = torch.exp(-10 * gray_v[valid_v] ** 2) * torch.abs(depth_v[valid_v])
    term_h = torch.exp(-10 * gray_h[valid_h] ** 2) * torch.abs(depth_h[valid_h])
    return term_h.mean() + term_v.mean()


def _as_depth_tensor(d, like):
    if not torch.is_tensor(d):
        d = torch.from_numpy(d)
    return d.to(dtype=torch.float32, device=like.device)[None]


def _rgb_mask(config, gt_image, shape):
    thr = config["Training"]["rgb_boundary_threshold"]
    return (gt_image.sum(dim=0) > thr).view(*shape)


def get_loss_tracking(config, image, depth, opacity, viewpoint, initialization=False):
    image_ab = torch.exp(viewpoint.exposure_a) * image + viewpoint.exposure_b
    if config["Training"]["monocular"]:
        return get_loss_tracking_rgb(config, image_ab, depth, opacity, viewpoint)
    return get_loss_tracking_rgbd(config, image_ab, depth, opacity, viewpoint)


def get_loss_tracking_rgb(config, image, depth, opacity, viewpoint):
    gt = viewpoint.original_image.to(image.device)
    _, h, w = gt.shape
    mask = _rgb_mask(config, gt, (1, h, w)) * viewpoint.grad_mask
    return (opacity * torch.abs(image * mask - gt * mask)).mean()


def get_loss_tracking_rgbd(config, image, depth, opacity, viewpoint, initialization=False):
    alpha = config["Training"].get("alpha", 0.95)
    gt_depth = _as_depth_tensor(viewpoint.depth, image)
    depth_mask = (gt_depth > 0.01).view(*depth.shape) * (opacity > 0.95).view(*depth.shape)
    l1_rgb = get_loss_tracking_rgb(config, image, depth, opacity, viewpoint)
    l1_depth = torch.abs(depth * depth_mask - gt_depth * depth_mask)
    return alpha * l1_rgb + (1 - alpha) * l1_depth.mean()


def get_loss_mapping(config, image, depth, viewpoint, opacity, initialization=False):
    image_ab = image if initialization else torch.exp(viewpoint.exposure_a) * image + viewpoint.exposure_b
    if config["Training"]["monocular"]:
        return get_loss_mapping_rgb(config, image_ab, depth, viewpoint)
    return get_loss_mapping_rgbd(config, image_ab, depth, viewpoint)


def get_loss_mapping_rgb(config, image, depth, viewpoint):
    gt = viewpoint.original_image.to(image.device)
    _, h, w = gt.shape
    mask = _rgb_mask(config, gt, (1, h, w))
    return torch.abs(image * mask - gt * mask).mean()


def get_loss_mapping_rgbd(config, image, depth, viewpoint, initialization=False):
    alpha = config["Training"].get("alpha", 0.95)
    gt = viewpoint.original_image.to(image.device)
    gt_depth = _as_depth_tensor(viewpoint.depth, image)
    rgb_mask = _rgb_mask(config, gt, depth.shape)
    depth_mask = (gt_depth > 0.01).view(*depth.shape)
    l1_rgb = torch.abs(image * rgb_mask - gt * rgb_mask)
    l1_depth = torch.abs(depth * depth_mask - gt_depth * depth_mask)
    return alpha * l1_rgb.mean() + (1 - alpha) * l1_depth.mean()


def compute_loss(gaussian_model, color, depth, color_gt, depth_gt, mask, compute_depth_loss=True):
    """Masked L1 colour (mean over 3HW) + L1 depth over valid pixels + 10 x isotropic regulariser."""
    m = mask.unsqueeze(0)
    loss = torch.nn.functional.l1_loss(color * m, color_gt * m)
    scales = gaussian_model.get_scaling
    loss = loss + 10.0 * torch.abs(scales - scales.mean(dim=1, keepdim=True)).mean()
    if compute_depth_loss:
        dgt = depth_gt if depth_gt.dim() == 2 else depth_gt.squeeze(0)
        valid = (dgt > 0.0) & mask
        loss = loss + torch.nn.functional.l1_loss(depth.squeeze(0)[valid], dgt[valid])
    return loss


def get_median_depth(depth, opacity=None, mask=None, return_std=False):
    """Reference :131-142: the (lower) median of the depths with depth > 0, opacity > 0.95 and mask, optionally with their unbiased
    standard deviation and the valid mask.  Device tensors go to gsaj.seeding.median_depth (one pass of kernels, no host
    synchronisation; no valid pixel gives 0 there instead of an exception); CPU tensors take the torch statement below.  Unlike
    the reference, opacity=None works."""
    if depth.device.type == "cuda":  # (always the kernels: they refuse what they do not cover, nothing falls back to torch ops)
        from gsaj.seeding import median_depth
        return median_depth(depth, None if opacity is None else opacity.detach(), mask, return_std)
    depth = depth.detach().clone()
    valid = depth > 0
    if opacity is not None:
        valid = torch.logical_and(valid, opacity.detach() > 0.95)
    if mask is not None:
        valid = torch.logical_and(valid, mask)
    valid_depth = depth[valid]
    if return_std:
        return valid_depth.median(), valid_depth.std(), valid
    return valid_depth.median()
