"""The image losses of the reference's gaussian_splatting/utils/loss_utils.py with its signatures, for stand-alone use (as
utils/slam_utils.py mirrors the tracking / mapping losses): `l1_loss`, `l2_loss` and `ssim`, whose forward and backward run as
HIP kernels (gsaj.ssim; fp32 device tensors only, gradient w.r.t. img1 only).  `l1_loss_weight` needs cv2 (Sobel) and is not
provided.  Inside the reference checkout the reference's own module wins the import."""
from gsaj.ssim import l1_loss, ssim  # noqa: F401


def l2_loss(network_output, gt):
    return ((network_output - gt) ** 2).mean()
