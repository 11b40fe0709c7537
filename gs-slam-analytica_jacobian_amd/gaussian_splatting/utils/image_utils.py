"""mse and psnr under the reference's names (gaussian_splatting/utils/image_utils.py): for a batch [N,...], the mean squared
difference of each image as [N,1], and 20 log10(1 / sqrt(mse)).  Plain torch on the input's device: these are the module's surface
and what tools time the device path against; eval_rendering's per-frame PSNR is gsaj.evaluation.FrameEvaluator (csrc/eval.hip),
which needs neither the boolean-index gathers nor a host read."""
import torch


def mse(img1, img2):
    d = (img1 - img2).reshape(img1.shape[0], -1)
    return (d * d).mean(dim=1, keepdim=True)


def psnr(img1, img2):
    return 20 * torch.log10(1.0 / torch.sqrt(mse(img1, img2)))
