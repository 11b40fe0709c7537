"""Parameter-space helpers with the reference's names
(gaussian_splatting/utils/general_utils.py: inverse_sigmoid :20-21, strip_lowerdiag /
strip_symmetric :97-110, build_rotation :113-136, build_scaling_rotation :139-148, the position learning-rate schedule
get_expon_lr_func / helper :42-94); device-agnostic (the reference hard-codes device="cuda")."""
import numpy as np
import torch


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def helper(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """The schedule of the xyz learning rate: lr_init at step 0, lr_final from max_steps on, interpolated linearly in the
    logarithm between them; with lr_delay_steps > 0 scaled by a factor that rises as a quarter sine from lr_delay_mult to 1 over
    those steps.  0 for a negative step or when both rates are 0 (the parameter is switched off)."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    delay = 1.0
    if lr_delay_steps > 0:
        delay = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
    t = np.clip(step / max_steps, 0, 1)
    return delay * np.exp((1 - t) * np.log(lr_init) + t * np.log(lr_final))


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """The reference's get_expon_lr_func returns `helper` itself, whatever it is given (its closure is commented out): the
    caller passes the schedule's numbers at every call.  Kept so."""
    return helper


def strip_lowerdiag(L):
    """(N,3,3) symmetric -> (N,6) as (xx, xy, xz, yy, yz, zz)."""
    return torch.stack([L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]], dim=1)


def strip_symmetric(sym):
    return strip_lowerdiag(sym)


def build_rotation(r):
    """Rotation matrices of (r, x, y, z) quaternions, normalised first."""
    q = r / r.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(dim=1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).view(-1, 3, 3)


def build_scaling_rotation(s, r):
    """L = R diag(s), so that Sigma = L L^T."""
    return build_rotation(r) * s.unsqueeze(1)
