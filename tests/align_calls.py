"""The call helpers of tests/test_gpu_align.py and tests/test_gpu_align_joint.py: the buffers of one gsaj_rgbd_align / gsaj_rgbd_align8
call, the call, the step on its row, the aligner.  One set, parametrised by the form: Calls(joint).  The forms differ in the state and
the row (gsaj._gn_state.layout("gn" | "gn8")), in the joint form's `gain` buffer and exposure slots, and in the entry points called.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import align_restated as ar

DEV = "cuda:0"
F = np.float32


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def dev(case, name):
    import torch
    return None if case.get(name) is None else torch.from_numpy(np.ascontiguousarray(case[name], F)).to(DEV)


class Calls:
    def __init__(self, joint):
        self.joint = joint
        self.entry, self.stepper = ("gsaj_rgbd_align8", "gsaj_pose_gn8_step") if joint else ("gsaj_rgbd_align", "gsaj_pose_gn_step")

    @property
    def layout(self):
        from gsaj import _gn_state
        return _gn_state.layout("gn8" if self.joint else "gn")

    def tensors(self, case, torch):
        """Every buffer of one call, taken from torch.empty / torch.zeros (the routes tests/guards.py fences), then filled."""
        W, H = case["W"], case["H"]
        from gsaj import _lib
        lib, lay = _lib.load(), self.layout
        t = dict(ref_color=torch.empty(3, H, W, dtype=torch.float32, device=DEV), ref_depth=torch.empty(H, W, dtype=torch.float32, device=DEV),
                 ref_w2c=torch.empty(16, dtype=torch.float32, device=DEV), cur_color=torch.empty(3, H, W, dtype=torch.float32, device=DEV),
                 cur_depth=torch.empty(H, W, dtype=torch.float32, device=DEV), state=torch.zeros(lay.floats, dtype=torch.float32, device=DEV),
                 rows=torch.empty(lib.gsaj_rgbd_align_partial_rows(W, H), lay.row, dtype=torch.float32, device=DEV),
                 row=torch.empty(lay.row, dtype=torch.float32, device=DEV))
        if self.joint:
            t["gain"] = torch.empty(1, dtype=torch.float32, device=DEV)
        t.update(pix=torch.empty(H, W, 16, dtype=torch.float32, device=DEV), valid=torch.empty(H, W, dtype=torch.uint8, device=DEV))
        for k in ("ref_color", "ref_depth", "cur_color"):
            t[k].copy_(torch.from_numpy(np.ascontiguousarray(case[k], F)))
        t["ref_w2c"].copy_(torch.from_numpy(np.asarray(case["ref_w2c"], F).reshape(16)))
        t["cur_depth"].copy_(torch.from_numpy(np.zeros((H, W), F) if case.get("cur_depth") is None else np.ascontiguousarray(case["cur_depth"], F)))
        t["state"][lay.sl["w2c"]] = torch.from_numpy(np.asarray(case["w2c"], F).reshape(16)).to(DEV)
        if self.joint:
            t["state"][lay.sl["exposure"]] = torch.from_numpy(np.asarray(case.get("exposure", (0.0, 0.0)), F)).to(DEV)
        return t

    def call(self, case, t, skip=None, outputs=True):
        import torch

        from gsaj import _lib
        lib = _lib.load()
        out = [t[k].data_ptr() if outputs else None for k in (("gain", "pix", "valid") if self.joint else ("pix", "valid"))]
        _lib.check(getattr(lib, self.entry)(case["W"], case["H"], case["fx"], case["fy"], case["cx"], case["cy"], t["ref_color"].data_ptr(),
                                            t["ref_depth"].data_ptr(), t["ref_w2c"].data_ptr(), t["cur_color"].data_ptr(),
                                            None if case.get("cur_depth") is None else t["cur_depth"].data_ptr(), t["state"].data_ptr(),
                                            case["w_depth"], case["delta_photo"], case["delta_depth"], case["ratio"], case["min_depth"],
                                            case["max_depth"], case["min_overlap"], t["rows"].data_ptr(), t["row"].data_ptr(), *out,
                                            None if skip is None else skip.data_ptr(), torch.cuda.current_stream().cuda_stream), self.entry)

    def run(self, case):
        import torch
        t = self.tensors(case, torch)
        self.call(case, t)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in t.items()}, t

    def step(self, t, projection):
        import torch

        from gsaj import _lib
        lib = _lib.load()
        _lib.check(getattr(lib, self.stepper)(t["row"].data_ptr(), 1, ar.LM["lambda_init"], ar.LM["nu"], ar.LM["lambda_min"], ar.LM["lambda_max"],
                                              ar.LM["converged_threshold"], projection.data_ptr(), t["state"].data_ptr(), None,
                                              torch.cuda.current_stream().cuda_stream), self.stepper)

    def aligner(self, **kw):
        import gsaj
        cam = ar.camera()
        cls = gsaj.JointRgbdAligner if self.joint else gsaj.RgbdAligner
        return cls(cam["W"], cam["H"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], DEV, levels=2, **kw)
