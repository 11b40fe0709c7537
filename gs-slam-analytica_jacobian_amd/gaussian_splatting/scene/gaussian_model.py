"""Parameter store + activations of the Gaussian map: the part of the reference's
GaussianModel that the render path reads (gaussian_splatting/scene/gaussian_model.py:141-177:
get_xyz, get_features, get_opacity, get_scaling, get_rotation, get_covariance,
active_sh_degree / max_sh_degree), plus what sits directly either side of it: the
densification bookkeeping fed by a backward (add_densification_stats :767-771, max_radii2D, n_obs --
one device launch, gsaj_densification_stats) and parameter I/O in the reference's formats
(load_tensors :70-138, save_ply :402-436, load_ply :453-542; gsaj.model_io), and map growth from a keyframe
(create_pcd_from_image[_and_depth] :183-279, extend_from_pcd[_seq] :284-319: on the device, gsaj.seeding, where the reference
goes through NumPy and Open3D).  The optimiser surgery of the mapping loop is here too: training_setup (:321-370, plain torch),
new rows enter an attached Adam with zero moments (cat_tensors_to_optimizer :599-631), rows leave the map and the Adam state
under a mask (prune_points, _prune_optimizer :559-597: one device launch, gsaj.pruning), and the consumer of the densification
statistics, densify_and_prune / densify_and_clone / densify_and_split (:669-765), is one plan, one 16-byte read, one launch that
moves every tensor and one that computes the children (gsaj.densify).  The step itself is one launch as well (map_step: the chain
rule through the activations, Adam, and reset_opacity / reset_opacity_nonvisible :438-451 fused or on their own; gsaj.map_step), and
update_learning_rate (:372-386) is host arithmetic.
"""
import torch

from gaussian_splatting.utils.general_utils import build_scaling_rotation, helper, inverse_sigmoid, strip_symmetric


class GaussianModel:
    def __init__(self, sh_degree: int, config=None):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        e = torch.empty(0)
        self._xyz = self._features_dc = self._features_rest = e
        self._scaling = self._rotation = self._opacity = e
        self.scaling_activation, self.scaling_inverse_activation = torch.exp, torch.log
        self.opacity_activation, self.inverse_opacity_activation = torch.sigmoid, inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize
        self.covariance_activation = self.build_covariance_from_scaling_rotation
        self.config = config
        self.isotropic = False
        self.optimizer = None
        self.seed = 0  # seed of the next keyframe's down-sample (create_pcd_from_image_and_depth) or split; advanced by every call
        self.percent_dense = 0.01  # (training_setup takes it from the training arguments)
        self.spatial_lr_scale = 0

    @classmethod
    def from_activated(cls, xyz, scales, rotations, opacities, shs, sh_degree=3, active_sh_degree=None,
                       device="cuda", requires_grad=True):
        """Build a model from *activated* parameters (what the getters will return)."""
        m = cls(sh_degree)
        t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=device)  # noqa: E731
        m._xyz = t(xyz).clone().requires_grad_(requires_grad)
        shs = t(shs)
        m._features_dc = shs[:, :1, :].clone().contiguous().requires_grad_(requires_grad)
        m._features_rest = shs[:, 1:, :].clone().contiguous().requires_grad_(requires_grad)
        m._scaling = torch.log(t(scales)).requires_grad_(requires_grad)
        m._rotation = t(rotations).clone().requires_grad_(requires_grad)
        m._opacity = inverse_sigmoid(t(opacities)).requires_grad_(requires_grad)
        m.active_sh_degree = sh_degree if active_sh_degree is None else active_sh_degree
        return m

    def build_covariance_from_scaling_rotation(self, scaling, scaling_modifier, rotation):
        L = build_scaling_rotation(scaling_modifier * scaling, rotation)
        return strip_symmetric(L @ L.transpose(1, 2))

    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    def get_covariance(self, scaling_modifier=1):
        return self.covariance_activation(self.get_scaling, scaling_modifier, self.rotation_activation(self._rotation))

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def parameters(self):
        return [self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation]

    def assign_bucket_gradients(self, g, accumulate=False):
        """.grad of the six raw parameters from the gradients a batched backward leaves in its bucket (gsaj.rasterizer.BatchContext /
        FrameContext: g["mean3D"], g["sh"], g["opacity"], g["scale"], g["rot"] w.r.t. the ACTIVATED quantities the rasteriser is fed):
        what loss.backward() would have left there through the activations of the reference model (exp, normalize, sigmoid, cat;
        gaussian_model.py:41-56, 141-165), in closed form.  accumulate=True adds to existing .grad (several windows per step)."""
        with torch.no_grad():
            P = self._xyz.shape[0]
            sh = g["sh"].view(P, -1, 3)
            op = self.get_opacity
            sc = self.get_scaling
            g_sc = g["scale"] * (sc if sc.shape[1] == 3 else sc.expand(-1, 3))
            if self._scaling.shape[1] == 1:  # isotropic model: one log-scale drives the three axes (gaussian_renderer/__init__.py:98-101)
                g_sc = g_sc.sum(dim=1, keepdim=True)
            q = self._rotation
            n = q.norm(dim=1, keepdim=True).clamp_min(1e-12)
            qh = q / n
            g_q = (g["rot"] - qh * (g["rot"] * qh).sum(dim=1, keepdim=True)) / n
            grads = ((self._xyz, g["mean3D"]), (self._features_dc, sh[:, :1, :]), (self._features_rest, sh[:, 1:, :]),
                     (self._opacity, g["opacity"].view(P, 1) * op * (1.0 - op)), (self._scaling, g_sc), (self._rotation, g_q))
            for prm, gr in grads:
                gr = gr.reshape(prm.shape).to(prm.dtype)
                if accumulate and prm.grad is not None:
                    prm.grad += gr
                else:
                    prm.grad = gr.clone()

    # ---- bookkeeping tensors + parameter I/O -----------------------------------------------------------
    def _init_aux(self):
        """The auxiliary tensors load_tensors / load_ply create (gaussian_model.py:124-131, 538-542)."""
        n, dev = self._xyz.shape[0], self._xyz.device
        self.max_radii2D = torch.zeros((n,), device=dev)
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.unique_kfIDs = torch.zeros((n,)).int()
        self.n_obs = torch.zeros((n,)).int()

    def _set_params(self, xyz, f_dc, f_rest, opacity, scaling, rotation, device):
        t = lambda a: torch.as_tensor(a, dtype=torch.float32).to(device).contiguous().requires_grad_(True)  # noqa: E731
        self._xyz, self._features_dc, self._features_rest = t(xyz), t(f_dc), t(f_rest)
        self._opacity, self._scaling, self._rotation = t(opacity), t(scaling), t(rotation)
        self._init_aux()

    def load_tensors(self, model_path, device="cuda"):
        """Reference load_tensors (:70-138): parameters in stored order xyz, f_dc, f_rest, opacity, scaling, rotation; a 2-D f_dc
        becomes [P,1,3]; active_sh_degree is left as it is (the reference never raises it here).  Nothing in the file is
        executed (gsaj.model_io.read_parameter_tensors).  Returns True / False like the reference."""
        from gsaj.model_io import read_parameter_tensors
        try:
            ts = read_parameter_tensors(model_path)
            # the reference takes named_parameters() of the scripted module (parameters only, in registration order); the
            # restricted reader returns every tensor of the pickled state in stored order and does NOT tell parameters from
            # buffers, so the six must be exactly six and must look like xyz, f_dc, f_rest, opacity, scaling, rotation -- an
            # archive with anything else in between would otherwise be mapped to the wrong fields without a word
            if len(ts) != 6:
                raise ValueError("expected exactly 6 parameter tensors (xyz, f_dc, f_rest, opacity, scaling, rotation), found %d" % len(ts))
            xyz, f_dc, f_rest, opacity, scaling, rotation = ts
            if f_dc.dim() == 2:
                f_dc = f_dc.unsqueeze(1)
            P = xyz.shape[0] if xyz.dim() == 2 else -1
            ok = (all(t.is_floating_point() for t in ts) and xyz.dim() == 2 and xyz.shape[1] == 3
                  and f_dc.dim() == 3 and tuple(f_dc.shape[::2]) == (P, 3) and f_dc.shape[1] == 1
                  and f_rest.dim() == 3 and tuple(f_rest.shape[::2]) == (P, 3)
                  and tuple(opacity.shape) == (P, 1)
                  and scaling.dim() == 2 and scaling.shape[0] == P and scaling.shape[1] in (1, 3)
                  and tuple(rotation.shape) == (P, 4))
            if not ok:
                raise ValueError("the 6 tensors do not have the shapes of (xyz [P,3], f_dc [P,1,3], f_rest [P,M-1,3], opacity [P,1], "
                                 "scaling [P,1|3], rotation [P,4]): %s" % ([tuple(t.shape) for t in ts],))
            self._set_params(xyz, f_dc, f_rest, opacity, scaling, rotation, device)
            return True
        except Exception as e:  # noqa: BLE001 -- the reference reports and returns False
            print("Error loading tensors from %s: %s" % (model_path, e))
            return False

    def construct_list_of_attributes(self):
        from gsaj.model_io import ply_attributes
        return ply_attributes(self._features_dc.shape[1] * self._features_dc.shape[2], self._features_rest.shape[1] * self._features_rest.shape[2],
                              self._scaling.shape[1], self._rotation.shape[1])

    def save_ply(self, path):
        import os
        from gsaj.model_io import write_ply
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        d = lambda x: x.detach().cpu().numpy()  # noqa: E731
        write_ply(path, d(self._xyz), d(self._features_dc), d(self._features_rest), d(self._opacity), d(self._scaling), d(self._rotation))

    def load_ply(self, path, device="cuda"):
        from gsaj.model_io import read_gaussian_ply
        g = read_gaussian_ply(path, self.max_sh_degree)
        self._set_params(g["xyz"], g["f_dc"], g["f_rest"], g["opacity"], g["scaling"], g["rotation"], device)
        self.ply_input = dict(points=g["xyz"], normals=g["normals"])
        self.active_sh_degree = self.max_sh_degree

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        """Reference :767-771, one device launch: xyz_gradient_accum[f] += ||grad[f, :2]||, denom[f] += 1.  update_filter is the
        view's visibility filter (radii > 0), as every caller passes it (slam_backend.py:119, 282)."""
        self.densification_step(viewspace_point_tensor.grad[None], update_filter[None].to(torch.int32), None, update_max_radii=False)

    def densification_step(self, dL_dmean2D, radii, n_touched=None, update_max_radii=True):
        """All bookkeeping of one mapping iteration over K views in ONE launch: dL_dmean2D [K,P,3] (BatchContext's g["mean2D"] or
        stacked viewspace_points.grad), radii [K,P] int32, n_touched [K,P] int32 or None.  Updates xyz_gradient_accum, denom,
        max_radii2D (visible = radii > 0) and, with n_touched, n_obs = number of views that touched each Gaussian
        (slam_backend.py:113-121, 236-250, 276-285)."""
        from gsaj import _lib
        lib = _lib.load()
        K, P = radii.shape
        g = dL_dmean2D.to(torch.float32).contiguous()
        r = radii.to(torch.int32).contiguous()
        nt = None if n_touched is None else n_touched.to(torch.int32).contiguous()
        dev = g.device
        n_obs = torch.zeros((P,), dtype=torch.int32, device=dev) if nt is not None else None
        if self.max_radii2D.device != dev:
            self.max_radii2D = self.max_radii2D.to(dev)
        with torch.cuda.device(dev):
            _lib.check(lib.gsaj_densification_stats(K, P, g.data_ptr(), r.data_ptr(), None if nt is None else nt.data_ptr(),
                                                    self.xyz_gradient_accum.data_ptr(), self.denom.data_ptr(),
                                                    self.max_radii2D.data_ptr() if update_max_radii else None,
                                                    None if n_obs is None else n_obs.data_ptr(),
                                                    torch.cuda.current_stream(dev).cuda_stream), "gsaj_densification_stats")
        if n_obs is not None:
            self.n_obs = n_obs
        return n_obs

    # ---- map growth from a keyframe (reference :183-319) ----------------------------------------------------------------
    def init_lr(self, spatial_lr_scale):
        self.spatial_lr_scale = spatial_lr_scale

    def create_pcd_from_image(self, cam_info, init=False, scale=2.0, depthmap=None):
        """Reference :183-207.  depthmap: [H,W] array or tensor (what add_new_keyframe returned); None: cam_info.depth, or, for
        a monocular sensor, (1 + 0.05 (randn - 0.5)) * scale.  The colour is cam_info.original_image under the camera's
        exposure, applied inside the kernel."""
        cam = cam_info
        dev = cam.original_image.device
        if depthmap is None:
            if self.config["Dataset"]["sensor_type"] == "monocular":
                shape = (cam.image_height, cam.image_width)
                depthmap = (torch.ones(shape) + (torch.randn(shape) - 0.5) * 0.05) * scale
            else:
                depthmap = cam.depth
        depth = torch.as_tensor(depthmap, dtype=torch.float32).to(dev)
        return self.create_pcd_from_image_and_depth(cam, cam.original_image, depth, init)

    def create_pcd_from_image_and_depth(self, cam, rgb, depth, init=False):
        """Reference :209-279 with tensors where it takes o3d.geometry.Image: rgb [3,H,W] fp32 in [0,1] BEFORE the exposure (the
        kernel applies exp(a) rgb + b, clamps and quantises to 8 bits as :185-187 does), depth [H,W] fp32, both on the device.
        Returns (xyz, features [m,3,M], scales, rots, opacities) like the reference.  The down-sample is a uniform subset
        reproducible from self.seed (the reference's Open3D shuffle is unseeded); self.seed advances by one per call."""
        from gsaj.seeding import seed_from_keyframe
        from gaussian_splatting.utils.graphics_utils import getWorld2View2
        ds = self.config["Dataset"]
        factor = ds["pcd_downsample_init"] if init else ds["pcd_downsample"]
        dev = depth.device
        w2c = getWorld2View2(cam.R, cam.T).to(device=dev, dtype=torch.float32).contiguous()
        ab = torch.cat([cam.exposure_a.detach().reshape(1), cam.exposure_b.detach().reshape(1)]).to(device=dev, dtype=torch.float32)
        seed, self.seed = self.seed, self.seed + 1
        return seed_from_keyframe(rgb, depth, w2c, cam.fx, cam.fy, cam.cx, cam.cy, factor, ds["point_size"],
                                 sh_degree=self.max_sh_degree, adaptive_pointsize=bool(ds.get("adaptive_pointsize", False)),
                                 isotropic=self.isotropic, exposure_ab=ab, seed=seed)

    def extend_from_pcd(self, fused_point_cloud, features, scales, rots, opacities, kf_id):
        """Reference :284-309 + densification_postfix :633-667: append the new Gaussians as new leaf tensors, reset max_radii2D /
        xyz_gradient_accum / denom to zeros of the new size, extend unique_kfIDs with kf_id and n_obs with zeros.  With an
        optimizer attached (torch.optim.Adam, one parameter per group, named xyz, f_dc, f_rest, opacity, scaling, rotation) the
        new parameters replace the old ones in their groups and exp_avg / exp_avg_sq are padded with zeros (:599-631)."""
        new = {"xyz": fused_point_cloud, "f_dc": features[:, :, 0:1].transpose(1, 2).contiguous(),
               "f_rest": features[:, :, 1:].transpose(1, 2).contiguous(), "opacity": opacities, "scaling": scales, "rotation": rots}
        old = {"xyz": self._xyz, "f_dc": self._features_dc, "f_rest": self._features_rest, "opacity": self._opacity,
               "scaling": self._scaling, "rotation": self._rotation}
        m = fused_point_cloud.shape[0]
        grown = {}
        with torch.no_grad():
            for name, ext in new.items():
                cur = old[name]
                ext = ext.detach().to(dtype=torch.float32)
                if cur.numel() == 0 and cur.dim() == 1:  # an empty model: the new rows are the map
                    grown[name] = ext.clone().requires_grad_(True)
                else:
                    grown[name] = torch.cat((cur.detach(), ext.to(cur.device)), dim=0).requires_grad_(True)
        moments = {}
        if self.optimizer is not None:
            for group in self.optimizer.param_groups:
                name = group["name"]
                state = self.optimizer.state.get(group["params"][0], None)
                if state is not None and "exp_avg" in state:
                    pad = torch.zeros((m,) + tuple(grown[name].shape[1:]), dtype=state["exp_avg"].dtype, device=state["exp_avg"].device)
                    moments[name] = (torch.cat((state["exp_avg"], pad), dim=0), torch.cat((state["exp_avg_sq"], pad), dim=0))
        self._install(grown, moments)
        n, dev = self._xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)

        def host_ints(name):  # (a model built without them, e.g. from_activated, gets zeros for its old rows)
            t = getattr(self, name, None)
            return t.cpu().int() if t is not None and t.shape[0] == n - m else torch.zeros((n - m,)).int()

        self.unique_kfIDs = torch.cat((host_ints("unique_kfIDs"), torch.ones((m,)).int() * kf_id)).int()
        self.n_obs = torch.cat((host_ints("n_obs"), torch.zeros((m,)).int())).int()

    def extend_from_pcd_seq(self, cam_info, kf_id=-1, init=False, scale=2.0, depthmap=None):
        fused_point_cloud, features, scales, rots, opacities = self.create_pcd_from_image(cam_info, init, scale=scale, depthmap=depthmap)
        self.extend_from_pcd(fused_point_cloud, features, scales, rots, opacities, kf_id)

    # ---- map pruning (reference :559-597) ---------------------------------------------------------------------------------
    def prune_points(self, mask, n_kept=None):
        """Reference prune_points + _prune_optimizer (:559-597): remove the rows where mask (bool or uint8 [P] on the device) is
        set.  One plan and one launch (gsaj.pruning.CompactPlan) move the six parameters, exp_avg / exp_avg_sq of every group of
        an attached optimizer that has state, xyz_gradient_accum, denom and max_radii2D, and unique_kfIDs / n_obs where those
        live on the device; host-resident ones are indexed on the host with the mask copied once (the reference's .cpu(),
        :596-597).  The new parameters are leaf tensors that replace the old ones in their optimizer groups; a group's state
        moves to the new key with every other entry (step) untouched, as in extend_from_pcd.  n_kept: the number of rows that
        stay, when the caller has it (P minus the n_pruned of CovisibilityWindow.prune_mask, read with its other scalars):
        then nothing is read here.  Returns the plan, for CovisibilityWindow.compact_plan.  A rasteriser context is sized for a
        fixed P: build a new one afterwards."""
        from gsaj.pruning import CompactPlan
        plan = CompactPlan(mask, remove=True, n_kept=n_kept)
        moved, ids = self._gather("prune_points", plan.dev)
        stats = [a for a in ("xyz_gradient_accum", "denom", "max_radii2D") if getattr(self, a, None) is not None]
        moved += [(("aux", a), getattr(self, a).contiguous(), "parent") for a in stats if getattr(self, a).device == plan.dev]
        out = dict(zip([k for k, _, _ in moved], plan.apply(*[t for _, t, _ in moved])))
        self._install_moved(out)
        keep_host = None
        for a in stats + ids:
            if ("aux", a) in out:
                setattr(self, a, out[("aux", a)])
            else:
                if keep_host is None:
                    keep_host = plan.keep_mask().cpu()
                setattr(self, a, getattr(self, a)[keep_host.to(getattr(self, a).device)])
        return plan

    # ---- what prune_points, _densify and extend_from_pcd share: the tensors of the map, and putting new ones in their place -----
    _NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")

    def _gather(self, who, dev, id_dtype=None):
        """The tensors whose rows follow the map's, as a list of (key, tensor, new-row mode): the six parameters ("param", name;
        a new row gets its parent's), exp_avg / exp_avg_sq of every optimizer group that has state ((moment, name); zeros), and
        unique_kfIDs / n_obs where they live on dev (("aux", attribute); the parent's; cast to id_dtype if given).  Beside it the
        names of the id vectors the model has, on dev or not.  who: the caller, for the message about a foreign optimizer."""
        old = dict(zip(self._NAMES, self.parameters()))
        moved = [(("param", n), old[n].detach().contiguous(), "parent") for n in self._NAMES]
        if self.optimizer is not None:
            for group in self.optimizer.param_groups:
                assert len(group["params"]) == 1
                name = group["name"]
                if group["params"][0] is not old[name]:
                    from gsaj._lib import GsajError
                    raise GsajError("%s: optimizer group %r does not hold the model's parameter of that name" % (who, name))
                state = self.optimizer.state.get(old[name], None)
                if state is not None and "exp_avg" in state:
                    moved += [((key, name), state[key].contiguous(), "zeros") for key in ("exp_avg", "exp_avg_sq")]
        ids = [a for a in ("unique_kfIDs", "n_obs") if getattr(self, a, None) is not None]
        for a in ids:
            t = getattr(self, a)
            if t.device == dev:
                moved.append((("aux", a), (t if id_dtype is None else t.to(id_dtype)).contiguous(), "parent"))
        return moved, ids

    def _install(self, new, moments):
        """new: the six parameters by name; they become the model's leaves and replace the old ones in the groups of an attached
        optimizer (one parameter per group, named as the parameters).  A group's state moves to the new key with step and every
        other entry untouched; moments: (exp_avg, exp_avg_sq) by name, for the groups whose state gets new ones."""
        new = {n: t.requires_grad_(True) for n, t in new.items()}
        if self.optimizer is not None:
            for group in self.optimizer.param_groups:
                assert len(group["params"]) == 1
                name = group["name"]
                state = self.optimizer.state.pop(group["params"][0], None)
                if name in moments:
                    state["exp_avg"], state["exp_avg_sq"] = moments[name]
                group["params"][0] = new[name]
                if state is not None:
                    self.optimizer.state[new[name]] = state
        self._xyz, self._features_dc, self._features_rest = new["xyz"], new["f_dc"], new["f_rest"]
        self._opacity, self._scaling, self._rotation = new["opacity"], new["scaling"], new["rotation"]

    def _install_moved(self, out):
        """_install from the outputs of a plan, keyed as _gather keys its list."""
        self._install({n: out[("param", n)] for n in self._NAMES},
                      {n: (out[("exp_avg", n)], out[("exp_avg_sq", n)]) for n in self._NAMES if ("exp_avg", n) in out})

    # ---- optimiser + densification (reference :321-370, :599-765) ---------------------------------------------------------
    def training_setup(self, training_args):
        """Reference :321-370 on the parameters' own device: percent_dense, zeroed xyz_gradient_accum / denom, and an Adam
        (lr=0.0, eps=1e-15) of six one-parameter groups named xyz, f_dc, f_rest, opacity, scaling, rotation with the reference's
        learning rates.  The schedule's numbers are kept (lr_init, lr_final, lr_delay_mult, max_steps); update_learning_rate
        applies it, and map_step (or optimizer.step() after assign_bucket_gradients) takes the step."""
        a = training_args
        self.percent_dense = a.percent_dense
        n, dev = self._xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        groups = [{"params": [self._xyz], "lr": a.position_lr_init * self.spatial_lr_scale, "name": "xyz"},
                  {"params": [self._features_dc], "lr": a.feature_lr, "name": "f_dc"},
                  {"params": [self._features_rest], "lr": a.feature_lr / 20.0, "name": "f_rest"},
                  {"params": [self._opacity], "lr": a.opacity_lr, "name": "opacity"},
                  {"params": [self._scaling], "lr": a.scaling_lr * self.spatial_lr_scale, "name": "scaling"},
                  {"params": [self._rotation], "lr": a.rotation_lr, "name": "rotation"}]
        self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        self.lr_init = a.position_lr_init * self.spatial_lr_scale
        self.lr_final = a.position_lr_final * self.spatial_lr_scale
        self.lr_delay_mult = a.position_lr_delay_mult
        self.max_steps = a.position_lr_max_steps

    def update_learning_rate(self, iteration):
        """Reference :372-386: the xyz group's learning rate of this iteration, set in the optimizer and returned."""
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = helper(iteration, lr_init=self.lr_init, lr_final=self.lr_final, lr_delay_mult=self.lr_delay_mult,
                                     max_steps=self.max_steps)
                return group["lr"]

    def map_step(self, g, reset=None, radii=None, freeze=()):
        """optimizer.step() of the reference's mapping loop (slam_backend.py:299-311) from the gradients a backward left in its
        context's slot g (ctx.g: mean3D, sh, opacity, scale, rot w.r.t. the ACTIVATED quantities, after any
        gsaj_isotropic_loss(accumulate=1) into g["scale"]), in ONE launch: the chain rule of assign_bucket_gradients, then Adam on
        the six raw parameters and on exp_avg / exp_avg_sq of the attached torch.optim.Adam, in place.  The optimizer keeps owning
        the state: absent state is created as torch creates it, each group's host `step` advances by one, learning rates and betas
        are read from param_groups at every call, and map_step and optimizer.step() may alternate.  .grad is not touched (it stays
        None) and g is only read.  freeze: names of groups that are not stepped, as if their .grad were None (no state created, no
        step counted), e.g. freeze=("xyz", "scaling", "rotation") for a colour refinement.
        reset: None, or the opacity reset the reference runs BEFORE the step in that iteration, fused: "all" (reset_opacity),
        "nonvisible" (reset_opacity_nonvisible; radii = int32 [K,P] or a list of bool [P] filters), "nonvisible_keep" (the same
        without the reference's quirk: visible rows keep their raw opacity instead of getting sigmoid(opacity)).  As in the
        reference the opacity group is then not stepped, its step count stays, its moments become zeros, and _opacity is a new leaf.
        An optimizer the kernel cannot reproduce raises GsajError with the reason."""
        from gsaj.map_step import map_step
        map_step(self, g, reset=reset, radii=radii, freeze=freeze)

    def reset_opacity(self):
        """Reference :438-441: every raw opacity becomes inverse_sigmoid(0.01), the opacity group's moments zeros (one launch)."""
        from gsaj.map_step import map_step
        map_step(self, None, reset="all")

    def reset_opacity_nonvisible(self, visibility_filters):
        """Reference :443-451: inverse_sigmoid(0.4) for the Gaussians no view sees, the opacity group's moments zeros (one
        launch).  visibility_filters: a list of bool [P] tensors (radii > 0 per view) or one int32 [K,P] radii tensor.  A visible
        Gaussian's raw opacity becomes sigmoid(raw), as in the reference (include/gsaj.h: kept quirk)."""
        from gsaj.map_step import map_step
        map_step(self, None, reset="nonvisible", radii=visibility_filters)

    def _densify(self, plan, seed, noise, who):
        """Send the model through a gsaj.densify.DensifyPlan: the six parameters (a new row gets its parent's), exp_avg /
        exp_avg_sq of every optimizer group that has state (a new row gets zeros; step and every other entry untouched),
        unique_kfIDs / n_obs (the parent's, int32; host-resident ones are indexed with plan.source_rows() after one copy), all in
        one rows launch; then the children's xyz and _scaling; xyz_gradient_accum, denom, max_radii2D become zeros of the new size."""
        dev = plan.dev
        moved, ids = self._gather(who, dev, id_dtype=torch.int32)
        src = {k[1]: t for k, t, _ in moved if k[0] == "param"}
        on_host = [a for a in ids if getattr(self, a).device != dev]
        if on_host:
            moved.append((("rows", None), torch.arange(plan.P, dtype=torch.int32, device=dev), "parent"))
        out = dict(zip([k for k, _, _ in moved], plan.apply([t for _, t, _ in moved], new_rows=[m for _, _, m in moved])))
        plan.children(src["xyz"], src["scaling"], src["rotation"], out[("param", "xyz")], out[("param", "scaling")], noise=noise, seed=seed)
        self._install_moved(out)
        n = plan.n_out
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)
        rows_host = None
        for a in ids:
            if a in on_host:
                if rows_host is None:
                    rows_host = out[("rows", None)].cpu().long()
                setattr(self, a, getattr(self, a)[rows_host.to(getattr(self, a).device)].int())
            else:
                setattr(self, a, out[("aux", a)])
        return plan

    def _densify_seed(self, seed, noise):
        if noise is None and seed is None:
            seed, self.seed = self.seed, self.seed + 1
        return 0 if seed is None else seed

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, seed=None, noise=None, counts=None):
        """Reference densify_and_prune (:750-765) with its densify_and_clone, densify_and_split (N = 2) and final prune_points, from
        the statistics xyz_gradient_accum / denom: one plan, one 16-byte read (none with counts = the plan's four), one rows
        launch, one children launch, three torch.zeros.  Output order and every copied bit are the reference's (include/gsaj.h
        has the rules and the kept quirks).  The children's positions are drawn from noise [2,P,3] (standard normal, indexed by
        source row) or, noise=None, from the counter-based generator under seed; seed=None takes and advances self.seed.
        Returns the plan, for CovisibilityWindow.densify_plan.  A rasteriser context is sized for a fixed P: build a new one."""
        from gsaj.densify import DensifyPlan
        plan = DensifyPlan(self.xyz_gradient_accum, self.denom, self._scaling, self._opacity, max_grad, min_opacity, extent,
                           max_screen_size, percent_dense=self.percent_dense, N=2, counts=counts)
        return self._densify(plan, self._densify_seed(seed, noise), noise, "densify_and_prune")

    def densify_and_clone(self, grads, grad_threshold, scene_extent, counts=None):
        """Reference densify_and_clone (:719-748): grads [P,1] or [P]; rows with |grads| >= grad_threshold and largest scale
        <= percent_dense * scene_extent are appended behind the map.  Nothing is pruned."""
        from gsaj.densify import CLONE, DensifyPlan
        if grads.numel() != self._xyz.shape[0]:
            from gsaj._lib import GsajError
            raise GsajError("densify_and_clone: grads must have one value per Gaussian (%d), got %s" % (self._xyz.shape[0], list(grads.shape)))
        plan = DensifyPlan(grads, None, self._scaling, self._opacity, grad_threshold, 0.0, scene_extent, None,
                           percent_dense=self.percent_dense, N=1, stages=CLONE, counts=counts)
        return self._densify(plan, 0, None, "densify_and_clone")

    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2, seed=None, noise=None, counts=None):
        """Reference densify_and_split (:669-717): grads of at most P values (the rows behind them have gradient 0); rows with
        grads >= grad_threshold and largest scale > percent_dense * scene_extent leave the map and N children each are appended,
        copy by copy.  noise [N,P,3] / seed as in densify_and_prune."""
        from gsaj.densify import SPLIT, DensifyPlan
        plan = DensifyPlan(grads, None, self._scaling, self._opacity, grad_threshold, 0.0, scene_extent, None,
                           percent_dense=self.percent_dense, N=N, stages=SPLIT, counts=counts)
        return self._densify(plan, self._densify_seed(seed, noise), noise, "densify_and_split")
