"""The keyframe window's covisibility, on the device (C ABI gsaj_covis_pack / gsaj_covis_query / gsaj_covis_prune_mask,
csrc/covis.hip).

The reference keeps occ_aware_visibility = {kf_id: (n_touched > 0).long()} (utils/slam_backend.py:236-240), one int64 [P]
vector per keyframe, and consults it with logical_and / logical_or / count_nonzero and a host comparison per keyframe
(utils/slam_frontend.py:198-286, 412-434) and with a sum over the window (n_obs, utils/slam_backend.py:248-263).  Here the
window is ONE uint32 word per Gaussian (bit s = "touched in the view held in slot s"), every count of one decision comes out
of one pass over the words, and the host reads them with one copy of 65 integers.  gsaj.keyframes takes the decisions from
those integers.  Inputs are int32 device tensors (FrameContext.n_touched [P], BatchContext.n_touched [K,P]); there is no CPU
path.
"""
import ctypes

import torch

from . import _lib

MAX_SLOTS = 32
PRUNE_MODES = {"odometry": 2, "slam": 3}  # mode -> the largest n_obs that is still pruned (n_obs < 3; n_obs <= prune_coviz = 3)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class CovisibilityWindow:
    """Pre-allocated for P Gaussians.  Keyframes are named by the caller's ids (the reference's frame indices); this object
    keeps the id -> slot book.  The tensors query() and prune_mask() return are buffers this object owns and are overwritten
    by the next call."""

    def __init__(self, P, device):
        self.lib = _lib.load()
        self.P, self.dev = int(P), torch.device(device)
        if self.dev.type != "cuda":
            raise _lib.GsajError("CovisibilityWindow needs a HIP device (there is no CPU path)")
        if self.P <= 0:
            raise _lib.GsajError("CovisibilityWindow needs P > 0 (got %d)" % self.P)
        self.words = torch.zeros(self.P, dtype=torch.int32, device=self.dev)  # (the 32 bits of a uint32; torch indexes int32)
        self.out = torch.zeros(2 * MAX_SLOTS + 1, dtype=torch.int32, device=self.dev)
        self.n_pruned = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._alloc_rows()
        self.slot_of = {}   # kf_id -> slot
        self.stale = 0      # slots freed by drop() whose bits are still in the words (cleared by the next pack)

    def _alloc_rows(self):
        self.to_prune = torch.zeros(self.P, dtype=torch.uint8, device=self.dev)
        self.n_obs = torch.zeros(self.P, dtype=torch.int32, device=self.dev)

    # ---- argument checks ------------------------------------------------------------------------------------------
    def _rows(self, t, what, shape, dtype=torch.int32):
        if not torch.is_tensor(t) or t.device.type != "cuda" or t.device != self.words.device:
            raise _lib.GsajError("%s must be a tensor on %s (there is no CPU path)" % (what, self.words.device))
        if t.dtype != dtype or tuple(t.shape) != tuple(shape):
            raise _lib.GsajError("%s must be %s %s (got %s %s)" % (what, dtype, list(shape), t.dtype, list(t.shape)))
        return t.detach().contiguous()

    def _slot(self, kf_id):
        if kf_id not in self.slot_of:
            raise _lib.GsajError("keyframe %r is not in the covisibility window (it holds %s)" % (kf_id, sorted(self.slot_of)))
        return self.slot_of[kf_id]

    @property
    def slot_mask(self):
        m = 0
        for s in self.slot_of.values():
            m |= 1 << s
        return m

    def _pack(self, n_touched, slots, clear_mask):
        arr = (ctypes.c_int * len(slots))(*slots)
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_covis_pack(len(slots), self.P, n_touched.data_ptr(), arr, clear_mask & 0xFFFFFFFF,
                                                self.words.data_ptr(), _stream(self.dev)), "gsaj_covis_pack")

    # ---- the window -----------------------------------------------------------------------------------------------
    def set_window(self, kf_ids, n_touched):
        """Rebuild the whole window: n_touched [K,P] int32 (BatchContext.n_touched), row k is keyframe kf_ids[k] -> slot k."""
        kf_ids = list(kf_ids)
        if not 1 <= len(kf_ids) <= MAX_SLOTS or len(set(kf_ids)) != len(kf_ids):
            raise _lib.GsajError("set_window: 1..%d distinct keyframe ids (got %r)" % (MAX_SLOTS, kf_ids))
        nt = self._rows(n_touched, "n_touched", (len(kf_ids), self.P))
        self._pack(nt, list(range(len(kf_ids))), 0xFFFFFFFF)
        self.slot_of = {kf: k for k, kf in enumerate(kf_ids)}
        self.stale = 0

    def set_keyframe(self, kf_id, n_touched):
        """Write one keyframe's row, n_touched [P] int32 (FrameContext.n_touched): into its slot if the window holds the id,
        else into the lowest free slot.  The other slots keep their bits."""
        nt = self._rows(n_touched, "n_touched", (self.P,))
        slot = self.slot_of.get(kf_id)
        if slot is None:
            used = self.slot_mask
            free = [s for s in range(MAX_SLOTS) if not (used >> s) & 1]
            if not free:
                raise _lib.GsajError("set_keyframe: all %d slots of the covisibility window are taken; drop() a keyframe first" % MAX_SLOTS)
            slot = free[0]
        self._pack(nt, [slot], self.stale)
        self.slot_of[kf_id] = slot
        self.stale = 0

    def drop(self, kf_id):
        """Free the keyframe's slot.  No launch: queries exclude the slot from now on, the next pack clears its bits."""
        self.stale |= 1 << self._slot(kf_id)
        del self.slot_of[kf_id]

    # ---- the per-frame question -----------------------------------------------------------------------------------
    def query(self, cur_n_touched=None, kf_id=None):
        """The device int32 [65] tensor of gsaj_covis_query for the query set cur_n_touched > 0 (int32 [P], the current frame: it is
        not packed) or the window's keyframe kf_id: [s] = |query & slot s|, [32 + s] = |slot s|, [64] = |query|.  No host read."""
        if (cur_n_touched is None) == (kf_id is None):
            raise _lib.GsajError("query: give either cur_n_touched or kf_id")
        cur = self._rows(cur_n_touched, "cur_n_touched", (self.P,)) if cur_n_touched is not None else None
        qs = self._slot(kf_id) if cur is None else 0
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_covis_query(self.P, self.words.data_ptr(), cur.data_ptr() if cur is not None else None, qs,
                                                 self.slot_mask, self.out.data_ptr(), _stream(self.dev)), "gsaj_covis_query")
        return self.out

    def counts(self, cur_n_touched=None, kf_id=None):
        """query() and ONE device-to-host copy -> ({kf_id: (intersection with the query, count)}, count of the query), Python ints.
        The union with keyframe k is n_query + count_k - intersection_k."""
        o = self.query(cur_n_touched, kf_id).cpu().tolist()
        return {kf: (o[s], o[MAX_SLOTS + s]) for kf, s in self.slot_of.items()}, o[2 * MAX_SLOTS]

    # ---- pruning --------------------------------------------------------------------------------------------------
    def prune_mask(self, window, unique_kfIDs=None, mode="slam", initialized=True):
        """The reference's to_prune (utils/slam_backend.py:246-263) over the keyframes `window` (ids this object holds):
        -> (to_prune uint8 [P], n_pruned int32 [1]), both on the device; self.n_obs [P] holds the observation counts.
        mode "odometry": n_obs < 3.  mode "slam": n_obs <= 3 and unique_kfIDs (int32 [P]) >= the third-newest id of the window, or
        >= 0 while not initialised.  Only the mask is produced: GaussianModel.prune_points(to_prune) removes the rows and returns the plan for compact_plan(); a
        caller who removes them another way follows with compact(~to_prune)."""
        if mode not in PRUNE_MODES:
            raise _lib.GsajError("prune_mask: mode must be one of %s (got %r)" % (sorted(PRUNE_MODES), mode))
        window = list(window)
        wmask = 0
        for kf in window:
            wmask |= 1 << self._slot(kf)
        ids, kf_min = None, 0
        if mode == "slam":
            ids = self._rows(unique_kfIDs, "unique_kfIDs", (self.P,))
            if initialized:
                if len(window) < 3:
                    raise _lib.GsajError("prune_mask: mode 'slam' needs a window of at least 3 keyframes (got %d)" % len(window))
                kf_min = int(sorted(window, reverse=True)[2])
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.gsaj_covis_prune_mask(self.P, self.words.data_ptr(), wmask, ids.data_ptr() if ids is not None else None,
                                                      kf_min, PRUNE_MODES[mode], self.to_prune.data_ptr(), self.n_obs.data_ptr(),
                                                      self.n_pruned.data_ptr(), _stream(self.dev)), "gsaj_covis_prune_mask")
        return self.to_prune, self.n_pruned

    def compact(self, keep):
        """After the caller removed rows from the map: keep the same rows here (bool or uint8 [P]; the reference's
        occ_aware_visibility[idx][~to_prune]).  P becomes the number of kept rows.  Plain torch indexing."""
        if not torch.is_tensor(keep) or keep.device != self.words.device or keep.dtype not in (torch.bool, torch.uint8) \
                or tuple(keep.shape) != (self.P,):
            raise _lib.GsajError("keep must be a bool or uint8 tensor of [%d] on %s" % (self.P, self.words.device))
        words = self.words[keep.bool()]
        if words.numel() == 0:
            raise _lib.GsajError("compact: no row is kept")
        self.words, self.P = words.contiguous(), int(words.numel())
        self._alloc_rows()

    def compact_plan(self, plan):
        """compact() through the plan the map was pruned with (gsaj.pruning.CompactPlan, what GaussianModel.prune_points returns):
        the words go through the same device compaction, with no further host read.  Leaves the window exactly as
        compact(keep) would.  (A plan made from this object's to_prune keeps that tensor: the new buffers are new tensors.)"""
        from .pruning import CompactPlan
        if not isinstance(plan, CompactPlan) or plan.dev != self.words.device or plan.P != self.P:
            raise _lib.GsajError("compact_plan: needs a CompactPlan of %d rows on %s" % (self.P, self.words.device))
        if plan.n_kept == 0:
            raise _lib.GsajError("compact: no row is kept")
        self.words = plan.apply(self.words)[0]
        self.P = int(self.words.numel())
        self._alloc_rows()

    def densify_plan(self, plan):
        """Follow a map update (gsaj.densify.DensifyPlan, what GaussianModel.densify_and_prune returns): a surviving original keeps
        its word, a new row (clone or child) starts with 0, it has been seen from no keyframe yet.  The words go through the
        plan's rows launch, with no further host read."""
        from .densify import DensifyPlan
        if not isinstance(plan, DensifyPlan) or plan.dev != self.words.device or plan.P != self.P:
            raise _lib.GsajError("densify_plan: needs a DensifyPlan of %d rows on %s" % (self.P, self.words.device))
        if plan.n_out == 0:
            raise _lib.GsajError("densify_plan: no row is left")
        self.words = plan.apply([self.words], new_rows="zeros")[0]
        self.P = int(self.words.numel())
        self._alloc_rows()

    # ---- the reference's form ---------------------------------------------------------------------------------------
    def as_reference_dict(self):
        """{kf_id: int64 [P] of 0 / 1}, what the reference calls occ_aware_visibility (new tensors)."""
        return {kf: ((self.words >> s) & 1).long() for kf, s in self.slot_of.items()}

    def from_reference_dict(self, d):
        """Load the reference's {kf_id: [P] of 0 / 1 (any integer or bool dtype)} as the whole window, in the dict's order."""
        if not d:
            raise _lib.GsajError("from_reference_dict: the dict is empty")
        rows = []
        for kf, v in d.items():
            if not torch.is_tensor(v) or v.device != self.words.device or tuple(v.shape) != (self.P,) or v.is_floating_point():
                raise _lib.GsajError("visibility of keyframe %r must be an integer or bool tensor of [%d] on %s" % (kf, self.P, self.words.device))
            rows.append((v != 0).to(torch.int32))
        self.set_window(list(d.keys()), torch.stack(rows))
        return self
