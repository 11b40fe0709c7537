"""NumPy restatement of the covisibility kernels (include/gsaj.h: gsaj_covis_pack / gsaj_covis_query / gsaj_covis_prune_mask)
and a generator of inputs for their tests.  Nothing here is shared with the code under test."""
import numpy as np

MAX_SLOTS = 32
# what a rasteriser's n_touched can hold: a truncation to a byte or a short, or an `== 1` test, shows against these
TOUCH_VALUES = np.array([0, 1, 7, 256, 65536, 2 ** 31 - 1], dtype=np.int32)


def make_case(P, K, density, seed):
    """n_touched int32 [K,P]: each entry is 0 with probability 1 - density, else one of the non-zero TOUCH_VALUES."""
    rng = np.random.default_rng(seed)
    vals = TOUCH_VALUES[1:][rng.integers(0, TOUCH_VALUES.size - 1, size=(K, P))]
    return np.where(rng.uniform(size=(K, P)) < density, vals, 0).astype(np.int32)


def bits_of(slots):
    m = 0
    for s in slots:
        m |= 1 << int(s)
    return m


def pack(words, n_touched, slots, clear_mask):
    """-> new words (uint32 [P]).  words: uint32 [P]; n_touched: [K,P]; slots: K distinct slots."""
    n_touched = np.asarray(n_touched).reshape(len(slots), -1)
    keep = np.uint32(~(int(clear_mask) | bits_of(slots)) & 0xFFFFFFFF)
    out = np.asarray(words, np.uint32) & keep
    for k, s in enumerate(slots):
        out = out | ((n_touched[k] > 0).astype(np.uint32) << np.uint32(s))
    return out.astype(np.uint32)


def query(words, cur_n_touched=None, query_slot=None, slot_mask=0xFFFFFFFF):
    """-> int32 [65]: [s] = |query & slot s|, [32 + s] = |slot s| for s in slot_mask, [64] = |query|."""
    words = np.asarray(words, np.uint32)
    q = (np.asarray(cur_n_touched) > 0) if cur_n_touched is not None else ((words >> np.uint32(query_slot)) & 1).astype(bool)
    out = np.zeros(2 * MAX_SLOTS + 1, np.int32)
    for s in range(MAX_SLOTS):
        if (int(slot_mask) >> s) & 1:
            b = ((words >> np.uint32(s)) & 1).astype(bool)
            out[s], out[MAX_SLOTS + s] = np.count_nonzero(b & q), np.count_nonzero(b)
    out[2 * MAX_SLOTS] = np.count_nonzero(q)
    return out


def prune_mask(words, window_mask, unique_kfIDs, kf_id_min, max_obs):
    """-> (to_prune uint8 [P], n_obs int32 [P], n_pruned)."""
    w = np.asarray(words, np.uint32) & np.uint32(int(window_mask) & 0xFFFFFFFF)
    n_obs = np.zeros(w.shape, np.int32)
    for s in range(MAX_SLOTS):
        n_obs += ((w >> np.uint32(s)) & 1).astype(np.int32)
    prune = n_obs <= max_obs
    if unique_kfIDs is not None:
        prune &= np.asarray(unique_kfIDs) >= kf_id_min
    return prune.astype(np.uint8), n_obs, int(prune.sum())


def prune_arguments(window, mode, initialized):
    """The reference's two modes (utils/slam_backend.py:252-263) -> (max_obs, kf_id_min or None when the ids are not read)."""
    if mode == "odometry":
        return 2, None
    return 3, (sorted(window, reverse=True)[2] if initialized else 0)
