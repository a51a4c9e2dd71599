"""The masked blend of two evaluated pose or rate arrays (include/mmdx.h, mmdx_pose_blend / mmdx_rate_blend): the checkers the
tests and the fixture generator share.

  * the numpy restatement: motion_blend_ref.blend_poses / blend_rates, imported, applied with one weight per (row, item) -- the
    effective weight float32(weights[i]) * float32(mask value), one multiply;
  * the REAL libmmd through tests/motion_blend_driver.cpp as it is: one call per bone or morph with that item's effective weights;
  * the fixture tests/golden/row_blend_expect.npz (tests/gen_row_blend_golden.py), its inputs and its coverage conditions.
Nothing compiled here is committed.
"""
import ctypes as C
import os

import numpy as np

from tests import golden_util as gu
from tests import motion_blend_ref as mb
from tests import motion_time_ref as mt

FIXTURE = os.path.join(gu.GOLDEN_DIR, "row_blend_expect.npz")
MASK_NONE = 0xFFFFFFFF                                                # MMDX_MASK_NONE
MASK_VALUES = np.array([0.0, 0.25, 0.5, 1.0], np.float32)             # what the fixture's mask rows are drawn from
N_MASKS = 4


def effective_weights(weights, items, masks=None, mask_ids=None):
    """weights f32 [N], masks f32 [n_masks, items], mask_ids u32 [N] or None -> e f32 [N, items]: weights[i] * mv, mv = 1 for
    MASK_NONE, masks[m] for m < n_masks, 0 for any other id.  One float32 multiply per item."""
    w = np.asarray(weights, np.float32).reshape(-1, 1)
    mv = np.ones((w.shape[0], items), np.float32)
    if mask_ids is not None:
        ids = np.asarray(mask_ids, np.uint32).reshape(-1)
        masks = np.zeros((0, items), np.float32) if masks is None else np.asarray(masks, np.float32).reshape(-1, items)
        for i, m in enumerate(ids):
            if m != MASK_NONE:
                mv[i] = masks[m] if m < masks.shape[0] else np.float32(0)
    with np.errstate(all="ignore"):
        return (w * mv).astype(np.float32)


def blend_poses(a, b, weights, masks=None, mask_ids=None):
    """a, b f32 [N, items, 8] -> [N, items, 8]: motion_blend_ref.blend_poses with the effective weight of every (row, item)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, items = a.shape[:2]
    e = effective_weights(weights, items, masks, mask_ids)
    return mb.blend_poses(a.reshape(n * items, 1, 8), b.reshape(n * items, 1, 8), e.reshape(-1)).reshape(n, items, 8)


def blend_rates(a, b, weights, masks=None, mask_ids=None):
    """a, b f32 [N, items] -> [N, items]."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, items = a.shape
    e = effective_weights(weights, items, masks, mask_ids)
    return mb.blend_rates(a.reshape(n * items, 1), b.reshape(n * items, 1), e.reshape(-1)).reshape(n, items)


def mask_rows(items, seed):
    """N_MASKS rows over `items` items, values drawn from MASK_VALUES; every value occurs in every row when items >= 4."""
    rng = np.random.RandomState(seed)
    rows = []
    for _ in range(N_MASKS):
        row = MASK_VALUES[np.arange(items) % MASK_VALUES.size]
        rows.append(row[rng.permutation(items)])
    return np.stack(rows).astype(np.float32)


# ---- the real libmmd ------------------------------------------------------------------------------
def driver_expect(bone_names, morph_names, clips_a, times_a, clips_b, times_b, e_bones, e_morphs):
    """libmmd's blend of (clip a, time a) with (clip b, time b) per row, bone j at the weights e_bones[:, j], morph k at
    e_morphs[:, k] -> poses f32 [N, NB, 8], rates f32 [N, NM]: tests/motion_blend_driver.cpp, one call per bone or morph."""
    lib = C.CDLL(mb.build_driver())
    lib.mbd_load.restype = C.c_void_p
    ca, cb = np.ascontiguousarray(clips_a, np.uint32), np.ascontiguousarray(clips_b, np.uint32)
    ta, tb = np.ascontiguousarray(times_a, np.float64), np.ascontiguousarray(times_b, np.float64)
    n = ca.size

    def run(fn, paths, names, e, width):
        hs = [lib.mbd_load(str(p).encode()) for p in paths]
        if not all(hs):
            raise RuntimeError("libmmd VmdReader failed on one of " + repr(paths))
        arr = (C.c_void_p * len(hs))(*hs)
        out = np.zeros((n, len(names)) + ((width,) if width > 1 else ()), np.float32)
        one = np.zeros((n, width), np.float32)
        for j, name in enumerate(names):
            w = np.ascontiguousarray(e[:, j], np.float32)
            fn(arr, C.c_uint32(len(hs)), name.encode("shift_jis"), C.c_uint32(n), mt.ptr(ca, C.c_uint32), mt.ptr(ta, C.c_double),
               mt.ptr(cb, C.c_uint32), mt.ptr(tb, C.c_double), mt.ptr(w, C.c_float), mt.ptr(one, C.c_float))
            out[:, j] = one if width > 1 else one[:, 0]
        for h in hs:
            lib.mbd_destroy(C.c_void_p(h))
        return out
    return (run(lib.mbd_blend_bone, mb.BONE_VMDS, bone_names, np.asarray(e_bones, np.float32), 8),
            run(lib.mbd_blend_morph, mb.MORPH_VMDS, morph_names, np.asarray(e_morphs, np.float32), 1))


# ---- the fixture ----------------------------------------------------------------------------------
def fixture():
    """dict: clips_a / clips_b u32 [N], times_a / times_b f64 [N], weights f32 [N], mask_ids u32 [N], bone_masks f32 [4, NB],
    morph_masks f32 [4, NM], bone_names [NB], morph_names [NM], a_poses / b_poses / expect_poses f32 [N, NB, 8], a_rates / b_rates
    / expect_rates f32 [N, NM]."""
    z = np.load(FIXTURE)
    out = {k: z[k] for k in z.files}
    out["bone_names"] = [str(n) for n in z["bone_names"]]
    out["morph_names"] = [str(n) for n in z["morph_names"]]
    return out


def check_coverage(z):
    """Conditions on the fixture, not measurements: both hemispheres among the mixed (row, bone) pairs, each side under every mask
    row, and effective weights that change side through the multiply at both thresholds."""
    nb, nm = z["a_poses"].shape[1], z["a_rates"].shape[1]
    for e, n_items in ((effective_weights(z["weights"], nb, z["bone_masks"], z["mask_ids"]), nb),
                       (effective_weights(z["weights"], nm, z["morph_masks"], z["mask_ids"]), nm)):
        side = mb.side_of(e)
        for m in list(range(N_MASKS)) + [MASK_NONE]:
            rows = z["mask_ids"] == m
            assert rows.any(), m
            for s in (0, 1, 2):
                assert (side[rows] == s).any(), (m, s, n_items)
    e = effective_weights(z["weights"], nb, z["bone_masks"], z["mask_ids"])
    side = mb.side_of(e)
    dots = mb.quaternion_dots(z["a_poses"], z["b_poses"])[side == 2]
    assert (dots < 0).sum() >= 8 and (dots >= 0).sum() >= 8, ((dots < 0).sum(), (dots >= 0).sum())
    # through the multiply: the instance weight alone is on one side of a threshold, the effective weight on the other
    w_side = np.broadcast_to(mb.side_of(z["weights"]).reshape(-1, 1), side.shape)
    assert ((w_side == 2) & (side == 0)).any()          # e.g. 1e-7 * 0.5: below 1e-7
    assert ((w_side == 2) & (side == 2)).any()          # e.g. 0.5 * 0.5: still at or above 1e-7
    assert ((w_side == 1) & (side == 2)).any()          # e.g. 1.0 * 0.25: at or below 1 - 1e-7
    assert ((w_side == 1) & (side == 1) & (e != np.broadcast_to(z["weights"].reshape(-1, 1), e.shape))).any()   # 2.0 * 0.5: above
    for weight in mb.WEIGHTS:
        assert (z["weights"].view(np.uint32) == np.float32(weight).view(np.uint32)).sum() >= len(mb.PAIRS), weight
    assert {(int(a), int(b)) for a, b in zip(z["clips_a"], z["clips_b"])} == set(mb.PAIRS)
