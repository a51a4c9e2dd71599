"""Additive layers (include/mmdx.h, mmdx_pose_add / mmdx_rate_add): the checkers the tests and the fixture generator share.

  * the numpy restatement (add_poses / add_rates), written from the header's text: float32 operations one rounding each, left to
    right as the header's expressions stand, acos and sin as math.acos / math.sin on Python floats rounded to float32;
  * the REAL libmmd through tests/pose_add_driver.cpp, a stand-alone program compiled with g++ where the reference's headers are
    present (they are not on the GPU machines);
  * the fixture tests/golden/pose_add_expect.npz (tests/gen_pose_add_golden.py), its synthetic rows and its coverage conditions.
Nothing compiled here is committed.
"""
import math
import os

import numpy as np

from tests import golden_util as gu
from tests import host_program as hp
from tests import row_blend_ref as rb

FIXTURE = os.path.join(gu.GOLDEN_DIR, "pose_add_expect.npz")
REF_NONE = 0xFFFFFFFF                                                 # MMDX_REF_NONE
MASK_NONE = rb.MASK_NONE
EPS = np.float32(1e-7)
ZERO, ONE = np.float32(0.0), np.float32(1.0)
# the weights the issue sets, as the float32 the entry points take
WEIGHTS = np.array([0.0, 5e-8, 1e-7, 0.25, 0.5, 1 - 5e-8, 1.0, 1.5], np.float32)
TIMES_PER_CASE = 3                                                    # (time a, time b) pairs per (weight, mask id, reference) case


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def _libm(fn, x):
    """float32 array -> float32(fn(double(x))) per element; outside fn's domain (and for NaN / infinities) NaN, as C's libm."""
    def one(v):
        try:
            return fn(v)
        except ValueError:
            return math.nan
    x = np.asarray(x, np.float32)
    return np.array([one(float(v)) for v in x.reshape(-1)], np.float64).astype(np.float32).reshape(x.shape)


def q_mul(a, q):
    """Quaternion::operator* (L/util/math_impl.inl:510-517); [..., 4] as i, j, k, e."""
    ai, aj, ak, ae = (a[..., k] for k in range(4))
    qi, qj, qk, qe = (q[..., k] for k in range(4))
    return np.stack([(ae * qi + ai * qe + aj * qk) - ak * qj,
                     (ae * qj + aj * qe + ak * qi) - ai * qk,
                     (ae * qk + ai * qj + ak * qe) - aj * qi,
                     ae * qe - (ai * qi + aj * qj + ak * qk)], -1).astype(np.float32)


def q_inverse(a):
    """Quaternion::Inverse (:474-477): Conjugate() * (1 / (i*i + j*j + k*k + e*e))."""
    ai, aj, ak, ae = (a[..., k] for k in range(4))
    n = ONE / (ai * ai + aj * aj + ak * ak + ae * ae)
    return np.stack([-ai * n, -aj * n, -ak * n, ae * n], -1).astype(np.float32)


def q_identity(shape):
    q = np.zeros(tuple(shape) + (4,), np.float32)
    q[..., 3] = 1
    return q


def slerp_terms(b):
    """comega after the flip, the flip, omega = float32(acos(comega)) of SLerp(Identity, b) (:1318-1323)."""
    a = q_identity(b.shape[:-1])
    comega = a[..., 3] * b[..., 3] + a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]
    flip = comega < 0
    comega = np.where(flip, -comega, comega).astype(np.float32)
    return comega, flip, _libm(math.acos, comega)


def q_slerp_from_identity(b, l):
    """SLerp(Identity, b)[l] (:1312-1337), l float32 [...]."""
    a = q_identity(b.shape[:-1])
    l = np.asarray(l, np.float32)
    _, flip, omega = slerp_terms(b)
    rs = ONE / _libm(math.sin, omega)
    p = _libm(math.sin, (ONE - l) * omega) * rs
    l2 = _libm(math.sin, l * omega) * rs
    l2 = np.where(flip, -l2, l2).astype(np.float32)
    mixed = a * p[..., None] + b * l2[..., None]
    return np.where((omega > EPS)[..., None], mixed, a).astype(np.float32)


def reference_rows(refs, ref_ids, n, item_shape):
    """-> (R f32 [n, ...] (zeros where there is none), has_ref bool [n], row_is_a bool [n]): ref_ids None = REF_NONE for everyone; an
    id that is neither below n_refs nor REF_NONE makes the row A (the device rule; the host call refuses it)."""
    r = np.full(n, REF_NONE, np.uint32) if ref_ids is None else np.asarray(ref_ids, np.uint32).reshape(n)
    refs = np.zeros((0,) + tuple(item_shape), np.float32) if refs is None or ref_ids is None else np.asarray(refs, np.float32)
    has = r < refs.shape[0]
    rows = np.zeros((n,) + tuple(item_shape), np.float32)
    if has.any():
        rows[has] = refs[r[has]]
    return rows, has, (r != REF_NONE) & ~has


def mixing(weights, items, masks=None, mask_ids=None, refs=None, ref_ids=None):
    """-> (e f32 [N, items], mix bool [N, items]): the effective weights and where B (and R) are read."""
    e = rb.effective_weights(weights, items, masks, mask_ids)
    n_refs = 0 if refs is None or ref_ids is None else np.asarray(refs).shape[0]
    r = np.full(e.shape[0], REF_NONE, np.uint32) if ref_ids is None else np.asarray(ref_ids, np.uint32).reshape(-1)
    row_is_a = (r != REF_NONE) & (r >= n_refs)
    with np.errstate(invalid="ignore"):
        return e, (e >= EPS) & ~row_is_a[:, None]


def add_poses(a, b, weights, masks=None, mask_ids=None, refs=None, ref_ids=None):
    """a, b f32 [N, items, 8] (t.xyz, 0, q.xyzw), refs f32 [n_refs, items, 8] -> [N, items, 8], the header's rules 1-8."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, items = a.shape[:2]
    e, mix = mixing(weights, items, masks, mask_ids, refs, ref_ids)
    rows, has, _ = reference_rows(refs, ref_ids, n, (items, 8))
    with np.errstate(all="ignore"):
        dq = np.where(has[:, None, None], q_mul(b[..., 4:], q_inverse(rows[..., 4:])), b[..., 4:]).astype(np.float32)
        dt = np.where(has[:, None, None], b[..., :3] - rows[..., :3], b[..., :3]).astype(np.float32)
        mt = ZERO + dt * e[..., None]
        mq = q_mul(q_identity((n, items)), q_slerp_from_identity(dq, e))
        out = np.zeros_like(a)
        out[..., 4:] = q_mul(mq, a[..., 4:])
        out[..., :3] = mt + a[..., :3]
    return np.where(mix[..., None], out, a).astype(np.float32)


def add_rates(a, b, weights, masks=None, mask_ids=None, refs=None, ref_ids=None):
    """a, b f32 [N, items], refs f32 [n_refs, items] -> [N, items]: a + (b - ref) * e, rule 9."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, items = a.shape
    e, mix = mixing(weights, items, masks, mask_ids, refs, ref_ids)
    rows, has, _ = reference_rows(refs, ref_ids, n, (items,))
    with np.errstate(all="ignore"):
        d = np.where(has[:, None], b - rows, b).astype(np.float32)
        out = a + d * e
    return np.where(mix, out, a).astype(np.float32)


# ---- the bone-morph property ----------------------------------------------------------------------
def morph_rig(seed=11, nb=20):
    """A small FK rig in which every bone is the target of at most one bone-morph application (T, Q), and the same applications as
    layer rows.  -> dict: rest, parent, level, flags; morphs (the table vmd.Skeleton and the oracle take: four bone morphs over
    disjoint bones); rates f32 [NI, 4]; poses f32 [NI, NB, 8] (P); b f32 [NI, NB, 8] (the (T, Q) rows; a NaN pattern in every
    untouched bone); weights f32 [NI], masks f32 [NI + 1, NB], mask_ids u32 [NI]: instance i < NI - 1 has weight 1 and the mask row
    that holds each touched bone's rate, the last instance has one rate for every morph as its weight and a 0 / 1 mask row."""
    from simple_mmd_renderer_amd import synth
    rest, parent, level, flags = synth.make_skeleton(nb, seed)
    rng = np.random.RandomState(seed)
    bones = [[1, 4, 7], [2, 9], [11], [13, 15, 17, 19]]
    off, index, value, rot = [0], [], [], []
    for k, bs in enumerate(bones):
        for b in bs:
            q = rng.normal(size=4)
            q = q / np.linalg.norm(q) * (0.9 if b == 9 else 1.0)          # one that is not of unit length
            if b == 15:
                q = np.array([0, 0, 0, 1.0])                              # a pure translation
            if b == 17:
                q[3] = -abs(q[3])                                          # the other hemisphere
            index.append(b); value.append(rng.uniform(-0.5, 0.5, 3)); rot.append(q)
        off.append(len(index))
    morphs = dict(type=np.full(len(bones), 2, np.int32), offset=np.asarray(off, np.uint32), index=np.asarray(index, np.uint32),
                  value=np.asarray(value, np.float32).reshape(-1, 3), rotation=np.asarray(rot, np.float32).reshape(-1, 4))
    rates = np.array([[0.3, 1.0, 1.7, 5e-8], [1, 1, 1, 1], [0.5, 0, -0.5, 0.25], [1e-7, 2.5, 0.125, 1 - 5e-8], [0.7, 0.7, 0.7, 0.7]],
                     np.float32)
    ni = rates.shape[0]
    poses = np.zeros((ni, nb, 8), np.float32)
    poses[..., :3] = rng.uniform(-1.5, 1.5, (ni, nb, 3))
    q = rng.normal(size=(ni, nb, 4))
    poses[..., 4:] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    b = np.full((ni, nb, 8), np.array([0x7FC0BAD1], np.uint32).view(np.float32)[0], np.float32)
    masks = np.zeros((ni + 1, nb), np.float32)
    for k, bs in enumerate(bones):
        for b_ in bs:
            e = index.index(b_)
            b[:, b_, :3], b[:, b_, 3], b[:, b_, 4:] = morphs["value"][e], 0, morphs["rotation"][e]
            masks[:ni, b_] = rates[:, k]
            masks[ni, b_] = 1
    weights = np.r_[np.ones(ni - 1, np.float32), rates[ni - 1, 0]].astype(np.float32)
    mask_ids = np.r_[np.arange(ni - 1), ni].astype(np.uint32)
    return dict(rest=rest, parent=parent, level=level, flags=flags, morphs=morphs, rates=rates, poses=poses, b=b, weights=weights,
                masks=masks, mask_ids=mask_ids)


# ---- the real libmmd ------------------------------------------------------------------------------
def build_driver() -> str:
    return hp.build("pose_add_driver", [os.path.join(hp.TESTS, "pose_add_driver.cpp")], strict=False, include=[hp.REF_INC])


def driver_expect(a_poses, b_poses, a_rates, b_rates, weights, bone_masks, morph_masks, mask_ids, pose_refs, rate_refs, ref_ids):
    """The same operands through libmmd's own operators (tests/pose_add_driver.cpp), one record per (row, item) -> poses f32
    [N, NB, 8], rates f32 [N, NM]."""
    a_poses, b_poses = np.asarray(a_poses, np.float32), np.asarray(b_poses, np.float32)
    a_rates, b_rates = np.asarray(a_rates, np.float32), np.asarray(b_rates, np.float32)
    n, nb = a_poses.shape[:2]
    nm = a_rates.shape[1]
    ep, _ = mixing(weights, nb, bone_masks, mask_ids, pose_refs, ref_ids)
    er, _ = mixing(weights, nm, morph_masks, mask_ids, rate_refs, ref_ids)
    rp, has, bad = reference_rows(pose_refs, ref_ids, n, (nb, 8))
    rr, _, _ = reference_rows(rate_refs, ref_ids, n, (nm,))
    assert not bad.any(), "the driver takes REF_NONE or a valid reference id"
    pose_t = np.dtype([("a", np.float32, 8), ("b", np.float32, 8), ("r", np.float32, 8), ("e", np.float32), ("has", np.uint32)])
    rate_t = np.dtype([("a", np.float32), ("b", np.float32), ("r", np.float32), ("e", np.float32), ("has", np.uint32)])
    assert pose_t.itemsize == 26 * 4 and rate_t.itemsize == 5 * 4
    pr, rt = np.zeros((n, nb), pose_t), np.zeros((n, nm), rate_t)
    pr["a"], pr["b"], pr["r"], pr["e"], pr["has"] = a_poses, b_poses, rp, ep, has[:, None]
    rt["a"], rt["b"], rt["r"], rt["e"], rt["has"] = a_rates, b_rates, rr, er, has[:, None]
    out = hp.run_files(build_driver(), lambda f: f.write(np.array([n * nb, n * nm], np.uint32).tobytes() + pr.tobytes() + rt.tobytes()),
                       lambda f: np.fromfile(f, np.float32))
    assert out.size == n * nb * 8 + n * nm
    return out[:n * nb * 8].reshape(n, nb, 8).copy(), out[n * nb * 8:].reshape(n, nm).copy()


# ---- the fixture ----------------------------------------------------------------------------------
def _pose(t=(0, 0, 0), q=(0, 0, 0, 1)):
    return np.array(list(t) + [0] + list(q), np.float32)


INF = np.float32(np.inf)
# what the clips cannot reach, as (A, B, R) items; each is used once without and once with its reference.  No item makes a NaN in
# its result (the sign and payload of a produced NaN are outside the contract and differ between processors).
SYNTHETIC_ITEMS = [
    # comega < 0: the flip, without a reference (B.q.e < 0) and through one (B.q * R.q.Inverse() lands in the other hemisphere)
    (_pose((1, 2, 3), (0.1, 0.2, 0.3, 0.9)), _pose((0.5, -1, 2), (0.2, -0.4, 0.1, -0.8)), _pose((0.25, 0, 0), (0.6, 0.1, -0.7, 0.3))),
    (_pose((0, 1, 0), (0, 0.6, 0, 0.8)), _pose((1, 1, 1), (0.7, 0, 0.1, -0.7)), _pose((0, 0, 1), (-0.7, 0.1, 0, 0.7))),
    # d.q equal to identity: omega <= 1e-7, SLerp returns Identity (B.q == R.q == an exact unit quaternion; B.q identity itself)
    (_pose((1, 2, 3), (0.3, 0.1, 0.2, 0.9)), _pose((3, 2, 1), (0, 0, 0, 1)), _pose((1, 1, 1), (0, 0, 0, 1))),
    (_pose((-1, 0.5, 2), (0.5, 0.5, 0.5, 0.5)), _pose((0.125, 0, -4), (0, 0, 0, 1)), _pose((0, 2, 0), (0, 0, 0, 1))),
    # not normalised, |comega| > 1: acos is NaN, omega > 1e-7f is false, Identity
    (_pose((0, 0, 0), (0.1, 0.2, 0.3, 0.9)), _pose((1, 0, 0), (0.5, 0, 0, 1.5)), _pose((0, 0, 0), (0, 0, 0, 0.5))),
    (_pose((2, 2, 2), (0, 1, 0, 0)), _pose((0, 1, 0), (0, 0, 0, -2.0)), _pose((0, 0, 0), (0, 0, 0, 0.25))),
    # not normalised, |comega| < 1: used as given
    (_pose((0, 0, 0), (0.2, 0.2, 0.2, 1.1)), _pose((1, 0, 1), (0.3, 0.1, 0, 0.6)), _pose((0, 1, 0), (0.2, 0, 0.4, 1.3))),
    # -0.0 translations in A, B and R
    (_pose((-0.0, -0.0, 1), (0, 0, 0.6, 0.8)), _pose((-0.0, 2, -0.0), (0.6, 0, 0, 0.8)), _pose((-0.0, -0.0, -0.0), (0, 0.6, 0, 0.8))),
    (_pose((-0.0, -0.0, -0.0), (0, 0, 0, 1)), _pose((-0.0, -0.0, -0.0), (0, 0.8, 0, 0.6)), _pose((0, 0, 0), (0, 0, 0, 1))),
    # infinities in translations (never two of opposite sign in one channel) and in B.q (comega is NaN: Identity)
    (_pose((1, 2, 3), (0, 0, 0.6, 0.8)), _pose((INF, -INF, 1), (0.6, 0, 0, 0.8)), _pose((0, 0, -INF), (0, 0.6, 0, 0.8))),
    (_pose((INF, 2, -INF), (0, 0.6, 0, 0.8)), _pose((1, 1, 1), (INF, 0, 0, 0.5)), _pose((0, 0, 0), (0, 0, 0, 1))),
]
SYNTHETIC_RATES = [(0.5, 0.75, 0.25), (-0.0, -0.0, -0.0), (1.0, INF, 0.5), (-INF, 0.5, 0.25), (0.25, 1.5, -INF), (1.0, -3.0, 2.0)]


def synthetic_rows(nb, nm):
    """-> (a_poses, b_poses, ref_pose_row, a_rates, b_rates, ref_rate_row, weights): one row of NB / NM items per weight of WEIGHTS,
    item j from SYNTHETIC_ITEMS[j % len] and SYNTHETIC_RATES[j % len] in every row."""
    n = len(WEIGHTS)
    pick = np.arange(nb) % len(SYNTHETIC_ITEMS)
    ap, bp, rp = (np.stack([SYNTHETIC_ITEMS[k][c] for k in pick]).astype(np.float32) for c in range(3))
    pick = np.arange(nm) % len(SYNTHETIC_RATES)
    ar, br, rr = (np.array([SYNTHETIC_RATES[k][c] for k in pick], np.float32) for c in range(3))
    tile = lambda x: np.ascontiguousarray(np.broadcast_to(x, (n,) + x.shape))          # noqa: E731
    return tile(ap), tile(bp), rp, tile(ar), tile(br), rr, WEIGHTS.copy()


def fixture():
    """dict: weights f32 [N], mask_ids u32 [N], ref_ids u32 [N], bone_masks f32 [4, NB], morph_masks f32 [4, NM], pose_refs f32
    [2, NB, 8], rate_refs f32 [2, NM] (row 0: clip b at time 0, row 1: synthetic), a_poses / b_poses / expect_poses f32 [N, NB, 8],
    a_rates / b_rates / expect_rates f32 [N, NM], times_a / times_b f64 [N] (NaN for the synthetic rows), synthetic bool [N]."""
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


def operands(z, what):
    """The positional operands of add_poses / add_rates (and of the test's runners) from the fixture: what = "poses" or "rates"."""
    if what == "poses":
        return z["a_poses"], z["b_poses"], z["weights"], z["bone_masks"], z["mask_ids"], z["pose_refs"], z["ref_ids"]
    return z["a_rates"], z["b_rates"], z["weights"], z["morph_masks"], z["mask_ids"], z["rate_refs"], z["ref_ids"]


def check_coverage(z):
    """Conditions on the fixture, not measurements."""
    nb, nm = z["a_poses"].shape[1], z["a_rates"].shape[1]
    syn = z["synthetic"]
    assert 200 <= syn.size <= 400 and syn.sum() == 2 * len(WEIGHTS)
    # every weight under every mask id with and without a reference, among the clip rows
    for w in WEIGHTS:
        for m in list(range(rb.N_MASKS)) + [MASK_NONE]:
            for r in (REF_NONE, 0):
                rows = ~syn & (z["weights"].view(np.uint32) == w.view(np.uint32)) & (z["mask_ids"] == m) & (z["ref_ids"] == r)
                assert rows.sum() == TIMES_PER_CASE, (w, m, r)
    assert set(z["ref_ids"][syn]) == {REF_NONE, 1} and (z["mask_ids"][syn] == MASK_NONE).all()
    for what, items in (("poses", nb), ("rates", nm)):
        a, b, w, masks, ids, refs, rids = operands(z, what)
        e, mix = mixing(w, items, masks, ids, refs, rids)
        for m in list(range(rb.N_MASKS)) + [MASK_NONE]:
            assert mix[ids == m].any() and (~mix[ids == m]).any(), (what, m)
        # through the multiply: the instance weight alone passes the test, the effective weight does not (1e-7 * 0.5), and both pass
        wide = np.broadcast_to((w >= EPS).reshape(-1, 1), mix.shape)
        assert (wide & ~mix).any() and (wide & mix & (e != np.broadcast_to(w.reshape(-1, 1), e.shape))).any()
        assert (e[mix] > 1).any() and (e[mix] == 1).any() and (e[mix] < 1).any()            # exaggerated, whole, partial
    # the quaternion cases, among the mixing items
    a, b, w, masks, ids, refs, rids = operands(z, "poses")
    e, mix = mixing(w, nb, masks, ids, refs, rids)
    rows, has, _ = reference_rows(refs, rids, w.size, (nb, 8))
    with np.errstate(all="ignore"):
        dq = np.where(has[:, None, None], q_mul(b[..., 4:], q_inverse(rows[..., 4:])), b[..., 4:]).astype(np.float32)
        comega, flip, omega = slerp_terms(dq)
        for h in (False, True):                                       # without and with a reference
            sel = mix & (has == h)[:, None]
            assert (flip & sel).sum() >= 8 and (~flip & sel).sum() >= 8, h
            assert (sel & (omega <= EPS)).sum() >= 4, h                # d.q equal to identity
            assert (sel & (comega > 1) & np.isnan(omega)).sum() >= 4, h    # not normalised: acos NaN, Identity
            assert (sel & (omega > EPS)).sum() >= 8, h
        neg_zero = lambda x: (x == 0) & np.signbit(x)                # noqa: E731
        assert (mix & neg_zero(a[..., :3]).any(-1)).sum() >= 4 and (mix & neg_zero(b[..., :3]).any(-1)).sum() >= 4
        assert (mix & has[:, None] & neg_zero(rows[..., :3]).any(-1)).sum() >= 2
        assert (mix & np.isinf(b[..., :3]).any(-1)).sum() >= 2 and (mix & np.isinf(a[..., :3]).any(-1)).sum() >= 2
        assert (mix & np.isinf(b[..., 4:]).any(-1)).sum() >= 2 and (mix & has[:, None] & np.isinf(rows[..., :3]).any(-1)).sum() >= 1
    assert not np.isnan(z["expect_poses"]).any() and not np.isnan(z["expect_rates"]).any()
    ar, br = z["a_rates"], z["b_rates"]
    _, mixr = mixing(z["weights"], nm, z["morph_masks"], z["mask_ids"], z["rate_refs"], z["ref_ids"])
    assert (mixr & neg_zero(ar)).any() and (mixr & np.isinf(br)).any() and (mixr & np.isinf(ar)).any()
