"""Root motion that turns (mmdx_animator_root_motion_turn, include/mmdx.h): what the tests and the fixture generator share.

  * apply(): a restatement of the call in numpy, written from the header's text -- whole arrays at a time, masks instead of
    branches, every numpy operation one IEEE rounding.  The clocks are tests/root_motion_ref.plan's (steps 1-2 of the plain call);
    (T, Q), the root's translation and rotation at those instants, come from the caller: the golden rows carry libmmd's, a GPU test
    takes them from the pinned MotionSet.eval_bones_time;
  * chain(): the same step as float64 matrices, W_p' = W_root(t1) * W_root(t0)^-1 * W_p, for the closure tests;
  * the clips: tests/root_motion_ref's six and tests/golden/root_q8.vmd, a root whose rotations are drawn from the quaternion group
    {+-1, +-i, +-j, +-k} and whose translations are dyadic, so that every value of its walk is exact;
  * the two stand-alone programs: tests/root_turn_driver.cpp (the REAL libmmd; built where the reference's headers are) and
    tests/root_turn_math_driver.cpp (csrc/root_math.hpp for the host, plain and under the sanitizers), both built and run by
    tests/host_program.py;
  * the fixture tests/golden/root_turn_expect.npz (tests/gen_root_turn_golden.py).
Nothing compiled here is committed.
"""
import os

import numpy as np

from tests import animator_ref as ar
from tests import golden_util as gu
from tests import host_program as hp
from tests import motion_blend_ref as mb
from tests import root_motion_ref as rm

F = np.float32
HERE = hp.TESTS
FIXTURE = os.path.join(gu.GOLDEN_DIR, "root_turn_expect.npz")
Q8_VMD = os.path.join(gu.GOLDEN_DIR, "root_q8.vmd")
NONE = ar.NONE
ROOT_NORMALIZE = 1 << 14                              # MMDX_ROOT_NORMALIZE
ROOT_NAME = rm.ROOT_NAME
T0, T1, NEAR, FAR = rm.T0, rm.T1, rm.NEAR, rm.FAR
IDENTITY = np.array([0, 0, 0, 1], F)

# ---- the clips ------------------------------------------------------------------------------------------------------------------
# tests/root_motion_ref's six clips, and root_q8 as clip 6: a loop of 60 frames = 2.0 s
CLIP_FILES = rm.CLIP_FILES + ("q8",)
CLIP_FRAMES = rm.CLIP_FRAMES + (60,)
CLIP_ROWS = rm.CLIP_ROWS + ((60 / 30.0, ar.LOOP, NONE, 0.0),)
N_CLIPS = len(CLIP_FILES)
Q8 = 6
# root_q8's root keys: frame, translation, rotation {x, y, z, w}.  Linear curves; the second key is a half-turn yaw.
Q8_KEYS = ((0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), (15, (0.5, 0.0, 1.0), (0.0, 1.0, 0.0, 0.0)),
           (30, (1.5, 0.25, 1.0), (1.0, 0.0, 0.0, 0.0)), (45, (1.5, 0.25, -0.5), (0.0, 0.0, 1.0, 0.0)),
           (60, (2.0, 0.5, 0.75), (0.0, 0.0, 0.0, -1.0)))
Q8_DT, Q8_STEPS = 0.5, 12                             # every sample lands on a key; twelve steps are three laps


def clip_paths():
    return [Q8_VMD if n == "q8" else rm.VMDS[n] for n in CLIP_FILES]


def table():
    return ar.table_of(ar.resolved_rows(CLIP_ROWS, CLIP_FRAMES))


def root_bank():
    """Every clip bound to the root's name alone -- a one-bone bank, root_bone = 0."""
    from simple_mmd_renderer_amd import vmd
    vs = [vmd.Vmd(p) for p in clip_paths()]
    bms = [v.bind_bones([ROOT_NAME]) for v in vs]
    ms = vmd.MotionSet(bms)
    for x in bms + vs:
        x.close()
    return ms


def write_q8():
    """tests/golden/root_q8.vmd (tests/gen_root_turn_golden.py writes it; it is committed): the root keys above, and one bone of
    rig_small that an in-place copy must leave alone."""
    from simple_mmd_renderer_amd import vmd
    name = rm.rig_small_names()[1]
    keys = [(ROOT_NAME, f, t, q, None) for f, t, q in Q8_KEYS]
    keys += [(name, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), None), (name, 60, (0.25, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), None)]
    with open(Q8_VMD, "wb") as f:
        f.write(vmd.write_vmd(keys, []))


def q8_at(times):
    """(T f32 [..., 3], Q f32 [..., 4]) of root_q8's root at `times`, every one of which is a key's (the GPU test holds
    MotionSet.eval_bones_time to these same values)."""
    frames = np.asarray(times, np.float64) * 30.0
    by_frame = {f: (t, q) for f, t, q in Q8_KEYS}
    assert all(float(f) in by_frame for f in frames.reshape(-1)), frames
    t = np.array([by_frame[float(f)][0] for f in frames.reshape(-1)], F).reshape(frames.shape + (3,))
    q = np.array([by_frame[float(f)][1] for f in frames.reshape(-1)], F).reshape(frames.shape + (4,))
    return t, q


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def q_mul(a, q):
    """Quaternion::operator* (L/util/math_impl.inl:510-517), {x, y, z, w} = libmmd's {i, j, k, e}."""
    ax, ay, az, aw = (a[..., k] for k in range(4))
    qx, qy, qz, qw = (q[..., k] for k in range(4))
    return np.stack([(aw * qx + ax * qw + ay * qz) - az * qy, (aw * qy + ay * qw + az * qx) - ax * qz,
                     (aw * qz + ax * qy + az * qw) - ay * qx, aw * qw - (ax * qx + ay * qy + az * qz)], -1)


def q_inverse(a):
    """Quaternion::Inverse (:474-477): the conjugate times 1 / (the squared norm, summed left to right)."""
    x, y, z, w = (a[..., k] for k in range(4))
    n = F(1) / (x * x + y * y + z * z + w * w)
    return np.stack([-x * n, -y * n, -z * n, w * n], -1)


def q_normalize(a):
    """Quaternion::Normalize (:457-465) with math::sqrt (L/util/math.inl:28-30)."""
    x, y, z, w = (a[..., k] for k in range(4))
    s = x * x + y * y + z * z + w * w
    n = F(1) / np.sqrt(s.astype(np.float64)).astype(F)
    return np.stack([x * n, y * n, z * n, w * n], -1)


def rotate(v, q):
    """rotate(v, q.ToRotateMatrix()) (:1032-1038 over :540-563): three-term sums left to right; q is not normalised."""
    i, j, k, e = (q[..., c] for c in range(4))
    ii, jj, kk, ij, jk, ki, ie, je, ke = i * i, j * j, k * k, i * j, j * k, i * k, i * e, j * e, k * e
    one, two = F(1), F(2)
    m = ((one - two * (jj + kk), two * (ij + ke), two * (ki - je)),
         (two * (ij - ke), one - two * (kk + ii), two * (jk + ie)),
         (two * (ki + je), two * (jk - ie), one - two * (ii + jj)))
    x, y, z = (v[..., c] for c in range(3))
    return np.stack([x * m[0][c] + y * m[1][c] + z * m[2][c] for c in range(3)], -1)


def leg(t0, q0, t1, q1):
    """From (t0, q0) to (t1, q1): qi = q0.Inverse(); D = rotate(t1 - t0, M(qi)); dq = qi * q1."""
    qi = q_inverse(q0)
    return rotate(t1 - t0, qi), q_mul(qi, q1)


def apply(state, tab, dt, t, q, axes, normalize, placements):
    """The call.  t f32 [N, 2, 4, 3] and q f32 [N, 2, 4, 4]: (T, Q) at the instants of root_motion_ref.plan() (ignored where not
    sampled); axes: a scalar or u32 [N]; normalize: a scalar or bool [N]; placements f32 [N, 8] -> (the placements after the call,
    events: name -> bool [N])."""
    pl = rm.plan(state, tab, dt)
    n = state["clips_a"].size
    dt = np.broadcast_to(np.asarray(dt, np.float64), (n,))
    axes = np.broadcast_to(np.asarray(axes, np.uint32), (n,))
    normalize = np.broadcast_to(np.asarray(normalize, bool), (n,))
    p = np.array(placements, F).reshape(n, 8)
    with np.errstate(all="ignore"):
        t = np.where(pl["sampled"][..., None], np.asarray(t, F), F(0))
        q = np.where(pl["sampled"][..., None], np.asarray(q, F), IDENTITY)
        plain_d, plain_q = leg(t[:, :, T0], q[:, :, T0], t[:, :, T1], q[:, :, T1])
        d1, dq1 = leg(t[:, :, T0], q[:, :, T0], t[:, :, NEAR], q[:, :, NEAR])
        d2, dq2 = leg(t[:, :, FAR], q[:, :, FAR], t[:, :, T1], q[:, :, T1])
        seam_d, seam_q = d1 + rotate(d2, dq1), q_mul(dq1, dq2)
        fold = pl["folded"][..., None]
        side_d = np.where(pl["reads"][..., None], np.where(fold, seam_d, plain_d), F(0)).astype(F)
        side_q = np.where(pl["reads"][..., None], np.where(fold, seam_q, plain_q), IDENTITY).astype(F)
        pose = np.concatenate([side_d, np.zeros((n, 2, 1), F), side_q], 2)                       # [N, 2, 8]: a pair as a pose
        mixed = mb.blend_poses(pose[:, :1], pose[:, 1:], state["weights"])[:, 0]                # blend_side / blend_pose
        bit = (axes[:, None] & np.array([rm.ROOT_X, rm.ROOT_Y, rm.ROOT_Z], np.uint32)[None, :]) != 0
        d = np.where(bit, mixed[:, :3], F(0)).astype(F)
        dq = mixed[:, 4:]
        h = p[:, 4:]
        moved = (p[:, :3] + rotate(d, h)).astype(F)
        turned = q_mul(h, dq)
        turned = np.where(normalize[:, None], q_normalize(turned), turned).astype(F)
    out = p.copy()
    ok = ~np.isnan(dt)
    out[ok, :3] = moved[ok]
    out[ok, 4:] = turned[ok]
    fading = state["fade_rate"] > F(0)
    forwards = (pl["times"][:, :, NEAR] > 0) & pl["folded"]
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)          # noqa: E731
    ev = dict(fold_forwards_a=forwards[:, 0], fold_forwards_b=forwards[:, 1], fold_backwards_a=(pl["folded"] & ~forwards)[:, 0],
              fold_backwards_b=(pl["folded"] & ~forwards)[:, 1], fold_while_fading=pl["folded"].any(1) & fading & (pl["side"] == 2),
              mix=pl["side"] == 2, row_a=pl["side"] == 0, row_b=pl["side"] == 1, b_not_fading=(pl["side"] != 0) & ~fading,
              moved=(bits(out[:, :3]) != bits(p[:, :3])).any(1), turned=(bits(out[:, 4:]) != bits(p[:, 4:])).any(1))
    return out, ev


# ---- the same step as float64 matrices ------------------------------------------------------------------------------------------
def world(t, q):
    """W of a "world bone": ToRotateMatrix of q {x, y, z, w} with row 4 = {t, 1}, row-vector convention, float64."""
    i, j, k, e = (float(x) for x in q)
    m = np.eye(4)
    m[0, :3] = 1 - 2 * (j * j + k * k), 2 * (i * j + k * e), 2 * (i * k - j * e)
    m[1, :3] = 2 * (i * j - k * e), 1 - 2 * (k * k + i * i), 2 * (j * k + i * e)
    m[2, :3] = 2 * (i * k + j * e), 2 * (j * k - i * e), 1 - 2 * (i * i + j * j)
    m[3, :3] = [float(x) for x in t]
    return m


def chain(w_p, t, q, folded):
    """One step of one side in float64: W_p' = W_root(t1) * W_root(t0)^-1 * W_p, or, across a seam, the two legs the fold gives:
    W_root(t1) * W_root(far)^-1 * W_root(near) * W_root(t0)^-1 * W_p.  t [4, 3], q [4, 4] at t0, t1, near, far."""
    w = [world(t[k], q[k]) for k in range(4)]
    if not folded:
        return w[T1] @ np.linalg.inv(w[T0]) @ w_p
    return w[T1] @ np.linalg.inv(w[FAR]) @ w[NEAR] @ np.linalg.inv(w[T0]) @ w_p


def walk(clip, t_start, dt, steps, place, tq_of, normalize=False, axes=7):
    """`steps` steps of the restatement for one instance that plays `clip` from t_start at speed 1 -> (the placement after every
    step f32 [steps, 8], the float64 chain's matrix after every step [steps, 4, 4], the number of folds).  tq_of(times f64 [1, 2,
    4], plan) gives (T, Q) at them."""
    tab = table()
    state = ar.initial_state(1)
    state["clips_a"][:] = clip
    place = np.array(place, F).reshape(1, 8)
    w_p = world(place[0, :3], place[0, 4:])
    t_now, folds, out, mats = float(t_start), 0, [], []
    for _ in range(steps):
        state["times_a"][:] = t_now
        pl = rm.plan(state, tab, dt)
        t, q = tq_of(pl["times"], pl)
        place, _ = apply(state, tab, dt, t, q, axes, normalize, place)
        w_p = chain(w_p, np.asarray(t, np.float64)[0, 0], np.asarray(q, np.float64)[0, 0], bool(pl["folded"][0, 0]))
        folds += int(pl["folded"][0, 0])
        t_now = float(pl["times"][0, 0, T1])
        out.append(place[0].copy())
        mats.append(w_p.copy())
    return np.array(out), np.array(mats), folds


# ---- the stand-alone programs ---------------------------------------------------------------------------------------------------
ROW_ARRAYS = rm.ROW_ARRAYS + (("flags", np.uint32),)


def build_math_driver(sanitize=False):
    return hp.build("root_turn_math_driver", [os.path.join(HERE, "root_turn_math_driver.cpp")], sanitize=sanitize)


def build_libmmd_driver():
    return hp.build("root_turn_driver", [os.path.join(HERE, "root_turn_driver.cpp")], strict=False, include=[hp.REF_INC])


def _run(exe, args, tab, rows, extra, with_tq_out):
    n = rows["dt"].size

    def read(f):
        out = dict(times=np.fromfile(f, np.float64, n * 8).reshape(n, 2, 4), folded=np.fromfile(f, np.uint32, n * 2).reshape(n, 2) != 0)
        if with_tq_out:
            out["t"] = np.fromfile(f, F, n * 24).reshape(n, 2, 4, 3)
            out["q"] = np.fromfile(f, F, n * 32).reshape(n, 2, 4, 4)
        out["expect"] = np.fromfile(f, F, n * 8).reshape(n, 8)
        return out
    return hp.run_files(exe, lambda f: rm.write_rows(f, [n, tab["length"].size], tab, rows, ROW_ARRAYS, extra), read, args)


def run_math_driver(exe, tab, rows, t, q):
    """csrc/root_math.hpp on the host over `rows` (dict of ROW_ARRAYS) with (T, Q) = t f32 [N, 2, 4, 3], q f32 [N, 2, 4, 4]."""
    return _run(exe, (), tab, rows, (t, q), False)


def run_libmmd_driver(tab, rows):
    """The real libmmd over `rows` -> times, folded, t, q (libmmd's (T, Q) at the sampled instants) and expect."""
    return _run(build_libmmd_driver(), rm.libmmd_driver_args(clip_paths()), tab, rows, (), True)


rows_as_state = rm.rows_as_state


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def fixture():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


def check_coverage(z):
    """The golden rows go through every case the issue names, counted."""
    tab = table()
    pl = rm.plan(rows_as_state(z), tab, z["dt"])
    normalize = (z["flags"] & ROOT_NORMALIZE) != 0
    _, ev = apply(rows_as_state(z), tab, z["dt"], z["t"], z["q"], z["axes"], normalize, z["placements"])
    n = {k: int(v.sum()) for k, v in ev.items()}
    for k in ("fold_forwards_a", "fold_forwards_b", "fold_backwards_a", "fold_backwards_b"):
        assert n[k] >= 8, n                                                   # forward and backward folds on either side
    assert n["fold_while_fading"] >= 4 and n["row_a"] >= 20 and n["row_b"] >= 20 and n["mix"] >= 20, n
    for c in ("clips_a", "clips_b"):                                          # a clip id outside the bank on either side, read
        read = pl["reads"][:, 0 if c == "clips_a" else 1]
        assert ((z[c] == NONE) & read).sum() >= 4 and ((z[c] >= N_CLIPS) & (z[c] != NONE) & read).sum() >= 4, c
    fading = z["fade_rate"] > 0
    assert (~fading).sum() >= 40 and n["b_not_fading"] >= 8, n               # fade_rate 0
    played = set(z["clips_a"][pl["reads"][:, 0]].tolist()) | set(z["clips_b"][pl["reads"][:, 1]].tolist())
    assert set(range(N_CLIPS)) <= played                                      # the track-less clip 2 and root_q8 among them
    assert (normalize & ev["turned"]).sum() >= 40 and (~normalize & ev["turned"]).sum() >= 40
    for a in range(8):                                                        # every axes subset, with and without the flag
        assert (normalize & (z["axes"] == a)).sum() >= 2 and (~normalize & (z["axes"] == a)).sum() >= 2, a
    assert set(np.unique(z["flags"]).tolist()) == {0, ROOT_NORMALIZE}
    h = z["placements"][:, 4:]
    norm = np.sqrt((h.astype(np.float64) ** 2).sum(1))
    ident = (h == IDENTITY).all(1)
    assert ident.sum() >= 8 and (np.abs(norm - 1) > 0.1).sum() >= 8 and ((np.abs(norm - 1) < 1e-6) & ~ident).sum() >= 8
    assert (z["placements"][:, 3] != 0).sum() >= z["dt"].size // 2            # a nonzero fourth float
    assert set(z["speed"].tolist()) >= {1.0, 0.5, -1.0, 0.0}                  # negative and zero speed
    assert (z["dt"] == 0).sum() >= 4 and np.isnan(z["dt"]).sum() >= 2
    assert not np.isnan(z["placements"]).any() and n["moved"] >= z["dt"].size // 3 and n["turned"] >= z["dt"].size // 3
    return n
