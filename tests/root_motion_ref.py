"""Root motion (mmdx_animator_root_motion, include/mmdx.h): what the tests and the fixture generator share.

  * plan() / apply(): a restatement of the call in numpy, written from the header's text -- whole arrays at a time, masks instead of
    branches, every numpy operation one IEEE rounding.  plan() gives the instants at which the root bone is sampled (the clocks
    are tests/animator_ref.py's wrap), apply() takes R, the root's translation at those instants, from its caller: the golden rows
    carry libmmd's, a GPU test takes it from the pinned MotionSet.eval_bones_time;
  * the clips of the fixture (tests/golden/root_*.vmd, written by vmd.write_vmd) and their clip table;
  * the two stand-alone programs: tests/root_motion_driver.cpp (the REAL libmmd; built where the reference's headers are) and
    tests/root_math_driver.cpp (csrc/root_math.hpp for the host, plain and under the sanitizers), both built and run by
    tests/host_program.py;
  * the fixture tests/golden/root_motion_expect.npz (tests/gen_root_motion_golden.py).
Nothing compiled here is committed.
"""
import os

import numpy as np

from tests import animator_ref as ar
from tests import golden_util as gu
from tests import host_program as hp
from tests import motion_blend_ref as mb
from tests import palette_place_ref as pp

F = np.float32
HERE = hp.TESTS
FIXTURE = os.path.join(gu.GOLDEN_DIR, "root_motion_expect.npz")
NONE = ar.NONE
ROOT_X, ROOT_Y, ROOT_Z = 1, 2, 4                     # MMDX_ROOT_*
ROOT_NAME = "全ての親"                                # the parentless root the clips move; not a bone of rig_small
T0, T1, NEAR, FAR = 0, 1, 2, 3

# ---- the clips ------------------------------------------------------------------------------------------------------------------
# four files, six clips: the curved and the linear walk are bound twice, so that they also play under HOLD and THEN
VMDS = {name: os.path.join(gu.GOLDEN_DIR, "root_%s.vmd" % name) for name in ("curved", "linear", "no_root", "still")}
CLIP_FILES = ("curved", "linear", "no_root", "still", "curved", "linear")
CLIP_FRAMES = (45, 30, 20, 0, 45, 30)                # the last key frame of each clip
# lengths are stated (frames / 30.0), so that a one-bone bank of the root alone -- where clip 2 has no key -- gives the same table;
# clip 3 keeps 0.0 = its own length, which is 0 in any binding
CLIP_ROWS = ((45 / 30.0, ar.LOOP, NONE, 0.0), (30 / 30.0, ar.LOOP, NONE, 0.0), (20 / 30.0, ar.LOOP, NONE, 0.0), (0.0, ar.LOOP, NONE, 0.0),
             (45 / 30.0, ar.HOLD, NONE, 0.0), (30 / 30.0, ar.THEN, 0, 0.25))
N_CLIPS = len(CLIP_FILES)


def rig_small_names():
    z = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    return [str(n) for n in z["model_bone_names"]]


def clip_paths():
    return [VMDS[n] for n in CLIP_FILES]


def table():
    return ar.table_of(ar.resolved_rows(CLIP_ROWS, CLIP_FRAMES))


def root_bank():
    """The intended cheap form: every clip bound to the root's name alone -- a one-bone bank, root_bone = 0."""
    from simple_mmd_renderer_amd import vmd
    vs = [vmd.Vmd(p) for p in clip_paths()]
    bms = [v.bind_bones([ROOT_NAME]) for v in vs]
    ms = vmd.MotionSet(bms)
    for x in bms + vs:
        x.close()
    return ms


def write_clips():
    """The four .vmd files (tests/gen_root_motion_golden.py writes them; they are committed).  Every clip also moves a few bones of
    rig_small, so that an in-place copy has something to leave alone."""
    from simple_mmd_renderer_amd import synth, vmd
    names = rig_small_names()
    ease = bytes([10, 90, 40, 100, 30, 20, 60, 70, 100, 20, 120, 127, 110, 100, 80, 60] * 4)      # four curves that are not linear
    ident = (0.0, 0.0, 0.0, 1.0)
    rng = np.random.RandomState(4711)

    def turn():
        q = rng.normal(size=4)
        return tuple(float(x) for x in (q / np.linalg.norm(q)).astype(F))
    body = {n: synth.make_bone_keys(names[1 + k:4 + k], 300 + k, keys_per=3, span=last) + [(names[1 + k], last, (0.5, -0.25, 0.125), turn(), None)]
            for k, (n, last) in enumerate((("curved", 45), ("linear", 30), ("no_root", 20)))}
    curved = [(ROOT_NAME, 0, (0.25, 0.0, -0.5), turn(), ease), (ROOT_NAME, 12, (1.5, 0.375, 2.0), turn(), ease),
              (ROOT_NAME, 31, (0.75, -0.25, 5.5), turn(), ease), (ROOT_NAME, 45, (3.0, 0.5, 9.25), turn(), None)]
    linear = [(ROOT_NAME, 0, (0.0, 0.0, 0.0), ident, None), (ROOT_NAME, 30, (0.0, 0.0, 7.5), ident, None)]
    still = [(ROOT_NAME, 0, (1.0, 2.0, 3.0), turn(), None), (names[2], 0, (0.5, 0.0, 0.0), turn(), None)]
    files = {"curved": curved + body["curved"], "linear": linear + body["linear"], "no_root": body["no_root"], "still": still}
    for n, keys in files.items():
        with open(VMDS[n], "wb") as f:
            f.write(vmd.write_vmd(keys, []))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _side_times(tab, clips, t0, s):
    """Step 2's clocks for whole arrays -> (instants f64 [N, 4]: t0, t1, near, far; folded bool [N])."""
    nc = tab["length"].size
    raw = t0 + s
    t1, fold = ar.wrap(tab, clips, raw)
    length = tab["length"][np.where(clips < nc, clips, 0)]
    forwards = raw >= length
    near = np.where(fold & forwards, length, 0.0)
    far = np.where(fold & ~forwards, length, 0.0)
    return np.stack([t0, t1, near, far], 1), fold


def plan(state, tab, dt):
    """Where R is needed.  state: the animator's arrays (dict) before the step; dt: a scalar or f64 [N] -> dict(
    clips u32 [N, 2], times f64 [N, 2, 4] (0 where not sampled), folded bool [N, 2], reads bool [N, 2] (the side is read at all),
    sampled bool [N, 2, 4] (R is taken at this instant; an id outside the bank still counts: its R is 0), side u32 [N])."""
    n = state["clips_a"].size
    dt = np.broadcast_to(np.asarray(dt, np.float64), (n,))
    with np.errstate(all="ignore"):
        s = state["speed"].astype(np.float64) * dt
        side = mb.side_of(state["weights"])
        reads = np.stack([side != 1, (side != 0) & (state["fade_rate"] > F(0))], 1) & ~np.isnan(dt)[:, None]
        times, folded = np.zeros((n, 2, 4)), np.zeros((n, 2), bool)
        for k, (c, t) in enumerate((("clips_a", "times_a"), ("clips_b", "times_b"))):
            safe_t = np.where(reads[:, k], state[t], 0.0)                     # a side that is not read may hold anything
            safe_c = np.where(reads[:, k], state[c], NONE).astype(np.uint32)
            tk, fk = _side_times(tab, safe_c, safe_t, s)
            times[:, k], folded[:, k] = tk, fk
    folded &= reads
    sampled = np.zeros((n, 2, 4), bool)
    sampled[:, :, :2] = reads[:, :, None]
    sampled[:, :, 2:] = folded[:, :, None]
    times = np.where(sampled, times, 0.0)
    clips = np.stack([state["clips_a"], state["clips_b"]], 1).astype(np.uint32)
    return dict(clips=clips, times=times, folded=folded, reads=reads, sampled=sampled, side=side)


def apply(state, tab, dt, r, axes, placements):
    """The call.  r f32 [N, 2, 4, 3]: R at the instants of plan() (ignored where not sampled); axes: a scalar or u32 [N];
    placements f32 [N, 8] -> (the placements after the call, events: name -> bool [N])."""
    pl = plan(state, tab, dt)
    n = state["clips_a"].size
    dt = np.broadcast_to(np.asarray(dt, np.float64), (n,))
    axes = np.broadcast_to(np.asarray(axes, np.uint32), (n,))
    p = np.array(placements, F).reshape(n, 8)
    w = state["weights"].astype(F)[:, None]
    with np.errstate(all="ignore"):
        r = np.where(pl["sampled"][..., None], np.asarray(r, F), F(0))
        plain = r[:, :, T1] - r[:, :, T0]
        seam = (r[:, :, NEAR] - r[:, :, T0]) + (r[:, :, T1] - r[:, :, FAR])
        d_side = np.where(pl["folded"][..., None], seam, plain).astype(F)
        d_side = np.where(pl["reads"][..., None], d_side, F(0))
        da, db = d_side[:, 0], d_side[:, 1]
        mix = da * (F(1) - w) + db * w
        side = pl["side"][:, None]
        d = np.where(side == 0, da, np.where(side == 1, db, mix)).astype(F)
        bit = (axes[:, None] & np.array([ROOT_X, ROOT_Y, ROOT_Z], np.uint32)[None, :]) != 0
        d = np.where(bit, d, F(0)).astype(F)
        m = pp.matrix_from_pose(p)                                            # ToRotateMatrix of p[4..7], not normalised
        turned = np.stack([d[:, 0] * m[:, c] + d[:, 1] * m[:, 4 + c] + d[:, 2] * m[:, 8 + c] for c in range(3)], 1)
        moved = (p[:, :3] + turned).astype(F)
    out = p.copy()
    ok = ~np.isnan(dt)
    out[ok, :3] = moved[ok]
    fading = state["fade_rate"] > F(0)
    forwards = (pl["times"][:, :, NEAR] > 0) & pl["folded"]
    ev = dict(fold_forwards=forwards.any(1), fold_backwards=(pl["folded"] & ~forwards).any(1),
              fold_while_fading=pl["folded"].any(1) & fading & (pl["side"] == 2), mix=pl["side"] == 2, row_a=pl["side"] == 0,
              row_b=pl["side"] == 1, b_not_fading=(pl["side"] != 0) & ~fading, moved=(out[:, :3] != p[:, :3]).any(1))
    return out, ev


# ---- the stand-alone programs ---------------------------------------------------------------------------------------------------
ROW_ARRAYS = (("clips_a", np.uint32), ("clips_b", np.uint32), ("times_a", np.float64), ("times_b", np.float64), ("weights", F),
              ("speed", F), ("fade_rate", F), ("dt", np.float64), ("axes", np.uint32), ("placements", F))


def build_math_driver(sanitize=False):
    return hp.build("root_math_driver", [os.path.join(HERE, "root_math_driver.cpp")], sanitize=sanitize)


def build_libmmd_driver():
    return hp.build("root_motion_driver", [os.path.join(HERE, "root_motion_driver.cpp")], strict=False, include=[hp.REF_INC])


def libmmd_driver_args(paths):
    """What both libmmd drivers take behind their two files: the root's name in Shift-JIS and the clips' paths."""
    return [ROOT_NAME.encode("shift_jis")] + [p.encode() for p in paths]


def write_rows(f, head, tab, rows, row_arrays=ROW_ARRAYS, extra=()):
    """A driver's input: the head words, the clip table, the row arrays and any float arrays behind them."""
    np.array(head, np.uint32).tofile(f)
    for k in ("length", "mode", "next", "fade"):
        tab[k].tofile(f)
    for k, t in row_arrays:
        np.ascontiguousarray(rows[k], t).tofile(f)
    for a in extra:
        np.ascontiguousarray(a, F).tofile(f)


def _run(exe, args, head, tab, rows, extra, with_r_out):
    n = rows["dt"].size

    def read(f):
        out = dict(times=np.fromfile(f, np.float64, n * 8).reshape(n, 2, 4), folded=np.fromfile(f, np.uint32, n * 2).reshape(n, 2) != 0)
        if with_r_out:
            out["r"] = np.fromfile(f, F, n * 24).reshape(n, 2, 4, 3)
        out["expect"] = np.fromfile(f, F, n * 3).reshape(n, 3)
        return out
    return hp.run_files(exe, lambda f: write_rows(f, head, tab, rows, extra=extra), read, args)


def run_math_driver(exe, tab, rows, r=None):
    """csrc/root_math.hpp on the host over `rows` (dict of ROW_ARRAYS) with R = r f32 [N, 2, 4, 3] (None: the instants only)."""
    return _run(exe, (), [rows["dt"].size, tab["length"].size, 0 if r is None else 1], tab, rows, () if r is None else (r,), False)


def run_libmmd_driver(tab, rows):
    """The real libmmd over `rows` -> times, folded, r (libmmd's R at the sampled instants) and expect."""
    return _run(build_libmmd_driver(), libmmd_driver_args(clip_paths()), [rows["dt"].size, tab["length"].size], tab, rows, (), True)


def rows_as_state(rows):
    """The seven arrays of a row set that are animator state."""
    return {k: rows[k] for k in ("clips_a", "clips_b", "times_a", "times_b", "weights", "speed", "fade_rate")}


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def fixture():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


def check_coverage(z):
    """The golden rows go through every case the issue names, counted."""
    tab = table()
    pl = plan(rows_as_state(z), tab, z["dt"])
    _, ev = apply(rows_as_state(z), tab, z["dt"], z["r"], z["axes"], z["placements"])
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)          # noqa: E731
    fading = z["fade_rate"] > 0
    for weight in mb.WEIGHTS:
        same = bits(z["weights"]) == bits(F(weight))
        assert (same & fading).sum() >= 2 and (same & ~fading).sum() >= 2, weight
    assert set(z["speed"].tolist()) >= {1.0, 0.5, -1.0, 0.0}
    assert ev["fold_forwards"].sum() >= 8 and ev["fold_backwards"].sum() >= 8 and ev["fold_while_fading"].sum() >= 4, {k: int(v.sum()) for k, v in ev.items()}
    length = tab["length"][np.where(z["clips_a"] < N_CLIPS, z["clips_a"], 0)]
    with np.errstate(all="ignore"):
        step = np.abs(z["speed"].astype(np.float64) * z["dt"])
    assert ((step > 2 * length) & pl["folded"][:, 0]).sum() >= 4                                   # several laps in one step
    hold = (z["clips_a"] == 4) & pl["reads"][:, 0]
    assert (hold & (pl["times"][:, 0, T1] == tab["length"][4]) & (z["times_a"] < tab["length"][4])).sum() >= 2        # clamps on HOLD
    assert (z["dt"] == 0).sum() >= 4 and np.isnan(z["dt"]).sum() >= 2
    for c in ("clips_a", "clips_b"):
        assert (z[c] == NONE).sum() >= 4 and ((z[c] >= N_CLIPS) & (z[c] != NONE)).sum() >= 4, c
    played = set(z["clips_a"][pl["reads"][:, 0]].tolist()) | set(z["clips_b"][pl["reads"][:, 1]].tolist())
    assert set(range(N_CLIPS)) <= played
    assert set(z["axes"].tolist()) == set(range(8))
    q = z["placements"][:, 4:]
    norm = np.sqrt((q.astype(np.float64) ** 2).sum(1))
    ident = (q == np.array([0, 0, 0, 1], F)).all(1)
    assert ident.sum() >= 8 and (np.abs(norm - 1) > 0.1).sum() >= 8 and ((np.abs(norm - 1) < 1e-6) & ~ident).sum() >= 8
    assert not np.isnan(z["placements"]).any()
    assert ev["b_not_fading"].sum() >= 8 and ev["moved"].sum() >= z["dt"].size // 3
    return {k: int(v.sum()) for k, v in ev.items()}
