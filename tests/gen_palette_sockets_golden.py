"""Generate tests/golden/palette_sockets_expect.npz: mmdx_palette_sockets (include/mmdx.h, out = (O *) G * S) as the real libmmd
computes it (tests/palette_sockets_driver.cpp: MakeIdentity + the row-4 assignment of global_offset_matrix_inv_,
Quaternionf::ToRotateMatrix + the row-4 assignment of local_matrix_, Matrix4f::operator*).

Skinning matrices S are real palettes of the rig_small fixture (tests/golden/rig_small_expect.npz), and the rest position p of a
row is that of the bone its S belongs to, unless the row says otherwise.  Rows, by `kind`:
  no offset    bone        S of a bone with that bone's rest position: G * S is the bone's local_matrix_
               rest        rest positions 0, -0, a denormal and 1e4 per axis
  pose form    unit        unit quaternions over both hemispheres (qw > 0 and qw < 0), translations from 1e-3 to 1e4, the ignored
                           fourth float set to something else than 0 on every other row
               nonunit     quaternions of length 0.25 .. 3 (libmmd does not normalise), and the zero quaternion
  matrix form  rigid       rotation + translation
               scaled      rigid with per-axis scales 0.1 .. 10 (one of them negative on some rows)
               sheared     scaled with off-diagonal shear, a few with a fourth column other than (0, 0, 0, 1)
  every form   negzero     one -0 element planted in S, in p or in the offset, at a position that walks through the row
               denormal    the same with denormals
               inf         the same with +-infinity
               nan         the same with a NaN
Needs the reference's headers:
    python -m tests.gen_palette_sockets_golden
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import golden_util as gu  # noqa: E402
from tests import gen_palette_place_golden as gp  # noqa: E402
from tests import palette_sockets_ref as ps  # noqa: E402

F = np.float32


def rows():
    rng = np.random.RandomState(2031)
    z = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    pal = z["expect_palettes"].reshape(-1, 16)
    nb = z["rest"].shape[0]
    order = rng.permutation(pal.shape[0])
    taken = [0]

    def real(n):
        """n real skinning matrices and the rest positions of their bones."""
        taken[0] += n
        idx = order[taken[0] - n:taken[0]]
        return pal[idx].copy(), z["rest"][idx % nb].astype(F).copy()
    form, kind, s, p, o = [], [], [], [], []

    def add(f, k, ss, pp_, off=None):
        n = len(ss)
        off = np.zeros((n, 16), F) if off is None else np.asarray(off, F)
        if off.shape[1] == 8:
            off = np.concatenate([off, np.zeros((n, 8), F)], axis=1)
        form.extend([f] * n); kind.extend([k] * n); s.append(np.asarray(ss, F)); p.append(np.asarray(pp_, F)); o.append(off)

    def poses(t, q, fourth=0.0):
        out = np.zeros((len(q), 8), F)
        out[:, :3], out[:, 4:] = t, q
        out[1::2, 3] = fourth
        return out

    # no offset
    add(ps.NONE, "bone", *real(64))
    ss, pr = real(16)
    special = np.array([0.0, -0.0, 1e-40, 1e4], F)
    for r in range(16):
        pr[r, r % 3] = special[(r // 3) % 4]
        if r >= 12:
            pr[r] = special[r - 12]
    add(ps.NONE, "rest", ss, pr)
    # pose-form offsets
    add(ps.POSE, "unit", *real(48), poses(gp.translations(rng, 48), gp.unit_quaternions(rng, 48), fourth=7.5))
    q = gp.unit_quaternions(rng, 16) * rng.uniform(0.25, 3.0, size=(16, 1)).astype(F)
    q[0] = 0.0
    add(ps.POSE, "nonunit", *real(16), poses(gp.translations(rng, 16), q, fourth=-3.0))
    # matrix-form offsets
    add(ps.MATRIX, "rigid", *real(24), gp.matrices(rng, 24))
    add(ps.MATRIX, "scaled", *real(24), gp.matrices(rng, 24, scaled=True))
    add(ps.MATRIX, "sheared", *real(24), gp.matrices(rng, 24, sheared=True))
    # the special classes, in every form: one planted element per row, in S, in p or in the offset, walking through the positions
    for f in (ps.NONE, ps.POSE, ps.MATRIX):
        live = [0, 1, 2, 4, 5, 6, 7] if f == ps.POSE else list(range(16))      # a pose's fourth float is ignored
        where = 2 if f == ps.NONE else 3

        def plant(kind_name, values, n=9):
            ss, pr = real(n)
            off = None if f == ps.NONE else (poses(gp.translations(rng, n), gp.unit_quaternions(rng, n)) if f == ps.POSE
                                             else gp.matrices(rng, n))
            for r in range(n):
                v = values[r % len(values)]
                if r % where == 0:
                    ss[r, (5 * r + 3) % 16] = v
                elif r % where == 1:
                    pr[r, (r // where) % 3] = v
                else:
                    off[r, live[(3 * r) % len(live)]] = v
            add(f, kind_name, ss, pr, off)
        plant("negzero", [F(-0.0)])
        plant("denormal", [F(1e-40), F(-3e-42), F(1.1754942e-38)])
        plant("inf", [F(np.inf), F(-np.inf)])
        plant("nan", [F(np.nan)])
    return np.array(form, np.uint8), np.array(kind), np.concatenate(s), np.concatenate(p), np.concatenate(o)


def main():
    form, kind, s, p, o = rows()
    expect = ps.run_driver(ps.build_libmmd_driver(), form, s, p, o)
    np.savez_compressed(ps.FIXTURE, form=form, kind=kind, s=s, rest=p, offset=o, expect=expect)
    print("%s: %d rows (%d none, %d pose, %d matrix), %.1f KB" % (os.path.basename(ps.FIXTURE), form.size, (form == 0).sum(),
                                                                   (form == 1).sum(), (form == 2).sum(), os.path.getsize(ps.FIXTURE) / 1024))
    for k in sorted(set(kind)):
        print("  %-9s %3d" % (k, (kind == k).sum()))


if __name__ == "__main__":
    main()
