"""Generate tests/golden/palette_place_expect.npz: mmdx_palette_place (include/mmdx.h, out = S * W) as the real libmmd computes it
(tests/palette_place_driver.cpp: Quaternionf::ToRotateMatrix, the row-4 assignment, Matrix4f::operator*).

Skinning matrices S are real palettes of the rig_small fixture (tests/golden/rig_small_expect.npz).  Rows, by `kind`:
  pose form    unit        unit quaternions over both hemispheres (qw > 0 and qw < 0), translations from 1e-3 to 1e4, the ignored
                           fourth float set to something else than 0 on every other row
               identity    the identity placement, on real palettes and on matrices with -0 elements (a -0 becomes +0)
               nonunit     quaternions of length 0.25 .. 3 (libmmd does not normalise), and the zero quaternion
  matrix form  rigid       rotation + translation
               scaled      rigid with per-axis scales 0.1 .. 10 (one of them negative on some rows)
               sheared     scaled with off-diagonal shear, a few with a fourth column other than (0, 0, 0, 1)
               identity    the identity matrix on matrices with -0 elements
  both forms   negzero     -0 elements in S and in the placement
               denormal    denormal elements in S and in the placement, and products that underflow into the denormals
               inf         one infinite element in S, or in the placement
               nan         one NaN element in S, or in the placement
Needs the reference's headers:
    python -m tests.gen_palette_place_golden
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import golden_util as gu  # noqa: E402
from tests import palette_place_ref as pp  # noqa: E402

F = np.float32


def unit_quaternions(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[:, 3] = np.abs(q[:, 3]) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)        # both hemispheres, alternating
    return q.astype(F)


def translations(rng, n):
    mag = 10.0 ** rng.uniform(-3, 4, size=(n, 3))
    mag[0], mag[1] = 1e-3, 1e4
    return (mag * rng.choice([-1.0, 1.0], size=(n, 3))).astype(F)


def rotation(q):
    """float64 rotation matrices [n, 3, 3] (row-vector convention) of unit quaternions, rounded by the caller."""
    x, y, z, w = (q[:, k].astype(np.float64) for k in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w)], -1),
                     np.stack([2 * (x * y - z * w), 1 - 2 * (z * z + x * x), 2 * (y * z + x * w)], -1),
                     np.stack([2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def matrices(rng, n, scaled=False, sheared=False):
    m = np.zeros((n, 4, 4))
    lin = rotation(unit_quaternions(rng, n))
    if scaled or sheared:
        s = 10.0 ** rng.uniform(-1, 1, size=(n, 3))
        s[::3, 0] *= -1.0
        lin = s[:, :, None] * lin
    if sheared:
        sh = np.tile(np.eye(3), (n, 1, 1))
        sh[:, 0, 1], sh[:, 0, 2], sh[:, 1, 2] = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        lin = sh @ lin
    m[:, :3, :3] = lin
    m[:, 3, :3] = translations(rng, n)
    m[:, 3, 3] = 1.0
    if sheared:
        m[::4, :3, 3] = rng.uniform(-0.01, 0.01, size=(m[::4].shape[0], 3))       # a fourth column of its own
        m[::4, 3, 3] = 0.5
    return m.reshape(n, 16).astype(F)


def rows():
    rng = np.random.RandomState(2028)
    pal = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))["expect_palettes"].reshape(-1, 16)
    pal = pal[rng.permutation(pal.shape[0])]
    taken = [0]

    def real(n):
        taken[0] += n
        return pal[taken[0] - n:taken[0]].copy()
    form, kind, s, p = [], [], [], []

    def add(f, k, ss, pl):
        pl = np.asarray(pl, F)
        if pl.shape[1] == 8:
            pl = np.concatenate([pl, np.zeros((pl.shape[0], 8), F)], axis=1)
        form.extend([f] * len(ss)); kind.extend([k] * len(ss)); s.append(np.asarray(ss, F)); p.append(pl)

    def poses(t, q, fourth=0.0):
        n = len(q)
        out = np.zeros((n, 8), F)
        out[:, :3], out[:, 4:] = t, q
        out[1::2, 3] = fourth
        return out
    ident_m = np.eye(4, dtype=F).reshape(1, 16)
    negz = real(8)
    negz[np.abs(negz) < 1e-6] = F(-0.0)                       # the exact zeros of a skinning matrix (column 4), negative
    negz[:, 0] = F(-0.0)

    # pose form
    add(pp.POSE, "unit", real(64), poses(translations(rng, 64), unit_quaternions(rng, 64), fourth=7.5))
    add(pp.POSE, "identity", real(6), np.tile(pp.IDENTITY_POSE, (6, 1)))
    add(pp.POSE, "identity", negz, np.tile(pp.IDENTITY_POSE, (8, 1)))
    q = unit_quaternions(rng, 24) * rng.uniform(0.25, 3.0, size=(24, 1)).astype(F)
    q[0] = 0.0
    add(pp.POSE, "nonunit", real(24), poses(translations(rng, 24), q, fourth=-3.0))
    # matrix form
    add(pp.MATRIX, "rigid", real(40), matrices(rng, 40))
    add(pp.MATRIX, "scaled", real(32), matrices(rng, 32, scaled=True))
    add(pp.MATRIX, "sheared", real(32), matrices(rng, 32, sheared=True))
    add(pp.MATRIX, "identity", negz, np.tile(ident_m, (8, 1)))
    # the special classes, in both forms: one planted element per row, at a position that walks through the matrix
    for f in (pp.POSE, pp.MATRIX):
        def placement(n):
            return poses(translations(rng, n), unit_quaternions(rng, n)) if f == pp.POSE else matrices(rng, n)
        live = [0, 1, 2, 4, 5, 6, 7] if f == pp.POSE else list(range(16))      # a pose's fourth float is ignored

        def plant(kind_name, values, n=10):
            ss, pl = real(n), placement(n)
            for r in range(n):
                v = values[r % len(values)]
                if r % 2 == 0:
                    ss[r, (5 * r + 3) % 16] = v
                else:
                    pl[r, live[(3 * r) % len(live)]] = v
            add(f, kind_name, ss, pl)
        plant("negzero", [F(-0.0)])
        plant("denormal", [F(1e-40), F(-3e-42), F(1.1754942e-38)])
        # products that underflow: tiny S against a tiny placement
        ss, pl = real(4) * F(1e-22), placement(4)
        pl[:, :3 if f == pp.POSE else 16] *= F(1e-20)
        add(f, "denormal", ss, pl)
        plant("inf", [F(np.inf), F(-np.inf)])
        plant("nan", [F(np.nan)])
    return np.array(form, np.uint8), np.array(kind), np.concatenate(s), np.concatenate(p)


def main():
    form, kind, s, p = rows()
    expect = pp.run_driver(pp.build_libmmd_driver(), form, s, p)
    np.savez_compressed(pp.FIXTURE, form=form, kind=kind, s=s, placement=p, expect=expect)
    print("%s: %d rows (%d pose, %d matrix), %.1f KB" % (os.path.basename(pp.FIXTURE), form.size, (form == 0).sum(), (form == 1).sum(),
                                                         os.path.getsize(pp.FIXTURE) / 1024))
    for k in sorted(set(kind)):
        print("  %-9s %3d" % (k, (kind == k).sum()))


if __name__ == "__main__":
    main()
