"""mmdx_palette_place (include/mmdx.h: out[i][b] = S[i][b] * W[i]): the checkers the tests and the fixture generator share.

  * a numpy float32 restatement (matrix_from_pose / place): one rounding per operation, every sum left to right;
  * the REAL libmmd through tests/palette_place_driver.cpp -- compiled with g++ where the reference's headers are present (they are
    not on the GPU machines);
  * the project's own arithmetic header on the CPU through tests/place_math_driver.cpp;
  * the fixture tests/golden/palette_place_expect.npz (tests/gen_palette_place_golden.py).
Rows are compared bit for bit, except that a NaN only has to be a NaN (golden_util.assert_bits_equal_or_both_nan): sign and
payload of a NaN are not part of the contract.  Nothing compiled here is committed.
"""
import os

import numpy as np

from tests import golden_util as gu
from tests import host_program as hp

FIXTURE = os.path.join(gu.GOLDEN_DIR, "palette_place_expect.npz")
ROOT = hp.ROOT
F = np.float32
ONE, TWO = F(1.0), F(2.0)
POSE, MATRIX = 0, 1                      # the `form` of a fixture row
IDENTITY_POSE = np.array([0, 0, 0, 0, 0, 0, 0, 1], F)


# ---- the restatement ------------------------------------------------------------------------------
def matrix_from_pose(poses):
    """poses f32 [..., 8] = {tx, ty, tz, ignored, qx, qy, qz, qw} -> W f32 [..., 16]: Quaternion::ToRotateMatrix
    (L/util/math_impl.inl:540-563, not normalised), row 4 = {tx, ty, tz, 1}."""
    p = np.asarray(poses, F)
    i, j, k, e = p[..., 4], p[..., 5], p[..., 6], p[..., 7]
    w = np.zeros(p.shape[:-1] + (16,), F)
    with np.errstate(all="ignore"):
        ii, jj, kk, ij, jk, ki, ie, je, ke = i * i, j * j, k * k, i * j, j * k, i * k, i * e, j * e, k * e
        w[..., 0] = ONE - TWO * (jj + kk); w[..., 1] = TWO * (ij + ke); w[..., 2] = TWO * (ki - je)
        w[..., 4] = TWO * (ij - ke); w[..., 5] = ONE - TWO * (kk + ii); w[..., 6] = TWO * (jk + ie)
        w[..., 8] = TWO * (ki + je); w[..., 9] = TWO * (jk - ie); w[..., 10] = ONE - TWO * (ii + jj)
    w[..., 12:15] = p[..., 0:3]
    w[..., 15] = ONE
    return w


def place(s, w):
    """s f32 [..., 16], w f32 [..., 16] (broadcast against each other) -> s * w, Matrix4x4::operator*
    (L/util/math_impl.inl:984-1003): every element the left-to-right sum of four products."""
    s, w = np.asarray(s, F), np.asarray(w, F)
    out = np.zeros(np.broadcast_shapes(s.shape, w.shape), F)
    with np.errstate(all="ignore"):
        for r in range(4):
            a1, a2, a3, a4 = (s[..., 4 * r + k] for k in range(4))
            for c in range(4):
                out[..., 4 * r + c] = a1 * w[..., c] + a2 * w[..., 4 + c] + a3 * w[..., 8 + c] + a4 * w[..., 12 + c]
    return out


def world_matrices(placements, matrix):
    """placements f32 [N, 8] (pose form) or [N, 16] (matrix form) -> W f32 [N, 16]."""
    return np.asarray(placements, F).reshape(-1, 16).copy() if matrix else matrix_from_pose(np.asarray(placements, F).reshape(-1, 8))


def place_crowd(palettes, placements, matrix):
    """palettes f32 [NI, NB, 16], one placement per instance -> the placed palettes [NI, NB, 16]."""
    return place(np.asarray(palettes, F), world_matrices(placements, matrix)[:, None, :])


def place_rows(forms, s, placements):
    """Fixture rows: forms u8 [N], s f32 [N, 16], placements f32 [N, 16] (a pose row uses the first 8) -> [N, 16]."""
    forms = np.asarray(forms)
    w = np.where((forms == POSE)[:, None], matrix_from_pose(placements[:, :8]), placements)
    return place(s, w)


assert_rows_equal = gu.assert_bits_equal_or_both_nan


# ---- the two drivers ------------------------------------------------------------------------------
def build_libmmd_driver() -> str:
    return hp.build("palette_place_driver", [os.path.join(hp.TESTS, "palette_place_driver.cpp")], strict=False, include=[hp.REF_INC])


def build_math_driver(sanitize: bool = False) -> str:
    return hp.build("place_math_driver", [os.path.join(hp.TESTS, "place_math_driver.cpp")], sanitize=sanitize)


def run_driver(exe, forms, s, placements):
    """The rows through one of the drivers (text in, text out, floats as hex bit patterns) -> f32 [N, 16]."""
    forms = np.asarray(forms)
    words = np.concatenate([gu.bits(s).reshape(-1, 16), gu.bits(placements).reshape(-1, 16)], axis=1)
    stdin = "".join("%d %s\n" % (f, hp.hex_words(row)) for f, row in zip(forms, words))
    out = hp.parse_hex_rows(hp.run(exe, stdin=stdin).stdout, 16)
    assert out.shape == (forms.size, 16), out.shape
    return out.view(F)


# ---- the fixture ----------------------------------------------------------------------------------
def fixture():
    """dict: form u8 [N] (0 pose, 1 matrix), kind [N] (what the row is there for), s f32 [N, 16], placement f32 [N, 16] (a pose row
    holds its 8 floats first, zeros behind), expect f32 [N, 16] (the real libmmd's S * W)."""
    z = np.load(FIXTURE)
    out = {k: z[k] for k in z.files}
    out["kind"] = [str(k) for k in z["kind"]]
    return out
