"""mmdx_palette_sockets (include/mmdx.h: out[s][i] = (O[s] *) G[s] * S[i][bone[s]]): the checkers the tests and the fixture
generator share.

  * a numpy float32 restatement (bone_frame / sockets): one rounding per operation, every sum left to right, no short circuits;
  * the REAL libmmd through tests/palette_sockets_driver.cpp -- compiled with g++ where the reference's headers are present (they
    are not on the GPU machines);
  * the project's own arithmetic header and table builder on the CPU through tests/socket_math_driver.cpp;
  * the fixture tests/golden/palette_sockets_expect.npz (tests/gen_palette_sockets_golden.py).
Rows are compared bit for bit, except that a NaN only has to be a NaN (golden_util.assert_bits_equal_or_both_nan): sign and
payload of a NaN are not part of the contract.  Nothing compiled here is committed.
"""
import os

import numpy as np

from tests import golden_util as gu
from tests import host_program as hp
from tests import palette_place_ref as pp

FIXTURE = os.path.join(gu.GOLDEN_DIR, "palette_sockets_expect.npz")
ROOT = hp.ROOT
F = np.float32
NONE, POSE, MATRIX = 0, 1, 2             # the `form` of a fixture row: what its offset is


# ---- the restatement ------------------------------------------------------------------------------
def offset_matrix(g_rest):
    """rest positions f32 [..., 3] -> G f32 [..., 16]: the identity with row 4 = {p.x, p.y, p.z, 1}."""
    p = np.asarray(g_rest, F)
    g = np.zeros(p.shape[:-1] + (16,), F)
    g[..., 0] = g[..., 5] = g[..., 10] = g[..., 15] = F(1.0)
    g[..., 12:15] = p
    return g


def bone_frame(s, rest):
    """B = G * S (broadcast against each other): the full four-term sums, the rows where G is 0 and 1 included."""
    return pp.place(offset_matrix(rest), np.asarray(s, F))


def offsets_as_matrices(offset, matrix):
    """A desc's offsets f32 [NS, 8] (poses) or [NS, 16] (matrices) -> O f32 [NS, 16], as the library's host table builder expands them."""
    return np.asarray(offset, F).reshape(-1, 16).copy() if matrix else pp.matrix_from_pose(np.asarray(offset, F).reshape(-1, 8))


def sockets(palettes, bone, rest, offset=None, matrix=False, has_offset=None):
    """palettes f32 [NI, NB, 16]; bone u32 [NS]; rest f32 [NS, 3]; offset None, [NS, 8] or (matrix) [NS, 16]; has_offset None or
    bool [NS] -> f32 [NS, NI, 16], socket-major like the call's output."""
    pal = np.asarray(palettes, F)
    bone = np.asarray(bone).reshape(-1)
    rest = np.asarray(rest, F).reshape(-1, 3)
    b = bone_frame(pal[:, bone, :].transpose(1, 0, 2), rest[:, None, :])            # [NS, NI, 16]
    if offset is None:
        return b
    o = offsets_as_matrices(offset, matrix)
    with_o = pp.place(o[:, None, :], b)
    has = np.ones(bone.size, bool) if has_offset is None else np.asarray(has_offset).astype(bool)
    return np.where(has[:, None, None], with_o, b)


def socket_rows(forms, s, rest, offsets):
    """Fixture rows: forms u8 [N], s f32 [N, 16], rest f32 [N, 3], offsets f32 [N, 16] (a pose row uses the first 8) -> [N, 16]."""
    forms = np.asarray(forms)
    b = bone_frame(s, rest)
    o = np.where((forms == POSE)[:, None], pp.matrix_from_pose(offsets[:, :8]), offsets)
    return np.where((forms == NONE)[:, None], b, pp.place(o, b))


assert_rows_equal = gu.assert_bits_equal_or_both_nan


# ---- the two drivers ------------------------------------------------------------------------------
def build_libmmd_driver() -> str:
    return hp.build("palette_sockets_driver", [os.path.join(hp.TESTS, "palette_sockets_driver.cpp")], strict=False, include=[hp.REF_INC])


def build_math_driver(sanitize: bool = False) -> str:
    return hp.build("socket_math_driver", [os.path.join(hp.TESTS, "socket_math_driver.cpp"), os.path.join(hp.CSRC, "error.cpp")],
                    sanitize=sanitize)


def run_driver(exe, forms, s, rest, offsets):
    """The rows through one of the drivers (text in, text out, floats as hex bit patterns) -> f32 [N, 16]."""
    forms = np.asarray(forms)
    rest4 = np.zeros((forms.size, 4), F)
    rest4[:, :3] = rest
    words = np.concatenate([gu.bits(s).reshape(-1, 16), gu.bits(rest4), gu.bits(offsets).reshape(-1, 16)], axis=1)
    stdin = "".join("%d %s\n" % (f, hp.hex_words(row)) for f, row in zip(forms, words))
    out = hp.parse_hex_rows(hp.run(exe, stdin=stdin).stdout, 16)
    assert out.shape == (forms.size, 16), out.shape
    return out.view(F)


# ---- the fixture ----------------------------------------------------------------------------------
def fixture():
    """dict: form u8 [N] (0 no offset, 1 pose, 2 matrix), kind [N] (what the row is there for), s f32 [N, 16], rest f32 [N, 3],
    offset f32 [N, 16] (a pose row holds its 8 floats first, zeros behind; zeros for form 0), expect f32 [N, 16] (the real libmmd)."""
    z = np.load(FIXTURE)
    out = {k: z[k] for k in z.files}
    out["kind"] = [str(k) for k in z["kind"]]
    return out
