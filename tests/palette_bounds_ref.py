"""mmdx_palette_bounds (include/mmdx.h): the checkers the tests share.

  * a numpy restatement of the bone-box table (bone_box_table) and of the box arithmetic (row_boxes / palette_bounds), written
    from the header's text: float32 operations one rounding each, every sum left to right, double only where the header says so;
  * the project's own arithmetic header on the CPU through tests/pbounds_math_driver.cpp.
Boxes are compared bit for bit, except that a NaN only has to be a NaN (sign and payload are not part of the contract).
Nothing compiled here is committed.
"""
import os

import numpy as np

from tests import golden_util as gu
from tests import host_program as hp

HERE, ROOT = hp.TESTS, hp.ROOT
F = np.float32
INF = F(np.inf)
U = 2.0 ** -24
VERTEX, GROUP = 1, 0

assert_rows_equal = gu.assert_bits_equal_or_both_nan


# ---- the table ------------------------------------------------------------------------------------
def vertex_morph_entries(model):
    """(vertex u32 [E'], offset f32 [E', 3]) of every vertex-morph entry after group expansion, in the accumulation order: top-level
    morphs ascending, a group's sub-morphs depth first in place, file order inside a morph.  One entry per slot application."""
    mt, mo = np.asarray(model.morph_type), np.asarray(model.morph_off, np.int64)
    mi, mv = np.asarray(model.morph_index, np.int64), np.asarray(model.morph_value, F).reshape(-1, 3)
    verts, offs = [], []

    def visit(m, depth):
        assert depth <= 64
        lo, hi = int(mo[m]), int(mo[m + 1])
        if mt[m] == VERTEX:
            verts.append(mi[lo:hi])
            offs.append(mv[lo:hi])
        elif mt[m] == GROUP:
            for j in range(lo, hi):
                visit(int(mi[j]), depth + 1)
    for m in range(len(mt)):
        visit(m, 0)
    if not verts:
        return np.zeros(0, np.int64), np.zeros((0, 3), F)
    return np.concatenate(verts), np.concatenate(offs)


def bone_box_table(model, skin, f16=False):
    """The table of include/mmdx.h from a FlatModel and its post-Normalize skin (type, ids, weights as mmdx_model_get_skin returns
    them) -> dict like DeformModel.bone_boxes()."""
    typ, ids, w = (np.asarray(x) for x in skin)
    w = w.astype(F)
    nv, nb = model.nv, model.nb
    pos = np.asarray(model.positions, F)
    ev, eo = vertex_morph_entries(model)
    if f16:
        with np.errstate(over="ignore"):
            pos, eo = pos.astype(np.float16).astype(F), eo.astype(np.float16).astype(F)
    cnt = np.bincount(ev, minlength=nv)
    r64 = np.zeros((nv, 3), np.float64)
    np.add.at(r64, ev, np.abs(eo.astype(np.float64)))                  # unbuffered, in entry order
    R = np.nextafter(r64.astype(F), INF)
    used = np.zeros((nv, 4), bool)
    one_minus = F(1.0) - w[:, 0]
    b1, b2, b4 = typ == 0, typ == 1, typ == 2
    assert (b1 | b2 | b4).all()
    used[b1, 0] = True
    used[b2, 0] = w[b2, 0] != 0
    used[b2, 1] = one_minus[b2] != 0
    used[b4] = w[b4] != 0
    s = np.ones(nv, np.float64)
    s[b2] = w[b2, 0].astype(np.float64) + one_minus[b2].astype(np.float64)
    s4 = np.zeros(nv, np.float64)
    for k in range(4):
        s4 = s4 + w[:, k].astype(np.float64)
    s[b4] = s4[b4]
    wdev = np.nextafter(F(np.abs(s - 1.0).max()), INF)
    nonconvex = (b4 & (w < 0).any(axis=1)) | (b2 & ((w[:, 0] < 0) | (w[:, 0] > 1)))
    bones, boxes = [], []
    for b in range(nb):
        mine = (used & (ids == b)).any(axis=1)
        if not mine.any():
            continue
        bones.append(b)
        boxes.append(np.concatenate([pos[mine].min(axis=0), pos[mine].max(axis=0), R[mine].max(axis=0)]))
    r_max = int(cnt.max()) if nv else 0
    eps = F(F((32 + r_max) * U) + wdev)
    return dict(bones=np.array(bones, np.uint32), boxes=np.array(boxes, F).reshape(-1, 9), n_boxes=len(bones),
                n_nonconvex=int(nonconvex.sum()), max_vertex_entries=r_max, eps=eps, weight_sum_dev=wdev)


# ---- the arithmetic -------------------------------------------------------------------------------
def _min(a, b):
    return np.where(b < a, b, a)


def _max(a, b):
    return np.where(a < b, b, a)


def row_boxes(boxes, mats, eps, morph_scale):
    """boxes f32 [n, 9], mats f32 [..., n, 16] (the matrix of each row's bone) -> (blo, bhi, pad) f32 [..., n, 3] each."""
    boxes, mats = np.asarray(boxes, F).reshape(-1, 9), np.asarray(mats, F)
    eps, ms = F(eps), F(morph_scale)
    lo, hi, reach = boxes[:, 0:3], boxes[:, 3:6], boxes[:, 6:9]
    blo, bhi, pads = (np.empty(mats.shape[:-1] + (3,), F) for _ in range(3))
    with np.errstate(all="ignore"):
        g = reach * ms
        L, H = lo - g, hi + g
        for j in range(3):
            pl = [L[:, k] * mats[..., 4 * k + j] for k in range(3)]
            ph = [H[:, k] * mats[..., 4 * k + j] for k in range(3)]
            t = mats[..., 12 + j]
            mn = ((_min(pl[0], ph[0]) + _min(pl[1], ph[1])) + _min(pl[2], ph[2])) + t
            mx = ((_max(pl[0], ph[0]) + _max(pl[1], ph[1])) + _max(pl[2], ph[2])) + t
            a = ((_max(np.abs(pl[0]), np.abs(ph[0])) + _max(np.abs(pl[1]), np.abs(ph[1]))) + _max(np.abs(pl[2]), np.abs(ph[2]))) + np.abs(t)
            pad = a * eps
            assert mn.dtype == F and pad.dtype == F
            blo[..., j], bhi[..., j], pads[..., j] = mn - pad, mx + pad, pad
    return blo, bhi, pads


def _key(x):
    b = np.ascontiguousarray(x, F).view(np.int32)
    return b ^ ((b >> 31) & np.int32(0x7fffffff))


def _unkey(k):
    k = np.ascontiguousarray(k, np.int32)
    return (k ^ ((k >> 31) & np.int32(0x7fffffff))).view(F)


def fold(blo, bhi, pos_scale):
    """blo, bhi f32 [NI, n, 3] -> rows f32 [NI, 6]: minimum / maximum in the total order (-0 < +0), times pos_scale; a NaN anywhere
    in an instance, or n == 0, makes its row NaN."""
    ni, n = blo.shape[0], blo.shape[1]
    out = np.full((ni, 6), np.nan, F)
    if n == 0:
        return out
    bad = np.isnan(blo).any(axis=(1, 2)) | np.isnan(bhi).any(axis=(1, 2))
    with np.errstate(all="ignore"):
        rows = np.concatenate([_unkey(_key(blo).min(axis=1)), _unkey(_key(bhi).max(axis=1))], axis=1) * F(pos_scale)
    out[~bad] = rows[~bad]
    return out


def palette_bounds(table, palettes, pos_scale, morph_scale):
    """The call: table as bone_box_table returns it, palettes f32 [NI, NB, 16] -> f32 [NI, 6]."""
    pal = np.asarray(palettes, F)
    mats = pal[:, table["bones"].astype(np.int64), :]
    blo, bhi, _ = row_boxes(table["boxes"], mats, table["eps"], morph_scale)
    return fold(blo, bhi, pos_scale)


def max_pad(table, palettes, pos_scale, morph_scale):
    """f32 [NI, 3]: the largest pad of any row per instance and axis, times pos_scale."""
    pal = np.asarray(palettes, F)
    _, _, pad = row_boxes(table["boxes"], pal[:, table["bones"].astype(np.int64), :], table["eps"], morph_scale)
    return pad.max(axis=1) * F(pos_scale)


# ---- the driver -----------------------------------------------------------------------------------
def build_math_driver(sanitize: bool = False) -> str:
    return hp.build("pbounds_math_driver", [os.path.join(HERE, "pbounds_math_driver.cpp")], sanitize=sanitize)


def run_driver(exe, boxes, mats, eps, morph_scale, pos_scale):
    """boxes f32 [n, 9], mats f32 [NI, n, 16] through the driver (text in, text out, floats as hex bit patterns) -> f32 [NI, 6]."""
    boxes, mats = np.asarray(boxes, F).reshape(-1, 9), np.asarray(mats, F)
    ni, n = mats.shape[0], boxes.shape[0]
    lines = ["%d %d %s" % (n, ni, hp.hex_words(np.array([eps, morph_scale, pos_scale], F)))]
    lines += [hp.hex_words(r) for r in boxes]
    lines += [hp.hex_words(mats[i, r]) for i in range(ni) for r in range(n)]
    out = hp.parse_hex_rows(hp.run(exe, stdin="\n".join(lines) + "\n").stdout, 6)
    assert out.shape == (ni, 6), out.shape
    return out.view(F)
