"""Models whose morph gather table has CHOSEN slice lengths, and the slice lengths restated.

The table (csrc/plan.cpp) is a sliced ELL: one slice per 64 consecutive engine slots, every row of a slice padded to the slice's
longest row.  The plan orders the vertices of a 512-vertex tile by deform class (BDEF1, BDEF2 / SDEF, BDEF4) and, inside a class,
by the number of morph entries on the vertex -- BDEF1 longest first, BDEF2 shortest first, BDEF4 longest first.  A tile of ONE
class is therefore a monotone sequence of row lengths cut into eight slices, and `ladder()` steers it: per tile a class and eight
slice lengths; slice i gets FULL lanes with exactly that many entries and 64 - FULL lanes with fewer (down to the neighbouring
slice's length), so that the longest row is real and padding is read.  A fourth tile keeps synth.make_model's class mix (slices
straddle class boundaries there), a fifth has three vertices.

Every vertex draws its morphs without replacement from NM vertex morphs, so an entry count is a number of DISTINCT slots and every
morph's rate matters somewhere.  tests/test_morph_rows.py is the user."""
import numpy as np

from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.synth import BDEF1, BDEF2, BDEF4, MORPH_GROUP, MORPH_VERTEX

TILE, SLICE = 512, 64                 # kTileVerts, lanes of a slice
NB, NM = 17, 80
FULL = 40                             # lanes of a slice that carry the slice's length

# one below, at and above every pipeline depth of the walks (4, 8, 16) and twice every depth; LONG: more than two refills at depth 16
REQUIRED = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33)
LONG = 65

# (class, slice lengths in ENGINE order): BDEF2 ascends, BDEF1 and BDEF4 descend
LADDER = ((BDEF2, (0, 1, 2, 3, 4, 5, 6, 7)), (BDEF1, (33, 32, 31, 17, 16, 15, 9, 8)), (BDEF4, (67, 33, 17, 16, 9, 8, 4, 0)))
# the same without the long row: fast-math models keep their rows at 33 entries (the contraction bound of the test is n^2)
LADDER33 = ((BDEF2, (0, 1, 2, 3, 4, 5, 6, 7)), (BDEF1, (33, 32, 31, 17, 16, 15, 9, 8)), (BDEF4, (33, 32, 17, 16, 9, 8, 4, 0)))
NV = (len(LADDER) + 1) * TILE + 3     # 2051: three steered tiles, one mixed, one of three vertices
LAST_TILE_COUNTS = (6, 3, 0)


def _steered_counts(lengths, ascending):
    """Row lengths of a one-class tile in engine order: slice i = FULL lanes of lengths[i] and 64 - FULL shorter ones that stay
    on the slice's side of its neighbour's length (so the class's sort reproduces the sequence)."""
    out = []
    for i, length in enumerate(lengths):
        if ascending:
            bound = lengths[i - 1] if i else 0
        else:
            bound = lengths[i + 1] if i + 1 < len(lengths) else 0
        assert bound <= length
        lo, hi = bound, max(length - 1, bound)
        short = np.rint(np.linspace(hi, lo, SLICE - FULL)).astype(np.int64) if length else np.zeros(SLICE - FULL, np.int64)
        full = np.full(FULL, length, np.int64)
        out.append(np.concatenate([short[::-1], full]) if ascending else np.concatenate([full, short]))
    return np.concatenate(out)


def ladder(tiles=LADDER, offset_scale=None, pos_scale=1.0, seed=4711):
    """The ladder model (NV = 2051, 17 bones, 80 vertex morphs).  offset_scale = a: offsets of magnitude a/2 .. a per component
    (else uniform in +-0.5); pos_scale shrinks the vertex and bone rest positions.  meta["counts"]: entries per file vertex."""
    m = synth.make_model(NV, NB, 1, 1, seed)
    rng = np.random.RandomState(seed + 1)
    counts = np.zeros(NV, np.int64)
    for t, (cls, lengths) in enumerate(tiles):
        assert len(lengths) == TILE // SLICE
        v = np.arange(t * TILE, (t + 1) * TILE)
        m.skin_type[v] = cls
        w = np.zeros((TILE, 4), np.float32)
        if cls == BDEF2:
            w[:, 0] = rng.uniform(0.01, 0.99, TILE)
        elif cls == BDEF4:
            w4 = rng.uniform(0.01, 1.0, size=(TILE, 4))
            w[:] = w4 / w4.sum(1, keepdims=True)
        m.bone_weights[v] = w
        # file order inside the tile is a shuffle of the engine order: the plan's permutation is not the identity
        counts[v[rng.permutation(TILE)]] = _steered_counts(lengths, cls == BDEF2)
    mixed = np.arange(len(tiles) * TILE, (len(tiles) + 1) * TILE)
    counts[mixed] = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 18], size=TILE)
    counts[mixed[-1] + 1:] = LAST_TILE_COUNTS
    hit = [[] for _ in range(NM)]
    for v in rng.permutation(NV):
        for k in rng.choice(NM, counts[v], replace=False):
            hit[k].append(v)
    assert all(hit), "a morph without entries"
    m.morph_type = np.full(NM, MORPH_VERTEX, np.int32)
    m.morph_off = np.concatenate([[0], np.cumsum([len(h) for h in hit])]).astype(np.uint32)
    m.morph_index = np.concatenate(hit).astype(np.uint32)
    ne = int(m.morph_off[-1])
    if offset_scale is None:
        val = rng.uniform(-0.5, 0.5, size=(ne, 3))
    else:
        val = rng.uniform(0.5, 1.0, size=(ne, 3)) * offset_scale * rng.choice([-1.0, 1.0], size=(ne, 3))
    m.morph_value = np.ascontiguousarray(val, np.float32)
    m.positions = np.ascontiguousarray(m.positions * np.float32(pos_scale))
    m.bone_pos = np.ascontiguousarray(m.bone_pos * np.float32(pos_scale))
    # -0.0 components: on vertices without entries (the sum stays +0: -0 + +0 = +0) and on morphed ones
    for v in (np.flatnonzero(counts == 0)[:3], np.flatnonzero(counts > 4)[:3]):
        m.positions[v, np.arange(3)] = np.float32(-0.0)
    m.meta = dict(nv=NV, nb=NB, nm=NM, seed=seed, counts=counts)
    return m


# morphs of the non-finite variants that carry the bad offsets; their rates are skipped in every instance
BAD_MORPHS = (11, 37, 59)


def with_nonfinite_offsets(m, f16):
    """One inf and one NaN offset component -- and, for an f16 model, a finite 70000.0 that rounds to inf as binary16 -- each on
    the LONGEST row its morph touches.  Row lengths do not change."""
    m = m.copy()
    counts = m.meta["counts"]
    for k, bad in zip(BAD_MORPHS, (np.inf, np.nan, 70000.0 if f16 else None)):
        if bad is None:
            continue
        lo, hi = int(m.morph_off[k]), int(m.morph_off[k + 1])
        e = lo + int(np.argmax(counts[m.morph_index[lo:hi]]))
        m.morph_value[e, k % 3] = np.float32(bad)
    return m


def many_slots(seed=4720):
    """At least 600 morph slots on short rows: 600 vertex morphs of three vertices each over 1027 vertices, and three group morphs
    (one nested, sub-rates around the 1e-7 skip) that expand 30 of them once more."""
    nv, nm = 2 * TILE + 3, 600
    m = synth.make_model(nv, NB, nm, 3, seed)
    rng = np.random.RandomState(seed + 1)
    subs = rng.choice(nm, 30, replace=False)
    idx, val, off = list(m.morph_index), [tuple(x) for x in m.morph_value], list(m.morph_off)
    for g in range(3):
        for s in subs[g * 10:(g + 1) * 10]:
            idx.append(int(s))
            val.append((float(rng.choice([0.5, 1.0, 2.0, 1e-4])), 0.0, 0.0))
        if g == 2:                         # depth 2: the last group also applies the first
            idx.append(nm)
            val.append((0.75, 0.0, 0.0))
        off.append(len(idx))
    m.morph_type = np.concatenate([m.morph_type, [MORPH_GROUP] * 3]).astype(np.int32)
    m.morph_off = np.asarray(off, np.uint32)
    m.morph_index = np.asarray(idx, np.uint32)
    m.morph_value = np.asarray(val, np.float32).reshape(-1, 3)
    return m


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def entry_counts(m):
    """(entries per file vertex, slots) after group expansion -- plan.cpp's SlotBuilder restated: the morphs in file order, a group
    morph expands to its sub-morphs depth first, every visit of a vertex morph is one slot."""
    cnt = np.zeros(m.nv, np.int64)
    slots = 0

    def visit(k, depth):
        nonlocal slots
        assert depth <= 16
        lo, hi = int(m.morph_off[k]), int(m.morph_off[k + 1])
        if m.morph_type[k] == MORPH_VERTEX:
            slots += 1
            np.add.at(cnt, np.asarray(m.morph_index[lo:hi], np.int64), 1)
        elif m.morph_type[k] == MORPH_GROUP:
            for j in range(lo, hi):
                visit(int(m.morph_index[j]), depth + 1)
    for k in range(m.nm):
        visit(k, 0)
    return cnt, slots


def slice_rows(engine_to_original, cnt):
    """Row lengths of every slice's lanes: a list, one int array per slice of 64 engine slots (8 slices per tile; the slices
    behind the last vertex are empty), from mmdx_model_get_vertex_order's engine_to_original and entry_counts()."""
    nv = len(engine_to_original)
    ntiles = (nv + TILE - 1) // TILE
    rows = cnt[np.asarray(engine_to_original, np.int64)]
    return [rows[g0:g0 + SLICE] for g0 in range(0, ntiles * TILE, SLICE)]


def slice_lengths(engine_to_original, cnt):
    """The padded length of every slice: its longest row."""
    return [int(r.max()) if r.size else 0 for r in slice_rows(engine_to_original, cnt)]


# ---- rates ---------------------------------------------------------------------------------------------------------------------------
def instance_rates(nm, ni, pack, floor=0.05, skipped=()):
    """Per-instance rates [ni, nm]: every instance its own, floor + (1 - floor) * ((13 i + 7 k) mod 97) / 96, so that
    consecutive packs (of 4 or 8) differ in every slot; the FIRST pack wholly below the 1e-7 skip (negative, zero, 5e-8 by thirds
    of the morphs) -- the later packs of a workgroup, which walk from a head requested between the packs, apply everything; single
    skips of all three kinds scattered over the instances behind the second pack; `skipped` morphs below the skip in every
    instance."""
    i, k = np.arange(ni)[:, None], np.arange(nm)[None, :]
    r = (floor + (1.0 - floor) * ((13 * i + 7 * k) % 97) / 96.0).astype(np.float32)
    assert all((r[i] != r[i + pack]).all() for i in range(ni - pack))
    kinds = np.array([-1.0, 0.0, 5e-8], np.float32)
    r[:pack] = np.where(np.arange(nm) % 3 == 0, -r[:pack], kinds[np.arange(nm) % 3])
    for i in range(2 * pack, ni):
        for j, k in enumerate(((5 * i + 1) % nm, (11 * i + 2) % nm, (17 * i + 3) % nm)):
            r[i, k] = kinds[j]
    for j, k in enumerate(skipped):
        r[:, k] = kinds[(np.arange(ni) + j) % 3]
    return r


def shared_rates(nm, frame, floor=0.05, skipped=()):
    """One set of rates: everything applied except three morphs (negative, zero, 5e-8) and `skipped`."""
    r = np.maximum(synth.morph_weights(nm, [frame])[0], np.float32(floor))
    r[[3 % nm, 29 % nm, 71 % nm]] = (-0.5, 0.0, 5e-8)
    r[list(skipped)] = (0.0, -1.0, 5e-8)[:len(skipped)]
    return r
