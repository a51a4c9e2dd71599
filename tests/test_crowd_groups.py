"""The crowd kernel's loop over a workgroup's instances, with SEVERAL instances per workgroup, at small shapes.

The launch planner (csrc/launch_shape.cpp) halves the group while ntiles * ceil(ni / group) < 2048, so every small crowd -- all the
ragged sweeps, pitch, bounds, select, tile-order and fast-math tests -- runs with one instance (one pack, per-instance weights)
per workgroup: `pal + g * pal_stride` for g > 0, the double-buffered stage image, both instance mappings and their gcount
arithmetic, a bad select id in the middle of a group and the pack-to-pack weight swap never run there.  That is the gap this file
closes: MMDX_GROUP forces a real group on crowds of a few dozen instances, mmdx_debug_last_launch_shape proves after every call
that the claimed shape ran, and every byte is compared with the oracle.

CPU: the case table ROWS is validated against the planner itself (tests/launch_shape_driver.cpp) and against the kernel's gcount
formulas restated here -- every row really has workgroups of three and more instances and a partial last group; without
MMDX_GROUP every row plans group == gmin.
GPU: every instantiation of deform_kernel once with such a group (a census of all 194), both instance mappings, dense and pitched
outputs, bounds, select lists with a bad id inside a group, fast math grouped against ungrouped, and one crowd large enough that
the planner picks a group by itself."""
import collections
import os

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count
from tests import host_program as hp

BPV = {api.OUT_SOA: (12, 12), api.OUT_VERTEX32: (32, 0), api.OUT_SOA_POS16: (6, 12)}   # bytes per vertex of out_a, out_b
TAIL = 64                                                                            # sentinel bytes behind the last instance
DEV = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE
NONE, SHARED, FUSED1, FUSED4 = 0, 1, 2, 3                                             # kMorph* (csrc/lds_layout.hpp)
MORPH_NAMES = {NONE: "none", SHARED: "shared-pass", FUSED1: "shared-gathered", FUSED4: "per-instance"}
LAYOUTS = ((api.OUT_SOA, False), (api.OUT_VERTEX32, False), (api.OUT_SOA_POS16, True))   # (layout, f16 model)
NB = 17
TILE = 512                                                                           # kTileVerts

# ---- the case table -----------------------------------------------------------------------------------------------------------------
# One row per launch shape.  ni: instances of the crowd; group / threads: MMDX_GROUP / MMDX_THREADS; n_ids / count: capacity and
# live prefix of the row's select list (the select launch is sized from n_ids).  File-order rows without per-instance weights
# take groups above 16 (production reaches them there only: the planner caps tile-order and per-instance-weight launches at 16 and
# write-through launches at 8).  Per-instance weights at 512 threads walk packs of 8, so the cap of 16 allows two packs per
# workgroup there and no more; at 256 threads (packs of 4) a workgroup has four.
Row = collections.namedtuple("Row", "name nv ni group threads morph tile_order write_through n_ids count")


def _rows():
    rows = []
    for threads in (256, 512):
        for tile in (False, True):
            # both vertex counts under both thread counts and both vertex orders: 1000 = 2 tiles (ntiles < 8: the remainder half of
            # map_workgroup), dense full tiles take the aligned copy-out; 4099 = 9 tiles (both halves), last tile 3 vertices, dense
            # instances start off 16-byte boundaries
            nv = 4099 if (threads == 256) != tile else 1000
            order = "tile" if tile else "file"
            for morph in (NONE, SHARED, FUSED1):
                ni, group, n_ids = (37, 16, 40) if tile else (45, 24, 48)
                rows.append(Row(f"{MORPH_NAMES[morph]}-{threads}-{order}", nv, ni, group, threads, morph, tile, False, n_ids, ni))
            rows.append(Row(f"{MORPH_NAMES[FUSED4]}-{threads}-{order}", nv, 45, 16, threads, FUSED4, tile, False, 48, 45))
    for morph in (NONE, SHARED):
        rows.append(Row(f"{MORPH_NAMES[morph]}-256-file-wt", 4099, 19, 8, 256, morph, False, True, 0, 0))
    # a last workgroup with ONE instance beside full ones (blocked 4, 4, 4, 1; interleaved 4, 3, 3, 3)
    rows.append(Row("none-256-file-tail1", 1000, 13, 4, 256, NONE, False, False, 16, 13))
    rows.append(Row("per-instance-256-tile-tail1", 1000, 13, 4, 256, FUSED4, True, False, 16, 13))
    return rows


ROWS = _rows()
ROW = {(r.threads, r.morph, r.tile_order): r for r in ROWS if not r.write_through and "tail1" not in r.name}
WT_ROW = {r.morph: r for r in ROWS if r.write_through}
TAIL1_ROWS = [r for r in ROWS if "tail1" in r.name]
BAD_POS = {48: 10, 40: 10, 16: 5}            # list position of the id >= ni, by the list's capacity


def gmin_of(row):
    return (8 if row.threads == 512 else 4) if row.morph == FUSED4 else 1


def interleaved(row, ilv):
    """deform_kernel's `ilv`: never with per-instance weights."""
    return bool(ilv) and row.morph != FUSED4


def gcounts(row, ilv, select):
    """gcount of every workgroup of one tile -- deform_kernel's formulas (kernels.hip) restated: plain and SELECT, interleaved
    and blocked.  select: over the live prefix `count` of a list of capacity n_ids."""
    n = row.n_ids if select else row.ni
    ngroups = (n + row.group - 1) // row.group
    out = []
    for grp in range(ngroups):
        inst0 = grp if interleaved(row, ilv) else grp * row.group
        if select:
            nlive = min(row.count, row.n_ids)
            end = min(inst0 + row.group, nlive)
            g = min(row.group, (nlive + ngroups - 1 - grp) // ngroups) if interleaved(row, ilv) else (end - inst0 if end > inst0 else 0)
        elif interleaved(row, ilv):
            g = min(row.group, (row.ni - grp + ngroups - 1) // ngroups) if row.ni > grp else 0
        else:
            g = min(row.group, row.ni - inst0)
        out.append(g)
    return out


def slot_of(row, ilv, pos):
    """(workgroup, g, gcount) of list position `pos` of the row's select launch."""
    ngroups = (row.n_ids + row.group - 1) // row.group
    grp, g = (pos % ngroups, pos // ngroups) if interleaved(row, ilv) else (pos // row.group, pos % row.group)
    return grp, g, gcounts(row, ilv, True)[grp]


def expected_variants():
    """for_each_deform_variant (kernels.hip) restated: (threads, layout, morph, f16, tile_order, write_through, bounds, select)."""
    out = set()
    for threads in (256, 512):
        for layout, f16 in LAYOUTS:
            for morph in (NONE, SHARED, FUSED1, FUSED4):
                for tile in (0, 1):
                    for bounds in (0, 1):
                        for select in (0, 1):
                            out.add((threads, layout, morph, int(f16), tile, 0, bounds, select))
                if threads == 256 and layout == api.OUT_SOA and morph in (NONE, SHARED):
                    out.add((threads, layout, morph, 0, 0, 1, 0, 0))
    return out


# ---- models and inputs ------------------------------------------------------------------------------------------------------------
def make_flat(nv, morphs):
    m = synth.make_model(nv, NB, 6 if morphs else 1, min(nv, 60) if morphs else 1, seed=8800 + nv)
    if not morphs:
        m.morph_type = np.zeros(0, np.int32)
        m.morph_off = np.zeros(1, np.uint32)
        m.morph_index = np.zeros(0, np.uint32)
        m.morph_value = np.zeros((0, 3), np.float32)
    return m


def crowd_inputs(m, ni, morph):
    """Every instance its own palette; with per-instance weights every instance its own rates, a whole pack below the 1e-7 skip
    (negative, zero, tiny) next to packs that apply everything."""
    pals = synth.make_palettes(m, np.arange(ni) * 3 + 1)
    if morph == NONE:
        return pals, np.zeros((ni, 0), np.float32), False
    rates = synth.morph_weights(m.nm, np.arange(ni) * 7 + 2)
    if morph != FUSED4:
        return pals, rates[:1].copy(), True
    rates = np.maximum(rates, np.float32(0.05))
    rates[8:16] *= -1.0
    rates[20:24] = 0.0
    rates[24:28] = 5e-8
    return pals, rates, False


# ---- CPU: the table against the planner ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner():
    """tests/launch_shape_driver.cpp `eval`: the program tests/test_launch_shape.py builds, by the same arguments."""
    exe = hp.build("launch_shape_driver", [os.path.join(hp.TESTS, "launch_shape_driver.cpp"), os.path.join(hp.CSRC, "launch_shape.cpp")],
                   sanitize=True)

    def plan(cases):
        """cases: dicts of the driver's Case fields (missing: the defaults) -> dicts of the planned shapes."""
        order = ("f16 tile_order ntiles max_tile_bones ns layout ni nwork flags morph bounds select out_dev out_host_mapped out_bytes "
                 "threads group lds_target fused_pack store_wt frame_kernel stagger").split()
        dflt = dict(flags=0, bounds=0, select=0, out_dev=1, out_host_mapped=0, out_bytes=1 << 20, threads=0, group=0, lds_target=0,
                    fused_pack=0, store_wt=-1, frame_kernel=1, stagger=0)
        text = "".join(" ".join(str(int(dict(dflt, **c)[k])) for k in order) + "\n" for c in cases)
        r = hp.run(exe, ["eval"], stdin=text)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return [{k: int(v) for k, v in (kv.split("=", 1) for kv in line.split(" "))} if line.startswith("status=0 ") else {"error": line}
                for line in lines]
    return plan


SCALARS = {}


def model_scalars(hip_lib, nv, morphs, f16, tile):
    """The model scalars the planner reads, from a MMDX_CREATE_HOST_ONLY handle."""
    key = (nv, morphs, f16, tile)
    if key not in SCALARS:
        with DeformModel(make_flat(nv, morphs), host_only=True, f16_positions=f16, tile_order=tile) as dm:
            SCALARS[key] = dict(f16=f16, tile_order=tile, ntiles=dm.info.n_tiles, max_tile_bones=dm.info.max_tile_bones,
                                ns=dm.info.n_slots)
    return SCALARS[key]


def test_case_table_forces_groups_the_planner_would_not_pick(hip_lib, planner):
    """The reviewer's check on a machine without a GPU.  Per row: the planner, given MMDX_GROUP / MMDX_THREADS, returns the
    deform kernel with exactly that group and those threads -- and WITHOUT MMDX_GROUP it returns group == gmin, which is why no
    other small-shape test reaches the code below; with the kernel's gcount formulas some workgroup serves >= 3 instances and
    the last group is partial, in both mappings, plain and select.  Across the table: the shapes listed in the asserts."""
    cases, meta = [], []
    for row in ROWS:
        for layout, f16 in LAYOUTS:
            if row.write_through and layout != api.OUT_SOA:
                continue
            sc = model_scalars(hip_lib, row.nv, row.morph != NONE, f16, row.tile_order)
            assert sc["ntiles"] == (row.nv + TILE - 1) // TILE and sc["max_tile_bones"] <= NB
            assert (sc["ns"] > 0) == (row.morph != NONE)
            for bounds, select in ((0, 0), (1, 0), (0, 1), (1, 1)):
                if (row.write_through and (bounds or select)) or (select and not row.n_ids):
                    continue
                call = dict(sc, layout=layout, ni=row.ni, nwork=row.n_ids if select else row.ni, morph=row.morph, bounds=bounds,
                            select=select, threads=row.threads, flags=api.OUT_STORES_WRITE_THROUGH if row.write_through else 0)
                cases += [dict(call, group=row.group), call]
                meta.append((row, layout, bounds, select))
    shapes = planner(cases)
    for k, (row, layout, bounds, select) in enumerate(meta):
        forced, free = shapes[2 * k], shapes[2 * k + 1]
        what = f"{row.name} layout={layout} bounds={bounds} select={select}"
        assert "error" not in forced and "error" not in free, what
        assert (forced["kernel"], forced["group"], forced["threads"]) == (1, row.group, row.threads), (what, forced)
        assert forced["write_through"] == int(row.write_through), what
        # the gap: on their own these crowds get the smallest group there is
        assert free["kernel"] == 1 and free["group"] == gmin_of(row), (what, free)

    for row in ROWS:
        assert row.group % gmin_of(row) == 0
        for select in ((False, True) if row.n_ids else (False,)):
            for ilv in (1, 0):
                gc = gcounts(row, ilv, select)
                what = f"{row.name} select={select} ilv={ilv}: {gc}"
                assert max(gc) >= 3 and min(gc) < max(gc) and min(gc) >= 1, what
                assert sum(gc) == (row.count if select else row.ni), what
                if row.tile_order or row.morph == FUSED4:
                    assert max(gc) <= 16, what             # the planner's cap for these: production reaches no more
                if row.write_through:
                    assert max(gc) <= 8, what
        if row.n_ids:
            # the select list: more capacity than live ids, the count ends inside a workgroup, and the bad id is neither the first
            # nor the last live position of its workgroup, in both mappings
            assert row.count < row.n_ids
            for ilv in (1, 0):
                grp, g, gc = slot_of(row, ilv, BAD_POS[row.n_ids])
                assert 0 < g < gc - 1, (row.name, ilv, grp, g, gc)
                gc_all = gcounts(row, ilv, True)
                assert any(0 < c < max(gc_all) for c in gc_all), (row.name, ilv, gc_all)

    def some(pred):
        return [r.name for r in ROWS if pred(r)]
    # a gcount of exactly 1 beside full groups
    assert some(lambda r: gcounts(r, 0, False)[-1] == 1 and gcounts(r, 0, False)[0] == r.group)
    # more than 16 instances per workgroup, both mappings, in every file-order mode without per-instance weights
    for morph in (NONE, SHARED, FUSED1):
        for threads in (256, 512):
            assert some(lambda r: r.morph == morph and r.threads == threads and not r.tile_order and
                        min(max(gcounts(r, 1, False)), max(gcounts(r, 0, False))) > 16), (morph, threads)
    # per-instance weights: several packs per workgroup and a last pack that is neither full nor a whole quad -- at 256 threads
    # (packs of 4) at least three packs; at 512 threads (packs of 8) the two packs that the cap of 16 allows
    for threads, pack, packs in ((256, 4, 3), (512, 8, 2)):
        for tile in (False, True):
            assert some(lambda r: r.morph == FUSED4 and r.threads == threads and r.tile_order == tile and
                        any(-(-c // pack) >= packs and c % pack not in (0, 4) for c in gcounts(r, 0, False))), (threads, tile)
    # both halves of map_workgroup's XCD mapping; full tiles with and without the aligned copy-out
    tiles = {(r.nv + TILE - 1) // TILE for r in ROWS}
    assert any(t < 8 for t in tiles) and any(t > 8 and t & 7 for t in tiles)
    assert {r.nv % 4 for r in ROWS} >= {0, 3}
    # every (threads, morph, order) of the kernel's instantiations has its row
    assert set(ROW) == {(t, m, o) for t in (256, 512) for m in (NONE, SHARED, FUSED1, FUSED4) for o in (False, True)}
    assert len(expected_variants()) == 194


# the crowd of the one unforced row (g): 683 tiles x 9 instances
UNFORCED_NV, UNFORCED_NI, UNFORCED_GROUP = 682 * TILE + 1, 9, 4


def test_smallest_crowd_the_planner_groups_by_itself(hip_lib, planner):
    """Without MMDX_GROUP a shared-morph SoA crowd gets group >= 4 only from ntiles * ceil(ni / group) >= 2048 on.  The smallest
    such crowd, by output size (ntiles * ni tile-instances): every crowd of up to 8192 tile-instances is planned here, and the
    smallest that reaches group 4 is the GPU test's (9 instances start at group 9, halved to 4: 683 * ceil(9 / 4) = 2049)."""
    sc = model_scalars(hip_lib, UNFORCED_NV, True, False, False)
    assert sc["ntiles"] == 683
    pairs = [(nt, ni) for nt in range(1, 8193) for ni in range(2, 8192 // nt + 1)]
    shapes = planner([dict(sc, ntiles=nt, layout=api.OUT_SOA, ni=ni, nwork=ni, morph=SHARED, out_bytes=nt * TILE * ni * 24)
                      for nt, ni in pairs])
    grouped = sorted((nt * ni, ni, nt, s["group"]) for (nt, ni), s in zip(pairs, shapes) if s["kernel"] == 1 and s["group"] >= 4)
    assert grouped[0] == (683 * UNFORCED_NI, UNFORCED_NI, 683, UNFORCED_GROUP) and grouped[1][0] > grouped[0][0], grouped[:4]


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"


@pytest.fixture
def crowd_env(hip_lib):
    """Sets launch-shape overrides and re-reads them; the teardown REMOVES every variable it set and re-reads again, so that no
    override outlives the test."""
    saved = {}

    def _set(**env):
        for k, v in env.items():
            saved.setdefault(k, os.environ.get(k))
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        hip_lib.mmdx_debug_reload_env()
    yield _set
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    hip_lib.mmdx_debug_reload_env()


class Expect:
    """Oracle results of one model per (rates row, palette row), as the bytes of one instance of each layout; the f16 layout from
    a model whose positions and offsets went through binary16 once (as tests/test_instance_pitch.py)."""

    def __init__(self, oracle, m, order=None):
        self.o, self.m = oracle, m
        self.q = m.copy()
        self.q.positions = m.positions.astype(np.float16).astype(np.float32)
        self.q.morph_value = m.morph_value.astype(np.float16).astype(np.float32)
        self.skin, self.qskin = oracle.normalize(m), oracle.normalize(self.q)
        self.order = order          # engine_to_original of a tile-order model
        self.memo = {}

    def rows(self, layout, rates, pal, scale):
        key = (layout, rates.tobytes(), pal.tobytes(), scale)
        if key not in self.memo:
            o, m = self.o, self.m
            if layout == api.OUT_SOA_POS16:
                p, n = o.skin(self.q, pal, o.morph(self.q, rates), self.qskin)
                a, b = p.astype(np.float16), n
            else:
                p, n = o.skin(m, pal, o.morph(m, rates), self.skin)
                a, b = (p, n) if layout == api.OUT_SOA else (o.repack32(m, p, n, scale), None)
            if self.order is not None:
                a = a[self.order]
                b = b[self.order] if b is not None else None
            self.memo[key] = (np.ascontiguousarray(a).view(np.uint8).reshape(-1),
                              np.ascontiguousarray(b).view(np.uint8).reshape(-1) if b is not None else None)
        return self.memo[key]


class Models:
    """Handles and oracle expectations, made once per module."""

    def __init__(self, oracle):
        self.oracle, self.flat, self.dm, self.exp = oracle, {}, {}, {}

    def get(self, nv, morphs, f16=False, tile=False, fast=False):
        if (nv, morphs) not in self.flat:
            self.flat[nv, morphs] = make_flat(nv, morphs)
        key = (nv, morphs, f16, tile, fast)
        if key not in self.dm:
            self.dm[key] = DeformModel(self.flat[nv, morphs], f16_positions=f16, tile_order=tile, fast_math=fast)
        dm = self.dm[key]
        ekey = (nv, morphs, f16, tile)
        if ekey not in self.exp:
            self.exp[ekey] = Expect(self.oracle, self.flat[nv, morphs], dm.vertex_order()[0] if tile else None)
        return dm, self.exp[ekey]

    def close(self):
        for dm in self.dm.values():
            dm.close()


@pytest.fixture(scope="module")
def models(_gpu, oracle):
    m = Models(oracle)
    yield m
    m.close()


def positions(a, layout, nv):
    """f32 [nv, 3] positions as written, out of one instance's bytes of out_a."""
    if layout == api.OUT_SOA:
        return a.view(np.float32).reshape(nv, 3)
    if layout == api.OUT_VERTEX32:
        return a.view(np.float32).reshape(nv, 8)[:, :3]
    return a.view(np.float16).reshape(nv, 3).astype(np.float32)


def select_list(row):
    """The row's device list: the live prefix names all but two instances in a seeded random (non-monotonic) order, one of them
    twice, and one id >= ni at BAD_POS; behind the count: ids of the two instances that are NOT listed.  Returns (ids, listed)."""
    rng = np.random.default_rng(700 + row.ni + row.group)
    perm = rng.permutation(row.ni).astype(np.uint32)
    live = list(perm[:row.count - 2])
    live.insert(7, live[2])                                  # one id twice
    live.insert(BAD_POS[row.n_ids], row.ni + 5)              # one id outside the crowd
    assert len(live) == row.count
    unlisted = list(perm[row.count - 2:])
    dead = (unlisted * row.n_ids)[:row.n_ids - row.count]
    return np.array(live + dead, np.uint32), sorted(int(i) for i in perm[:row.count - 2])


def run(dm, row, layout, pals, rates, shared, pitch, scale, bounds, ids=None, host_list=False, flags=0):
    """One call with every operand in HBM into 0xFF-filled arrays.  ids: a select call; the device list has the row's capacity and
    count, the host list is passed whole.  Returns (out_a bytes, out_b bytes | None, bounds u32 [ni + 2, 6] | None)."""
    ni, rows_v = row.ni, pitch or dm.nv
    ba, bb = BPV[layout]
    na, nb = ni * rows_v * ba + TAIL, (ni * rows_v * bb + TAIL if bb else 0)
    w = np.ascontiguousarray(rates[0] if shared else rates, np.float32)
    bufs = dict(a=DeviceBuffer(na), b=DeviceBuffer(nb) if nb else None, pal=DeviceBuffer.from_numpy(pals),
                w=DeviceBuffer.from_numpy(w if w.size else np.zeros(1, np.float32)), bnd=DeviceBuffer((ni + 2) * 24) if bounds else None)
    try:
        for k in ("a", "b", "bnd"):
            if bufs[k] is not None:
                bufs[k].memset(0xFF)
        fl = flags | DEV | (api.WEIGHTS_SHARED if shared else 0)
        args = (ni, bufs["w"].ptr, bufs["pal"].ptr, bufs["a"].ptr, bufs["b"].ptr if bufs["b"] else None, layout, fl, scale, pitch,
                bufs["bnd"].ptr if bounds else None)
        if ids is None:
            dm.deform_batched_raw(*args)
        elif host_list:
            dm.deform_batched_select(ni, ids, *args[1:])
        else:
            bufs["ids"] = DeviceBuffer.from_numpy(ids)
            bufs["cnt"] = DeviceBuffer.from_numpy(np.array([row.count], np.uint32))
            dm.deform_batched_raw(*args, select_ptr=bufs["ids"].ptr, select_count_ptr=bufs["cnt"].ptr, n_select=len(ids))
        dm.sync()
        return (bufs["a"].download((na,), np.uint8), bufs["b"].download((nb,), np.uint8) if nb else None,
                bufs["bnd"].download((ni + 2, 6), np.uint32) if bounds else None)
    finally:
        for x in bufs.values():
            if x is not None:
                x.free()


def check_shape(dm, row, layout, f16, bounds, select, ilv, n_work, write_through=False):
    """The call that just returned ran the row's shape (mmdx_debug_last_launch_shape); returns the census tuple."""
    s = dm.last_launch_shape()
    want = dict(kernel="deform", threads=row.threads, group=row.group, ngroups=(n_work + row.group - 1) // row.group,
                morph=row.morph, layout=layout, f16=int(f16), tile_order=int(row.tile_order), bounds=int(bounds), select=int(select),
                write_through=int(write_through), interleave=ilv, sel_interleave=ilv if select else 0)
    assert {k: s[k] for k in want} == want, (row.name, s)
    assert 0 < s["lds"] <= 160 * 1024
    return (s["threads"], s["layout"], s["morph"], s["f16"], s["tile_order"], s["write_through"], s["bounds"], s["select"])


def verify(exp, out, row, layout, nv, pitch, pals, rates, shared, scale, listed, what):
    """Listed instances: the oracle's bytes, both arrays, and (bounds call) min / max over those bytes' positions, exactly.
    Everything else -- unlisted instances, their bounds rows, the rows behind the last instance, every pitch gap, the tails --
    still the 0xFF sentinel."""
    a, b, bnd = out
    ni, rows_v = row.ni, pitch or nv
    listed = set(range(ni)) if listed is None else set(listed)
    want = {i: exp.rows(layout, rates[0] if shared else rates[i], pals[i], scale) for i in listed}
    for k, buf in enumerate((a, b)):
        bpv = BPV[layout][k]
        if not bpv:
            assert buf is None
            continue
        span = ni * rows_v * bpv
        assert buf.size == span + TAIL
        body = buf[:span].reshape(ni, rows_v * bpv)
        for i in range(ni):
            got = body[i, :nv * bpv]
            if i in listed:
                if not np.array_equal(got, want[i][k]):
                    bad = np.flatnonzero(got != want[i][k])
                    raise AssertionError(f"{what}: out_{'ab'[k]} instance {i}: {bad.size} of {got.size} bytes differ from the oracle, "
                                         f"first at vertex {bad[0] // bpv}")
            else:
                assert (got == 0xFF).all(), f"{what}: out_{'ab'[k]}: unlisted instance {i} written"
        assert (body[:, nv * bpv:] == 0xFF).all(), f"{what}: out_{'ab'[k]}: a pitch gap was written"
        assert (buf[span:] == 0xFF).all(), f"{what}: out_{'ab'[k]}: bytes behind the last instance written"
    if bnd is not None:
        assert (bnd[ni:] == 0xFFFFFFFF).all(), f"{what}: bounds rows behind the last instance written"
        for i in range(ni):
            if i in listed:
                p = positions(want[i][0], layout, nv)
                w6 = np.concatenate([p.min(axis=0), p.max(axis=0)])
                assert np.array_equal(bnd[i].view(np.float32), w6), f"{what}: bounds of instance {i}: {bnd[i].view(np.float32)} != {w6}"
            else:
                assert (bnd[i] == 0xFFFFFFFF).all(), f"{what}: bounds row of unlisted instance {i} written"


def poisoned(pals, rates, shared, listed):
    """Palettes and per-instance rates of unlisted instances filled with NaN."""
    unl = np.setdiff1d(np.arange(pals.shape[0]), np.array(sorted(listed), np.int64))
    gp = pals.copy()
    gp[unl] = np.nan
    gr = rates
    if not shared and rates.size:
        gr = rates.copy()
        gr[unl] = np.nan
    return gp, gr


def env_of(row, ilv, group=None):
    return dict(MMDX_GROUP=row.group if group is None else group, MMDX_THREADS=row.threads,
                MMDX_SHARED_FUSED={SHARED: 0, FUSED1: 2}.get(row.morph), MMDX_INTERLEAVE=ilv, MMDX_SELECT_INTERLEAVE=ilv,
                MMDX_STORE_WT=None, MMDX_LDS_TARGET=None, MMDX_FUSED_PACK=None)


def pitches(dm, layout):
    """dense, mmdx_model_output_pitch's pitch (every instance 64-byte aligned), and a pitch that starts instances off 16-byte
    boundaries"""
    return (0, dm.output_pitch(layout), dm.nv + 13)


CENSUS = {}         # (threads, morph, tile_order, ilv) -> census tuples of the calls it made


def run_row(models, crowd_env, row, ilv):
    """Every flavour of one row: 3 layouts x {plain, bounds, select, select + bounds}; the plain call dense and with both
    pitches, the others with one of the three in turn; the select list once more as a host list without its bad id."""
    key = (row.threads, row.morph, row.tile_order, ilv)
    if key in CENSUS:
        return CENSUS[key]
    crowd_env(**env_of(row, ilv))
    seen = set()
    ids, listed = select_list(row)
    for li, (layout, f16) in enumerate(LAYOUTS):
        dm, exp = models.get(row.nv, row.morph != NONE, f16, row.tile_order)
        pals, rates, shared = crowd_inputs(exp.m, row.ni, row.morph)
        scale = 0.1 if layout == api.OUT_VERTEX32 else 1.0
        kinds = pitches(dm, layout)
        turn = li + (row.threads == 512) + 2 * ilv
        for fi, (bounds, select) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            for pitch in (kinds if fi == 0 else (kinds[(turn + fi) % 3],)):
                what = f"{row.name} ilv={ilv} layout={layout} bounds={bounds} select={select} pitch={pitch}"
                if not select:
                    out = run(dm, row, layout, pals, rates, shared, pitch, scale, bounds)
                    seen.add(check_shape(dm, row, layout, f16, bounds, False, ilv, row.ni))
                    verify(exp, out, row, layout, dm.nv, pitch, pals, rates, shared, scale, None, what)
                    continue
                gp, gr = poisoned(pals, rates, shared, listed)
                out = run(dm, row, layout, gp, gr, shared, pitch, scale, bounds, ids=ids)
                seen.add(check_shape(dm, row, layout, f16, bounds, True, ilv, row.n_ids))
                verify(exp, out, row, layout, dm.nv, pitch, pals, rates, shared, scale, listed, what)
                if not bounds:
                    host = np.delete(ids[:row.count], BAD_POS[row.n_ids])
                    again = run(dm, row, layout, gp, gr, shared, pitch, scale, bounds, ids=host, host_list=True)
                    check_shape(dm, row, layout, f16, bounds, True, ilv, len(host))
                    assert np.array_equal(out[0], again[0]) and (out[1] is None or np.array_equal(out[1], again[1])), \
                        f"{what}: the host list without the bad id wrote other bytes"
    CENSUS[key] = seen
    return seen


def run_write_through(models, crowd_env, morph, ilv):
    """The two write-through kernels at their cap of 8 instances per workgroup: by the caller's hint and by MMDX_STORE_WT=1."""
    key = ("wt", morph, ilv)
    if key in CENSUS:
        return CENSUS[key]
    row = WT_ROW[morph]
    dm, exp = models.get(row.nv, morph != NONE)
    pals, rates, shared = crowd_inputs(exp.m, row.ni, morph)
    seen = set()
    for how, env, flags in (("hint", {}, api.OUT_STORES_WRITE_THROUGH), ("MMDX_STORE_WT", dict(MMDX_STORE_WT=1), 0)):
        crowd_env(**dict(env_of(row, ilv), **env))
        for pitch in pitches(dm, api.OUT_SOA):
            out = run(dm, row, api.OUT_SOA, pals, rates, shared, pitch, 1.0, False, flags=flags)
            seen.add(check_shape(dm, row, api.OUT_SOA, False, False, False, ilv, row.ni, write_through=True))
            verify(exp, out, row, api.OUT_SOA, dm.nv, pitch, pals, rates, shared, 1.0, None, f"{row.name} {how} ilv={ilv} pitch={pitch}")
    CENSUS[key] = seen
    return seen


ROW_PARAMS = [(t, m, o, ilv) for ilv in (1, 0) for t in (256, 512) for m in (NONE, SHARED, FUSED1, FUSED4) for o in (False, True)
              if ilv or m != FUSED4]          # (per-instance weights are always dealt blocked: nothing to run a second time)
ROW_IDS = [f"{MORPH_NAMES[m]}-{t}-{'tile' if o else 'file'}-{'interleaved' if ilv else 'blocked'}" for t, m, o, ilv in ROW_PARAMS]


# ---- GPU: (a) every instantiation with a real group, (b) both mappings, (c) dense and pitched, (d) bounds, (e) select ----------------
@pytest.mark.gpu
@pytest.mark.parametrize("threads,morph,tile_order,ilv", ROW_PARAMS, ids=ROW_IDS)
def test_grouped_rows_bit_exact_against_the_oracle(models, crowd_env, threads, morph, tile_order, ilv):
    """One table row under one instance mapping (MMDX_INTERLEAVE = MMDX_SELECT_INTERLEAVE = ilv): SoA, 32-byte vertices (pos_scale
    0.1) and f16 positions; plain, bounds, select and select + bounds; dense, pitched and unaligned-pitched.  All instances, both
    arrays, byte for byte against the oracle; gaps, tails, unlisted instances and their bounds rows keep the sentinel; unlisted
    palettes and rates are NaN; the shape getter confirms kernel, threads, group, ngroups and flavour after every call."""
    seen = run_row(models, crowd_env, ROW[threads, morph, tile_order], ilv)
    assert len(seen) == 12


@pytest.mark.gpu
@pytest.mark.parametrize("ilv", [1, 0], ids=["interleaved", "blocked"])
@pytest.mark.parametrize("morph", [NONE, SHARED], ids=["none", "shared-pass"])
def test_write_through_rows_bit_exact_against_the_oracle(models, crowd_env, morph, ilv):
    assert len(run_write_through(models, crowd_env, morph, ilv)) == 1


@pytest.mark.gpu
def test_census_every_deform_instantiation_ran_with_a_real_group(models, crowd_env):
    """The (threads, layout, morph, f16, tile_order, write_through, bounds, select) read back from the library over the rows equal
    for_each_deform_variant's 194, none missing, none extra: an instantiation added later without a row here fails this test.
    (Rows that already ran in this session are not run again.)"""
    seen = set()
    for t, m, o, ilv in ROW_PARAMS:
        if ilv:
            seen |= run_row(models, crowd_env, ROW[t, m, o], 1)
    for m in (NONE, SHARED):
        seen |= run_write_through(models, crowd_env, m, 1)
    want = expected_variants()
    assert seen == want, f"missing {sorted(want - seen)} extra {sorted(seen - want)}"
    assert len(seen) == 194


@pytest.mark.gpu
@pytest.mark.parametrize("row", TAIL1_ROWS, ids=[r.name for r in TAIL1_ROWS])
def test_last_workgroup_with_one_instance(models, crowd_env, row):
    """Blocked 4, 4, 4, 1 (per-instance weights: a last pack of one instance); interleaved 4, 3, 3, 3."""
    ids, listed = select_list(row)
    for ilv in ((1, 0) if row.morph != FUSED4 else (1,)):
        crowd_env(**env_of(row, ilv))
        for layout, f16 in LAYOUTS:
            dm, exp = models.get(row.nv, row.morph != NONE, f16, row.tile_order)
            pals, rates, shared = crowd_inputs(exp.m, row.ni, row.morph)
            scale = 0.1 if layout == api.OUT_VERTEX32 else 1.0
            out = run(dm, row, layout, pals, rates, shared, 0, scale, True)
            check_shape(dm, row, layout, f16, True, False, ilv, row.ni)
            verify(exp, out, row, layout, dm.nv, 0, pals, rates, shared, scale, None, f"{row.name} ilv={ilv} layout={layout}")
            gp, gr = poisoned(pals, rates, shared, listed)
            out = run(dm, row, layout, gp, gr, shared, dm.nv + 13, scale, True, ids=ids)
            check_shape(dm, row, layout, f16, True, True, ilv, row.n_ids)
            verify(exp, out, row, layout, dm.nv, dm.nv + 13, pals, rates, shared, scale, listed, f"{row.name} ilv={ilv} layout={layout} select")


# ---- GPU: (f) grouping never changes a value, fast math included -------------------------------------------------------------------
def within_fast_math_tolerance(out, exp, row, layout, nv, pals, rates, shared, scale):
    """include/mmdx.h, MMDX_CREATE_FAST_MATH: |x - x_ref| <= 1e-5 (1 + |x_ref|) per position component (pos_scale scales the 1),
    2e-6 per normal component, binary16 positions within that plus one binary16 ulp (at most 2^-10 |x|, 2^-24 for subnormals)."""
    ba, bb = BPV[layout]
    for i in range(row.ni):
        wa, wb = exp.rows(layout, rates[0] if shared else rates[i], pals[i], scale)
        ga = out[0][i * nv * ba:(i + 1) * nv * ba]
        ref = positions(wa, layout, nv).astype(np.float64)
        tol = 1e-5 * (scale + np.abs(ref))
        if layout == api.OUT_SOA_POS16:
            tol = tol + np.abs(ref) * 2.0 ** -10 + 2.0 ** -24
        assert np.all(np.abs(positions(ga, layout, nv).astype(np.float64) - ref) <= tol), f"positions of instance {i}"
        if layout == api.OUT_VERTEX32:
            gn, rn = ga.view(np.float32).reshape(nv, 8)[:, 3:6], wa.view(np.float32).reshape(nv, 8)[:, 3:6]
            assert np.array_equal(ga.view(np.uint32).reshape(nv, 8)[:, 6:], wa.view(np.uint32).reshape(nv, 8)[:, 6:]), f"uv of instance {i}"
        else:
            gn, rn = out[1][i * nv * bb:(i + 1) * nv * bb].view(np.float32), wb.view(np.float32)
        assert np.all(np.abs(gn.astype(np.float64) - rn) <= 2e-6), f"normals of instance {i}"


@pytest.mark.gpu
@pytest.mark.parametrize("morph", [NONE, SHARED, FUSED1, FUSED4], ids=[MORPH_NAMES[m] for m in (NONE, SHARED, FUSED1, FUSED4)])
def test_fast_math_grouped_equals_ungrouped(models, crowd_env, morph):
    """MMDX_CREATE_FAST_MATH models run the second code object (kernels_fast.hip).  One row per layout x morph mode at the forced
    group and again with MMDX_GROUP=1: bit-identical to each other, and the grouped run within the fast-math tolerance."""
    row = ROW[256, morph, False]
    one = row._replace(group=gmin_of(row))
    for layout, f16 in LAYOUTS:
        dm, exp = models.get(row.nv, morph != NONE, f16, False, fast=True)
        pals, rates, shared = crowd_inputs(exp.m, row.ni, morph)
        scale = 0.1 if layout == api.OUT_VERTEX32 else 1.0
        crowd_env(**env_of(row, 1))
        grouped = run(dm, row, layout, pals, rates, shared, 0, scale, False)
        check_shape(dm, row, layout, f16, False, False, 1, row.ni)
        crowd_env(**env_of(row, 1, group=1))
        alone = run(dm, row, layout, pals, rates, shared, 0, scale, False)
        check_shape(dm, one, layout, f16, False, False, 1, row.ni)
        assert np.array_equal(grouped[0], alone[0]), f"layout={layout}: out_a differs between group {row.group} and MMDX_GROUP=1"
        assert grouped[1] is None or np.array_equal(grouped[1], alone[1]), f"layout={layout}: out_b differs"
        within_fast_math_tolerance(grouped, exp, row, layout, dm.nv, pals, rates, shared, scale)


# ---- GPU: (g) one unforced row -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_group_the_planner_picks_by_itself(_gpu, oracle, crowd_env):
    """The smallest crowd that gets a group without MMDX_GROUP (test_smallest_crowd_the_planner_groups_by_itself): 683 tiles x 9
    instances, shared rates through the separate morph pass, SoA, dense (NV % 4 = 1: most instances start off 16-byte
    boundaries).  The getter shows group 4, three workgroups per tile; every instance is compared with the oracle."""
    crowd_env(**dict.fromkeys(("MMDX_GROUP", "MMDX_THREADS", "MMDX_SHARED_FUSED", "MMDX_INTERLEAVE", "MMDX_SELECT_INTERLEAVE",
                               "MMDX_STORE_WT", "MMDX_LDS_TARGET", "MMDX_FUSED_PACK")))
    m = make_flat(UNFORCED_NV, True)
    row = Row("unforced", UNFORCED_NV, UNFORCED_NI, UNFORCED_GROUP, 256, SHARED, False, False, 0, 0)
    pals, rates, shared = crowd_inputs(m, row.ni, SHARED)
    exp = Expect(oracle, m)
    with DeformModel(m) as dm:
        out = run(dm, row, api.OUT_SOA, pals, rates, shared, 0, 1.0, False)
        check_shape(dm, row, api.OUT_SOA, False, False, False, 1, row.ni)
        verify(exp, out, row, api.OUT_SOA, dm.nv, 0, pals, rates, shared, 1.0, None, "unforced 683 tiles x 9")
