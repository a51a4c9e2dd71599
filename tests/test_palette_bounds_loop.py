"""The same-frame crowd loop, recorded once and replayed: mmdx_palette_place -> mmdx_palette_bounds -> mmdx_cull_bounds ->
mmdx_deform_batched_select (no out_bounds), everything in device memory on the handle's one stream.  The boxes the cull tests are
this frame's, made from the palette the deform is about to read: no bounds call of the deform kernel anywhere, no margin.
Checked after every replay: the lists equal the numpy restatement of the cull (tests/test_cull_bounds.py) applied to the numpy
restatement of the boxes (tests/palette_bounds_ref.py); listed instances carry the plain call's bytes; everything else keeps its
sentinel; and an instance that was culled in one replay and stands inside the view in the next is listed there."""
import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count, planes_from_matrix
from tests import golden_util as gu
from tests import palette_bounds_ref as pb
from tests import palette_place_ref as pp
from tests.test_cull_bounds import F, SENT, View, cull_ref, look_at, mat_mul, perspective

DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
PLACE_DEV = DEV | api.PLACE_ON_DEVICE
NI, SHAPE, SPACING, LOD = 64, (3000, 40, 8, 64), 12.0, (66.0, 0.0, 0.0)
NV = SHAPE[0]


def placements(shift):
    """Pose form: instance i at x = (i - NI/2) * SPACING + shift, turned about y a little more with every instance."""
    p = np.zeros((NI, 8), F)
    p[:, 0] = (np.arange(NI) - NI / 2) * SPACING + shift
    yaw = 0.05 + 0.03 * np.arange(NI)
    p[:, 5], p[:, 7] = np.sin(yaw / 2), np.cos(yaw / 2)
    return p


def camera(x, fov=50.0):
    """A camera 80 in front of x that sees a handful of instances, the LOD ring (66 from the eye) through them; margin 0."""
    eye = (x, 10.0, 80.0)
    cam = mat_mul(perspective(fov, 1.0, 0.1, 1000.0), look_at(eye, (x, 10.0, 0.0)))
    return View(planes_from_matrix(cam, True), 6, 2, eye, 0.0, LOD)


@pytest.mark.gpu
def test_recorded_place_palette_bounds_cull_select_loop(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    m = synth.make_model(*SHAPE, seed=7400)
    model_space = synth.make_palettes(m, np.arange(NI) * 5 + 2).copy()
    rates = synth.morph_weights(m.nm, np.arange(NI) * 3)
    frames = [(placements(0.0), camera(-40.0)), (placements(150.0), camera(-40.0)), (placements(0.0), camera(95.0, 35.0)),
              (placements(150.0), camera(95.0, 35.0))]
    with DeformModel(m) as dm:
        table = dm.bone_boxes()
        na, nb = dm.out_sizes(api.OUT_SOA, NI)
        d_model, d_rates = DeviceBuffer.from_numpy(model_space), DeviceBuffer.from_numpy(rates)
        d_place, d_pal, d_bnd = DeviceBuffer(NI * 32), DeviceBuffer(model_space.nbytes), DeviceBuffer(NI * 24)
        plain = [DeviceBuffer(na), DeviceBuffer(nb)]
        lod_out = [[DeviceBuffer(na), DeviceBuffer(nb)] for _ in range(2)]
        d_ids, d_cnt, d_lvl = DeviceBuffer(2 * NI * 4), DeviceBuffer(4 * 4), DeviceBuffer(NI * 4)
        d_view = DeviceBuffer.from_numpy(np.frombuffer(bytes(frames[0][1].struct()), np.uint8))
        flags = DEV | api.WEIGHTS_ON_DEVICE

        def frame():
            dm.place_palettes(NI, d_model.ptr, d_place.ptr, d_pal.ptr, PLACE_DEV)
            dm.palette_bounds_raw(NI, d_pal.ptr, d_bnd.ptr, DEV, 1.0, 1.0)
            dm.cull_bounds(d_bnd, d_view, NI, d_ids, d_cnt, d_lvl)
            for l in range(2):
                dm.deform_batched_raw(NI, d_rates.ptr, d_pal.ptr, lod_out[l][0].ptr, lod_out[l][1].ptr, api.OUT_SOA, flags,
                                      select_ptr=d_ids.ptr + 4 * l * NI, select_count_ptr=d_cnt.ptr + 4 * l, n_select=NI)

        # what every instance looks like when it is deformed, per placement array: the plain call on the placed palettes
        want = {}
        for pl, _ in frames:
            if pl.tobytes() in want:
                continue
            placed = pp.place_crowd(model_space, pl, False)
            d_placed = DeviceBuffer.from_numpy(placed)
            dm.deform_batched_raw(NI, d_rates.ptr, d_placed.ptr, plain[0].ptr, plain[1].ptr, api.OUT_SOA, flags)
            dm.sync()
            pos = plain[0].download((NI, NV, 3), F)
            want[pl.tobytes()] = (placed, [plain[0].download((NI, NV * 12), np.uint8), plain[1].download((NI, NV * 12), np.uint8)],
                                  np.concatenate([pos.min(axis=1), pos.max(axis=1)], axis=1))
            d_placed.free()

        # once un-recorded (sizes the handle's scratch), then recorded into one graph
        d_place.upload(frames[0][0])
        frame()
        dm.sync()
        dm.graph_begin()
        frame()
        graph = dm.graph_end()

        culled_before, reentered, seen = None, 0, []
        for k, (pl, view) in enumerate(frames):
            what = "replay %d" % k
            d_place.upload(pl)
            d_view.upload(np.frombuffer(bytes(view.struct()), np.uint8))
            for buf in lod_out[0] + lod_out[1] + [d_pal, d_bnd]:
                buf.memset(0xFF)
            d_ids.upload(np.full(2 * NI, SENT, np.uint32))
            d_cnt.upload(np.full(4, SENT, np.uint32))
            d_lvl.upload(np.full(NI, SENT, np.uint32))
            graph.launch()
            dm.sync()
            placed, plain_bytes, true_box = want[pl.tobytes()]
            gu.assert_bits_equal(d_pal.download(placed.shape, F), placed, what + ": placed palettes")
            boxes = pb.palette_bounds(table, placed, 1.0, 1.0)
            gu.assert_bits_equal(d_bnd.download((NI, 6), F), boxes, what + ": boxes")
            assert (boxes[:, :3] <= true_box[:, :3]).all() and (boxes[:, 3:] >= true_box[:, 3:]).all(), what
            lists, levels = view.ref(boxes, True)
            ids, cnt, lvl = d_ids.download((2, NI), np.uint32), d_cnt.download((4,), np.uint32), d_lvl.download((NI,), np.uint32)
            assert cnt.tolist() == [len(lists[0]), len(lists[1]), 0, 0], what
            assert np.array_equal(lvl, levels), what
            for l in range(2):
                assert np.array_equal(ids[l, :cnt[l]], lists[l]), what
                assert (ids[l, cnt[l]:] == SENT).all(), what
                listed = np.zeros(NI, bool)
                listed[lists[l]] = True
                for j in range(2):
                    got = lod_out[l][j].download((NI, NV * 12), np.uint8)
                    assert np.array_equal(got[listed], plain_bytes[j][listed]), f"{what}: list {l}: listed instances differ from the plain call"
                    assert (got[~listed] == 0xFF).all(), f"{what}: list {l}: an unlisted instance was written"
            culled = levels == api.CULLED
            # inside the view by its TRUE box (the vertices the plain call wrote), margin 0
            inside = cull_ref(true_box, view.planes, view.n_planes, view.n_lods, view.eye, 0.0, view.lod)[1] != api.CULLED
            assert not (inside & culled).any(), what + ": an instance in view was culled"
            if culled_before is not None:
                back = culled_before & inside
                assert not culled[back].any(), what + ": an instance that came back into view was not listed"
                reentered += int(back.sum())
            culled_before = culled
            seen.append([len(lists[0]), len(lists[1]), int(culled.sum())])
        print("lists / culled per replay:", seen, "re-entered:", reentered)
        assert all(s[0] + s[1] > 0 and s[2] > 0 for s in seen) and any(s[0] > 0 and s[1] > 0 for s in seen), seen
        assert len({tuple(s) for s in seen}) >= 2 and reentered >= 3, (seen, reentered)
        graph.close()
        for buf in [d_model, d_rates, d_place, d_pal, d_bnd, d_ids, d_cnt, d_lvl, d_view] + plain + lod_out[0] + lod_out[1]:
            buf.free()
