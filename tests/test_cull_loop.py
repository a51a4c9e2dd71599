"""The GPU-resident crowd loop end to end, recorded once and replayed: mmdx_cull_bounds turns the boxes of a bounds call into two
LOD lists in device memory (a device view, rewritten between replays), and one mmdx_deform_batched_select call per list deforms
exactly the listed instances -- no read-back anywhere in the loop, every call on the handle's one stream.
Checked after every replay: the lists equal the numpy restatement (tests/test_cull_bounds.py) applied to the bounds read back,
listed instances carry the plain call's bytes, everything else keeps its sentinel."""
import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count, planes_from_matrix
from tests.test_cull_bounds import F, SENT, View, look_at, mat_mul, perspective

DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
NI, NV, SPACING = 24, 300, 12.0


def crowd_palettes(m):
    """Every instance in its own pose, spread along x through the translation row of its bone matrices."""
    pals = synth.make_palettes(m, np.arange(NI) * 5 + 2).copy()
    pals[:, :, 12] += ((np.arange(NI) - NI / 2) * SPACING).astype(F)[:, None]
    return pals


def loop_views():
    """(what, view): a camera that sees part of the crowd with the LOD ring through it; everything culled; everything visible."""
    eye = (-40.0, 10.0, 80.0)
    cam = mat_mul(perspective(50.0, 1.0, 0.1, 1000.0), look_at(eye, (-40.0, 10.0, 0.0)))
    lod = (82.0, 0.0, 0.0)
    return [("frustum moved", View(planes_from_matrix(cam, True), 6, 2, eye, 1.0, lod)),
            ("everything culled", View([[0, 0, 0, -1]], 1, 2, eye, 0.0, lod)),
            ("everything visible", View([], 0, 2, eye, 0.0, lod))]


@pytest.mark.gpu
def test_recorded_bounds_cull_select_loop(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    m = synth.make_model(NV, 6, 0, 0, seed=7300)
    pals = crowd_palettes(m)
    views = loop_views()
    with DeformModel(m) as dm:
        na, nb = dm.out_sizes(api.OUT_SOA, NI)
        d_pal = DeviceBuffer.from_numpy(pals)
        d_bnd = DeviceBuffer(NI * 24)
        plain = [DeviceBuffer(na), DeviceBuffer(nb)]
        lod_out = [[DeviceBuffer(na), DeviceBuffer(nb)] for _ in range(2)]         # what list 0 / list 1 deform into
        d_ids = DeviceBuffer(2 * NI * 4)
        d_cnt = DeviceBuffer(4 * 4)
        d_lvl = DeviceBuffer(NI * 4)
        d_view = DeviceBuffer.from_numpy(np.frombuffer(bytes(views[0][1].struct()), np.uint8))

        # 1. the plain bounds call: every instance's bytes and box
        dm.deform_batched_raw(NI, None, d_pal.ptr, plain[0].ptr, plain[1].ptr, api.OUT_SOA, DEV, bounds_ptr=d_bnd.ptr)
        dm.sync()
        want = [plain[0].download((NI, NV * 12), np.uint8), plain[1].download((NI, NV * 12), np.uint8)]
        bounds = d_bnd.download((NI, 6), F)
        assert np.isfinite(bounds).all() and bounds[-1, 0] - bounds[0, 0] > (NI - 2) * SPACING      # spread along x

        def frame():
            dm.cull_bounds(d_bnd, d_view, NI, d_ids, d_cnt, d_lvl)
            for l in range(2):
                dm.deform_batched_raw(NI, None, d_pal.ptr, lod_out[l][0].ptr, lod_out[l][1].ptr, api.OUT_SOA, DEV,
                                      select_ptr=d_ids.ptr + 4 * l * NI, select_count_ptr=d_cnt.ptr + 4 * l, n_select=NI)

        # 2. once un-recorded (sizes the handle's scratch), then recorded into one graph
        frame()
        dm.sync()
        dm.graph_begin()
        frame()
        graph = dm.graph_end()

        # 3. three replays, the view rewritten in place between them
        seen = []
        for what, view in views:
            d_view.upload(np.frombuffer(bytes(view.struct()), np.uint8))
            for pair in lod_out:
                for buf in pair:
                    buf.memset(0xFF)
            d_ids.upload(np.full(2 * NI, SENT, np.uint32))
            d_cnt.upload(np.full(4, SENT, np.uint32))
            d_lvl.upload(np.full(NI, SENT, np.uint32))
            graph.launch()
            dm.sync()
            lists, levels = view.ref(bounds, True)
            ids, cnt, lvl = d_ids.download((2, NI), np.uint32), d_cnt.download((4,), np.uint32), d_lvl.download((NI,), np.uint32)
            assert cnt.tolist() == [len(lists[0]), len(lists[1]), 0, 0], what
            assert np.array_equal(lvl, levels), what
            for l in range(2):
                assert np.array_equal(ids[l, :cnt[l]], lists[l]), what
                assert (ids[l, cnt[l]:] == SENT).all(), what
                listed = np.zeros(NI, bool)
                listed[lists[l]] = True
                for k in range(2):
                    got = lod_out[l][k].download((NI, NV * 12), np.uint8)
                    assert np.array_equal(got[listed], want[k][listed]), f"{what}: list {l}: listed instances differ from the plain call"
                    assert (got[~listed] == 0xFF).all(), f"{what}: list {l}: an unlisted instance was written"
            seen.append([len(lists[0]), len(lists[1]), int((levels == api.CULLED).sum())])
        # the three frames are the three cases: a real split, nothing, everything
        assert min(seen[0]) > 0 and seen[1] == [0, 0, NI] and seen[2][2] == 0 and seen[2][0] + seen[2][1] == NI and min(seen[2][:2]) > 0, seen
        graph.close()
        for buf in [d_pal, d_bnd, d_ids, d_cnt, d_lvl, d_view] + plain + lod_out[0] + lod_out[1]:
            buf.free()
