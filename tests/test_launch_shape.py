"""CPU: the launch planner (simple_mmd_renderer_amd/csrc/launch_shape.cpp) -- which kernel, how many threads, which group size
and LDS layout a deform call gets -- without a GPU.  tests/launch_shape_driver.cpp, built from launch_shape.cpp alone under
ASan + UBSan, (1) sweeps the planner over a cross product of calls, models and overrides and checks every shape against the
code's own rules, (2) evaluates the calls of tests/golden/launch_shapes.json, whose pinned shapes were recorded from the code
as it stood before the planner was split out: a change that moves one of them fails here, on any machine."""
import json
import os

import pytest

from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.engine import DeformModel
from tests import host_program as hp
from tests.host_program import ROOT

TABLE = os.path.join(ROOT, "tests", "golden", "launch_shapes.json")
KERNELS = ["none", "deform", "pack", "frame"]        # LaunchShape::Kernel


@pytest.fixture(scope="module")
def driver():
    # -O2: the sweep is 22 million planner calls; about 15 s under the sanitizers on an 8-core build machine
    return hp.build("launch_shape_driver", [os.path.join(hp.TESTS, "launch_shape_driver.cpp"), os.path.join(hp.CSRC, "launch_shape.cpp")],
                    sanitize=True)


def test_every_planned_shape_obeys_the_layout_rules(driver):
    r = hp.run(driver, ["sweep"], timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    counts = dict(kv.split("=") for kv in r.stdout.split())
    assert int(counts["failures"]) == 0 and "ERROR" not in r.stderr
    # the cross product: 3 layouts x 4 morph modes x tile order x bounds x 8 crowd sizes x (no list + 4 list capacities) x 6 tile
    # counts x 4 bone counts x 6 slot counts x 3 store hints x 3 output placements x 9 override sets
    assert int(counts["rows"]) == 3 * 4 * 2 * 2 * 8 * 5 * 6 * 4 * 6 * 3 * 3 * 9
    assert 0 < int(counts["rejected"]) < int(counts["rows"])


def test_pinned_launch_shapes(driver):
    table = json.load(open(TABLE))
    rows = table["rows"]
    assert 100 <= len(rows) <= 999
    stdin = "".join(" ".join(str(v) for v in row["in"]) + "\n" for row in rows)
    r = hp.run(driver, ["eval"], stdin=stdin)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    moved = []
    for row, line in zip(rows, lines):
        got = dict(kv.split("=", 1) for kv in line.split(" ")) if line.startswith("status=0 ") else {"error": line}
        if "error" not in got:
            del got["status"]
            got = {k: int(v) for k, v in got.items()}
            got["kernel"] = KERNELS[got["kernel"]]
        if got != row["shape"]:
            moved.append("%s\n    pinned  %s\n    planned %s" % (row["call"], row["shape"], got))
    assert not moved, "%d pinned launch shapes moved:\n%s" % (len(moved), "\n".join(moved))


def test_pinned_table_describes_the_synthetic_models(hip_lib):
    """The model scalars in the table are those of the synthetic BASELINE models (host-only handles: no GPU)."""
    table = json.load(open(TABLE))
    idx = {f: i for i, f in enumerate(table["fields"])}
    for mod in table["models"]:
        flat = synth.make_config(mod["name"].replace("_tile_order", "").replace("_f16", ""))
        with DeformModel(flat, host_only=True, tile_order=bool(mod["tile_order"]), f16_positions=bool(mod["f16"])) as dm:
            info = dm.info
            assert (info.n_vertices, info.n_tiles, info.max_tile_bones, info.n_slots) == (mod["nv"], mod["ntiles"], mod["max_tile_bones"],
                                                                                         mod["ns"])
        mine = [r for r in table["rows"] if r["call"].startswith(mod["name"] + " ")]
        assert mine
        for r in mine:
            assert [r["in"][idx[k]] for k in ("f16", "tile_order", "ntiles", "max_tile_bones", "ns")] == \
                   [mod["f16"], mod["tile_order"], mod["ntiles"], mod["max_tile_bones"], mod["ns"]]
