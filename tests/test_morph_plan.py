"""The morph planner (plan_morph_pass, simple_mmd_renderer_amd/csrc/launch_shape.cpp): the morph mode of a deform call, the pass in
front of its deform kernel, and what the handle remembers about the positions it keeps.

CPU: tests/morph_plan_driver.cpp, built from launch_shape.cpp alone under ASan + UBSan, (a) sweeps the planner over a cross product
of models, calls, overrides and handle records and checks every plan against the rules of launch_shape.hpp, (b) proves the records
SOUND over every short sequence of calls and replays -- the kept positions are never read for rates they were not computed from, and
MMDX_MORPH_UNCHANGED is refused exactly when the handle holds none -- against a simulated device record and a model of the truth,
(c) replays the scripted sequences of tests/golden/morph_plan_sequences.json, recorded on an MI355X from the library as it stood
before the planner was split out of api.cpp: every morph mode, kernel kind and pass counter must come out as pinned.
GPU: (d) the built library reproduces the same file line for line, and every sequence's last outputs are the oracle's bit for bit."""
import json
import os

import pytest

from tests import host_program as hp
from tests import morph_plan_seq as mps
from tests.host_program import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "morph_plan_sequences.json")
KERNELS = ["none", "deform", "pack", "frame"]        # LaunchShape::Kernel
EVENTS, SETTINGS = 15, 3 * 3 * 2                     # the driver's alphabet; (slot class, shared_fused, autoskip)
LENGTH = 6                                           # 216 million sequences: about 40 s under the sanitizers


@pytest.fixture(scope="module")
def driver():
    return hp.build("morph_plan_driver", [os.path.join(hp.TESTS, "morph_plan_driver.cpp"), os.path.join(hp.CSRC, "launch_shape.cpp")],
                    sanitize=True)


@pytest.fixture(scope="module")
def pinned():
    doc = json.load(open(FIXTURE))
    assert 24 <= len(doc["sequences"]) <= 60
    return doc


def counts_of(r):
    assert r.returncode == 0, r.stdout + r.stderr
    counts = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    assert counts["failures"] == 0 and "ERROR" not in r.stderr
    return counts


def test_every_plan_obeys_the_rules(driver):
    counts = counts_of(hp.run(driver, ["sweep"]))
    # 4 slot counts x 5 crowd sizes x shared x unchanged x host / device rates x (no list + 3 capacities) x 3 shared_fused x autoskip
    # x the record: morphed_valid x host_rates_valid x (no kept rates, the call's, others)
    assert counts["rows"] == 4 * 5 * 2 * 2 * 2 * 4 * 3 * 2 * (2 * 2 * 3)
    # refused: a crowd's MMDX_MORPH_UNCHANGED on a handle without positions, whatever else the call says
    assert counts["refusals"] == 4 * 4 * 2 * 4 * 3 * 2 * (2 * 3)


def test_the_record_is_sound_over_every_short_sequence(driver):
    counts = counts_of(hp.run(driver, ["sequences", str(LENGTH)], timeout=900))
    print(counts)
    assert counts["events"] == EVENTS and counts["settings"] == SETTINGS
    assert counts["sequences"] == SETTINGS * sum(EVENTS ** k for k in range(1, LENGTH + 1))
    assert counts["refusals"] > 0 and counts["reads"] > 0


def expected_rows(seq):
    return ["refused" if e == "refused" else "morph=%d kernel=%d walks=%d device_skips=%d host_skips=%d" % (
        e["morph"], KERNELS.index(e["kernel"]), *e["stats"]) for e in seq["expect"]]


def test_pinned_sequences(driver, pinned):
    seqs = pinned["sequences"]
    stdin = "".join(line + "\n" for s in seqs for line in mps.driver_lines(s, pinned["models"][s["model"]]))
    r = hp.run(driver, ["eval"], stdin=stdin)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == sum(len(s["steps"]) for s in seqs)
    moved = []
    for s in seqs:
        got, lines = lines[:len(s["steps"])], lines[len(s["steps"]):]
        moved += ["%s, step %d %s\n    pinned  %s\n    planned %s" % (s["name"], k, s["steps"][k], w, g)
                  for k, (g, w) in enumerate(zip(got, expected_rows(s))) if g != w]
    assert not moved, "%d pinned steps moved:\n%s" % (len(moved), "\n".join(moved))


def test_pinned_file_holds_the_scripted_sequences(pinned, hip_lib):
    """The file's sequences are those of tests/morph_plan_seq.py, its model scalars those of the synthetic models (host-only handles)."""
    assert [{k: s[k] for k in ("name", "model", "env", "steps")} for s in pinned["sequences"]] == json.loads(json.dumps(mps.SEQUENCES))
    for name, spec in mps.MODELS.items():
        assert pinned["models"][name] == dict(spec, **mps.model_scalars(name))
    assert pinned["models"]["small"]["ns"] <= 8192 < pinned["models"]["big"]["ns"]
    covered = {(s["model"], s["env"].get("MMDX_SHARED_FUSED", "1"), s["env"].get("MMDX_MORPH_AUTOSKIP", "1")) for s in pinned["sequences"]}
    assert {("small", "0", "1"), ("small", "2", "1"), ("small", "1", "0"), ("big", "1", "1"), ("small_f16", "1", "1")} <= covered
    steps = [st for s in pinned["sequences"] for st in s["steps"]]
    assert {8, 9} <= {st["ni"] for st in steps if st["op"] == "call"} and any(st["op"] == "replay" for st in steps)
    assert {(st["shared"], st["sel"] == 0) for st in steps if st["op"] == "call" and st["sel"] >= 0} == {(a, b) for a in (False, True)
                                                                                                      for b in (False, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(mps.SEQUENCES)), ids=lambda i: mps.SEQUENCES[i]["name"].replace(" ", "_"))
def test_library_reproduces_the_pinned_sequence(index, pinned, oracle, hip_lib):
    seq = pinned["sequences"][index]
    assert seq["name"] == mps.SEQUENCES[index]["name"]
    rows, final = mps.run(seq)
    moved = ["step %d %s\n    pinned  %s\n    library %s" % (k, seq["steps"][k], w, g)
             for k, (g, w) in enumerate(zip(rows, seq["expect"])) if g != w]
    assert len(rows) == len(seq["expect"]) and not moved, "%d steps moved:\n%s" % (len(moved), "\n".join(moved))
    mps.check_final(oracle, final, seq["name"])
