"""Generate tests/golden/morph_plan_sequences.json: what a library does with the scripted call sequences of tests/morph_plan_seq.py
-- after every step the morph mode and the kernel kind of mmdx_debug_last_launch_shape and the (walks, device skips, host skips) of
mmdx_debug_morph_pass_stats, or "refused".  Needs a GPU.  The committed file was recorded from the library of the commit BEFORE the
morph step was split into plan_morph_pass and its executor (MMDX_LIB names the library to load):
    MMDX_LIB=<that build's libmmdx.so> python -m tests.gen_morph_plan_golden
Every sequence's last outputs are checked against the oracle here too, so that no wrong behaviour is pinned."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyoracle import Oracle  # noqa: E402
from simple_mmd_renderer_amd import _capi as api  # noqa: E402
from simple_mmd_renderer_amd import build  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests import morph_plan_seq as mps  # noqa: E402

FIXTURE = os.path.join(gu.GOLDEN_DIR, "morph_plan_sequences.json")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    orc = Oracle()
    seqs = []
    for seq in mps.SEQUENCES:
        rows, final = mps.run(seq)
        mps.check_final(orc, final, seq["name"])
        seqs.append(dict(seq, expect=rows))
        print("%-70s %2d steps, stats %s" % (seq["name"], len(rows), rows[-1]["stats"]))
    doc = dict(library_source_sha=build.library_sha(api.LIB_PATH),
               models={k: dict(v, **mps.model_scalars(k)) for k, v in mps.MODELS.items()})
    with open(out, "w") as f:
        f.write("{\n\"library_source_sha\": %s,\n\"models\": %s,\n\"sequences\": [\n" % (json.dumps(doc["library_source_sha"]),
                                                                                   json.dumps(doc["models"])))
        for k, s in enumerate(seqs):
            f.write("{\"name\": %s, \"model\": %s, \"env\": %s,\n \"steps\": [\n  %s],\n \"expect\": [\n  %s]}%s\n" % (
                json.dumps(s["name"]), json.dumps(s["model"]), json.dumps(s["env"]), ",\n  ".join(json.dumps(x) for x in s["steps"]),
                ",\n  ".join(json.dumps(x) for x in s["expect"]), "," if k + 1 < len(seqs) else ""))
        f.write("]}\n")
    json.load(open(out))
    print("%s: %d sequences, %d steps, %.1f KB" % (os.path.basename(out), len(seqs), sum(len(s["steps"]) for s in seqs),
                                                    os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
