"""Generate tests/golden/seam_fix_classes.json and tests/golden/seam_fix_expect.npz for tests/test_seam_fix.py.

seam_fix_classes.json   "required": the classes of inverse (tests/seam_cases.classify) that the crowd must contain -- written down
                        here by hand, from what the kernel's inverse can do, NOT from what the crowd happens to hold;
                        "min_zero_last_pivot_orders": the zero last pivot must be reached after that many different pivot orders;
                        "histogram": per override list, how many inversions of the crowd fall into each class (the oracle's trace).
seam_fix_expect.npz     libmmd's own palettes of the crowd under every override list (expected outputs only; the inputs are
                        rebuilt by tests/seam_cases.py).  Needs the reference build (oracle/_ref):
    python -m tests.gen_seam_fix_golden
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyoracle import Oracle  # noqa: E402
from tests import seam_cases as sc  # noqa: E402


def required_classes():
    req = ["inverted/" + "".join(map(str, o)) for o in sc.ORDERS]
    req += ["zero_row/%d" % r for r in range(4)] + ["zero_row/negative_zero"]
    req += ["tie/column%d" % c for c in range(3)] + ["zero_pivot/column%d" % c for c in range(3)]
    req += ["input/nan", "input/inf", "input/denormal", "input/huge_overflows", "input/rigid",
            "mixed_scale/scaled_pivot_differs_from_plain"]
    return req


def main():
    doc = dict(required=required_classes(), min_zero_last_pivot_orders=4, histogram=sc.histogram(Oracle()))
    with open(sc.CLASSES, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(sc.EXPECT, **{name: sc.reference_palettes(name) for name in sc.LISTS})
    print(f"{os.path.basename(sc.CLASSES)}: {len(doc['required'])} required classes; "
          f"{os.path.basename(sc.EXPECT)}: {os.path.getsize(sc.EXPECT)} bytes, {len(sc.LISTS)} lists x {sc.NI} instances")


if __name__ == "__main__":
    main()
