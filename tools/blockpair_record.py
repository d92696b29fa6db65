"""Record tests/golden/blockpair_parent.npz: scores, decisions and the row signatures of layer 1 after the first forward half-pass, for the
cases of tests/test_gpu_blockpair.py, computed by the library BEFORE the fused half-pass walked edge 1 in row pairs (run once, on the GPU box):

    tools/mklib.sh <parent revision> parent
    GNNB_LIB=tools/ablate/parent.so python tools/blockpair_record.py [out.npz]

The fused and the two-kernel half-pass of that library must agree bit for bit and leave a status word of 0 (the script checks both); both
paths are recorded."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import test_gpu_blockpair as T     # noqa: E402
from tests.common import FAMILIES             # noqa: E402

WHAT = ("scores", "decisions", "row_sig")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {}
    for case in T.CASES:
        for fam in FAMILIES:
            runs = {path: T.run_case(case, fam, opts) for path, opts in T.PATHS.items()}
            for path, r in runs.items():
                assert r["status"] == 0, (case, fam, path, r["status"])
                for what in WHAT:
                    assert np.array_equal(runs["default"][what], r[what]), (case, fam, what)
                    rec[f"{case}/{fam}/{path}/{what}"] = r[what]
            fwd1 = [u for u in runs["default"]["describe"]["updates"] if u["update"] == "fwd" and u["layer"] == 1][0]
            print(f"{case} {fam}: edge 1 tile {fwd1['tile']} window {fwd1['window']} {fwd1['kernel']}, scores {runs['default']['scores'].shape}, "
                  f"decisions {runs['default']['decisions'].tolist()}")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes; library:", os.environ.get("GNNB_LIB", "in-tree"))


if __name__ == "__main__":
    main()
