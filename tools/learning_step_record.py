"""Record tests/golden/learning_step_parent.npz: what gnnb_online_step, gnnb_online_step_rows and gnnb_imitation_step_rows compute on the
cases of tests/test_gpu_learning_step_parent.py, by the library BEFORE the learning step became `struct Step` (run once, on the MI355X; the
C ABI is the same on both sides, so this tree's Python drives the parent's library):

    git worktree add <dir> <parent revision>  &&  build <dir>/gnn_branching_amd/csrc/libgnnb.so there
    GNNB_LIB=<dir>/gnn_branching_amd/csrc/libgnnb.so python tools/learning_step_record.py [out.npz]

Per case the digests of its inputs are recorded beside the results, and the recorded library's gnnb_build_id() once; the test asserts the
digests first."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import test_gpu_learning_step_parent as T              # noqa: E402


def main():
    from gnn_branching_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {T.BUILD_ID_KEY: np.array(_lib.load().gnnb_build_id().decode())}
    for case in T.CASES:
        for what, d in T.input_digests(case).items():
            rec[f"{case}/inputs/{what}"] = np.array(d)
        run = T.run_case(case)
        again = T.run_case(case)
        assert all(T.same_bits(run[k], again[k]) for k in run), (case, "two runs of the recorded library differ")
        for k, v in run.items():
            rec[f"{case}/{k}"] = v
        print(f"{case}: " + ", ".join(f"{k} {np.asarray(v).reshape(-1)[:3].tolist()}" for k, v in run.items() if k != "scores"), flush=True)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes; library:", os.environ.get("GNNB_LIB", "in-tree"), str(rec[T.BUILD_ID_KEY]))


if __name__ == "__main__":
    main()
