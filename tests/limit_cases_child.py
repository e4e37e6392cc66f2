"""Helper of tests/test_gpu_limits.py (run as a script, its environment set by the test): the ragged list of boundary queries three times
through lx_extend_batch_list in a fresh process, the results written as an .npz; argv = out.npz."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from lambda_amd import capi
from tests import limit_cases

if __name__ == "__main__":
    q, s, ext, _ = limit_cases.case_codes_ragged_list()
    h = capi.Handle(0)
    h.set_scoring(limit_cases.blosum62(), 0)
    h.set_option(capi.LX_OPT_PASS2_MODE, 2)
    out = {}
    for k in range(3):
        score, index, hsp, off, codes = h.extend_batch_list(q, s, ext, 60)
        out.update({f"score{k}": score, f"index{k}": index, f"hsp{k}": hsp, f"off{k}": off, f"codes{k}": codes,
                    f"kernel{k}": np.array(h.last_trace_kernel_name())})
    np.savez(sys.argv[1], **out)
    h.close()
