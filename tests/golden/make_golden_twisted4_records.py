"""Golden fixture for tests/test_gpu_twisted4_records.py: what the four-wave twisted kernel computes on seven cases of the
test_gpu_twisted4_tilesweep.py table, to the bit — Φ (all values of the plan, zeros where the plan solves nothing), residuals,
status words and pass counts — under the default plan (plan-time static blocks) and under SLS_T4_PRESTATIC=0 (the rebuild
instantiation).

A DEVICE output, recorded on an MI355X with the library of the commit BEFORE the chain wave took its scaled pivot rows from the
published records: that change moves operands between lanes through another path and must not change one bit.  Re-record only
from a commit whose arithmetic is meant to be the new reference.

Run (needs the GPU and the built library):  python tests/golden/make_golden_twisted4_records.py
"""
import os
import sys

os.environ.setdefault("SLS_LAB", "1")                      # SLS_T4_PRESTATIC is a lab-mode knob
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import slc_amd as slc  # noqa: E402
from test_gpu_twisted4_tilesweep import CASES, FOUR, _plant, _run  # noqa: E402

RECORD_CASES = ("c10_T7", "c12_mix", "c12_top24", "c10_T17_mix", "load_path", "weighted", "four_tile")
PLANS = (("pre", None), ("rebuild", "0"))                 # key, SLS_T4_PRESTATIC


def main():
    ctx = slc.Context([0])
    out = {}
    for cid in RECORD_CASES:
        kind, d, T, alpha, cols, _, cls = CASES[cid]
        P = _plant(slc, kind)
        S = list(slc.workloads.localization_masks(P.A, P.B2, d, T, alpha))
        for key, pre in PLANS:
            os.environ.pop("SLS_T4_PRESTATIC", None)
            if pre is not None:
                os.environ["SLS_T4_PRESTATIC"] = pre
            plan = slc.Plan(ctx, P, S, [[c] for c in cols])
            try:
                desc = plan.describe()
                assert FOUR + cls in desc and desc.count(";") == 1, desc
                phi, st, rs, it = _run(plan)
            finally:
                plan.close()
            os.environ.pop("SLS_T4_PRESTATIC", None)
            out[f"{cid}/{key}/phi"] = phi
            out[f"{cid}/{key}/status"] = st
            out[f"{cid}/{key}/resid"] = rs
            out[f"{cid}/{key}/passes"] = it
            print(f"{cid} [{key}]: {desc.split(' lds=')[0]}; status {st.tolist()} passes {it.tolist()} residual {rs.max():.1e}; "
                  f"{np.count_nonzero(phi)} of {phi.size} values non-zero")
    ctx.close()
    path = os.path.join(HERE, "twisted4_records_parent.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
