"""The C restatement of the oracle as the GPU tests call it (shared by test modules; not a conftest)."""
import numpy as np

from conftest import flat_phi

TOL = 1e-8                                  # the suite's bound on |Φ − Φ_oracle|; derivation: header of test_gpu_parity.py


def c_oracle_flat(slc, P, S, cols):
    """Φ values of the given columns from the C restatement, in mask order (zeros elsewhere) + per-column status."""
    import sls_oracle as o
    import sls_oracle_cport as cp
    Po = o.OraclePlant(P.A, P.B1, P.B2)
    ox, ou, info = cp.SLS_H2(Po, S, cols=cols, nthreads=8)
    return np.concatenate([flat_phi(ox, S[0]), flat_phi(ou, S[1])]), info
