"""Host twin of tests/test_gpu_closed_loop_edges.py: what the GPU tests rest on, checked without a device.

The inputs: the ladder operator of tests/closed_loop_cases.py must put a row on either side of every loop boundary of
closed_loop_step_kernel<SCN>'s `fir` lambda, for each of the seven lane layouts — asserted from the masks, so that an edit of
the ladder cannot silently drop a boundary.  The reference: the long-double dense restatement equals oracle.closed_loop
(plain FP64 sparse mat-vecs) to 1e-13·max(1, max|x|); the two differ only by double rounding in the oracle.  And the run is
bounded, so the relative tolerance of the GPU tests is not loosened by growth of the state."""
import numpy as np
import pytest

import closed_loop_cases as clc


@pytest.fixture(scope="module")
def ladder():
    return clc.ladder()


def test_ladder_has_the_prescribed_shape(ladder):
    nb, nu = clc.row_lengths(ladder.Sx, ladder.Su)
    assert tuple(nb) == clc.LADDER_BETA and tuple(nu) == clc.LADDER_U
    assert (ladder.Nx, ladder.Nu, ladder.T, ladder.steps) == (24, 6, 24, 60)
    assert ladder.n_entries == sum(clc.LADDER_BETA) + sum(clc.LADDER_U)
    assert ladder.steps > 2 * ladder.T                              # the history ramps in, then runs at full length for > T steps
    # Sx[0] is stored (the value offsets of the later slices are not trivial) and exactly one mask entry is stored false
    assert ladder.Sx[0].nnz == ladder.Nx
    stored = sum(m.nnz for m in ladder.Sx[1:]) + sum(m.nnz for m in ladder.Su)
    assert stored == ladder.n_entries + 1
    # the device value array is poisoned exactly where the operator must not read
    assert np.count_nonzero(np.isnan(ladder.values)) == ladder.Nx + 1 and len(ladder.values) == stored + ladder.Nx
    # plant: B1 = I, one actuator drives two states, one none, one state has an empty A row
    assert (abs(ladder.B1 - np.eye(ladder.Nx))).max() == 0
    per_act = np.diff(ladder.B2.indptr)
    assert per_act[clc.LADDER_SHARED] == 2 and per_act[clc.LADDER_ORPHAN] == 0 and np.count_nonzero(per_act == 0) == 1
    assert nu[clc.LADDER_ORPHAN] > 0 and nu[clc.LADDER_SHARED] > 0
    assert ladder.A.tocsr()[clc.LADDER_EMPTY_A_ROW].nnz == 0 and ladder.A.nnz > 0


@pytest.mark.parametrize("NE", clc.NES)
def test_ladder_rows_sit_on_both_sides_of_every_fir_loop_boundary(ladder, NE):
    """Lane le of NE runs the unrolled body while le + 3·NE < length and the tail for what is left: lengths 0, NE − 1, NE,
    NE + 1 (the tail's first and second trip), one in (NE, 3·NE] (tail only, several trips), one in [3·NE + 1, 4·NE] (the
    unrolled body on some lanes only), one ≥ 4·NE + 1 (unrolled body, then the tail)."""
    nb, nu = clc.row_lengths(ladder.Sx, ladder.Su)
    lengths = set(int(n) for n in nb) | set(int(n) for n in nu)
    assert 0 in lengths
    assert {NE - 1, NE, NE + 1} <= lengths
    assert any(NE < n <= 3 * NE for n in lengths)
    assert any(3 * NE + 1 <= n <= 4 * NE for n in lengths)
    assert any(n >= 4 * NE + 1 for n in lengths)


def _against_oracle(oracle, case, w):
    x, u = clc.reference(case, w)
    Phix, Phiu = clc.sparse_phi(case)
    for s in (0, w.shape[2] - 1):
        xo, uo = oracle.closed_loop(case.A, case.B1, case.B2, Phix, Phiu, steps=case.steps, w=w[:, :, s])
        tol = 1e-13 * max(1.0, np.abs(xo).max())
        assert np.abs(x[:, :, s].T - xo).max() <= tol
        assert uo.shape == (case.Nu, case.steps) and (case.Nu == 0 or np.abs(u[:, :, s].T - uo).max() <= tol)
    return x, u


def test_reference_equals_the_oracle_on_the_ladder_and_is_bounded(oracle, ladder):
    w = clc.ladder_w(5)
    x, u = _against_oracle(oracle, ladder, w)
    assert x.shape == (60, 24, 5) and u.shape == (60, 6, 5)
    assert np.abs(x).max() <= 10.0 * np.abs(w).max()
    assert np.abs(x[0]).max() == 0 and np.abs(u[-1]).max() == 0
    assert np.abs(u[:, 0]).max() == 0 and np.abs(u[:, clc.LADDER_ORPHAN]).max() > 0


@pytest.mark.parametrize("name", clc.SMALL)
def test_reference_equals_the_oracle_on_the_small_cases(oracle, name):
    case = clc.small_case(name)
    assert (case.Nx, case.steps) == (9, 12)
    if name == "T1":
        assert case.T == 1 and case.n_entries == case.Su[0].nnz > 0
    elif name == "T2":
        assert case.T == 2 and case.Sx[1].nnz > 0
    else:
        assert case.Nu == 0 and case.B2.shape == (9, 0) and all(m.shape == (0, 9) for m in case.Su) and len(case.Su) == case.T
    x, u = _against_oracle(oracle, case, clc.small_w(5))
    assert u.shape == (12, case.Nu, 5) and np.abs(x).max() > 0


def test_reference_without_disturbance_is_zero(ladder):
    x, u = clc.reference(ladder, None, steps=8, nscen=2)
    assert x.shape == (8, 24, 2) and u.shape == (8, 6, 2) and not x.any() and not u.any()
