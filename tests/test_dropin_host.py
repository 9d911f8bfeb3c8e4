"""Host arithmetic of the one-shot calls (no GPU): csrc/sls_dropin_host.cpp — the layering of overlapping groups, the shard
cuts, the refinement selection, the block-diagonal composite of a batch, the unpack of packed shards and the status fold that
sls_h2_sf_solve / _batch / _localized (csrc/sls_dropin.cpp) are written on.  The known answers live in the stand-alone program
tests/host_sanitize/sanitize_dropin.cpp, each derived by hand beside its check; the GPU tests of tests/test_gpu_parity.py pin
the same code end to end."""
import os
import shutil
import subprocess

import numpy as np
import pytest


def test_dropin_host_under_sanitizers(tmp_path):
    """csrc/sls_dropin_host.cpp + csrc/sls_symbolic.cpp (plain C++, no HIP) compiled by g++ with AddressSanitizer and
    UndefinedBehaviorSanitizer and driven by tests/host_sanitize/sanitize_dropin.cpp, in both index bases."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "systemlevelcontrol.jl_amd", "csrc")
    src = [os.path.join(here, "host_sanitize", "sanitize_dropin.cpp"), os.path.join(csrc, "sls_dropin_host.cpp"),
           os.path.join(csrc, "sls_symbolic.cpp")]
    exe = str(tmp_path / "sanitize_dropin")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__host__=", "-D__device__=", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", *src, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitize_dropin: clean" in r.stdout and "runtime error" not in r.stderr


@pytest.mark.parametrize("nshards", [1, 3, 8, 200])
def test_cuts_through_the_export_partition_the_groups(slc, readme, nshards):
    """balanced_cuts behind sls_shard_groups (no device needed): the cuts of the README chain's default groups start at 0, end
    at Nx and never descend — also with more shards than groups."""
    P, S, _ = readme
    cuts = np.asarray(slc.dist.shard_groups(P, S, None, nshards))
    assert len(cuts) == nshards + 1 and cuts[0] == 0 and cuts[-1] == P.Nx
    assert np.all(np.diff(cuts) >= 0)
