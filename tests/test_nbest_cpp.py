"""CPU: the C++ host mirror's n-best table (include/whisper_mi.hpp Whisper::nbest_table, driven by tests/cpp/nbest_check.cpp) equals
the Python builder's arrays (_lib.nbest_args) on a fixed candidate list, and makes its refusals.  Host code only: nothing
of the library is linked or called."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANDS = [[[1, 2, 3]], [[4, 5], [6, 7, 8, 9, 10, 11, 12], [1, 1], [9, 9, 9]], [[2, 3, 4, 5, 6], [9, 8]]]  # the list nbest_check.cpp builds


def test_cpp_table_equals_the_python_builder():
    from whisper_mojo_amd import _lib
    exe = os.path.join(ROOT, "tests", "cpp", "nbest_check")
    subprocess.check_call([shutil.which("g++") or shutil.which("c++"), "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "nbest_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = {ln.split()[0]: np.asarray(ln.split()[1:], np.int32) for ln in out.stdout.strip().split("\n")}
    tab, lens, _ctx, n_cand, utt_of, row0 = _lib.nbest_args(CANDS, None, 3, 100, 32, 8)
    want = dict(shape=np.asarray(tab.shape), tab=tab.ravel(), len=lens, n_cand=n_cand, row0=row0, utt_of=utt_of)
    assert sorted(got) == sorted(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert subprocess.run([exe, "bad"], capture_output=True, timeout=60).returncode == 0
