"""CPU: the C++ host mirror's trie flattening (include/whisper_mi.hpp Whisper::constraint_trie, driven by
tests/cpp/constraint_check.cpp) equals the Python builder's arrays (_lib.constraint_trie) on a fixed list, and refuses a duplicate
phrase.  Host code only: nothing of the library is linked or called."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _phrases():
    """the list tests/cpp/constraint_check.cpp builds"""
    ph = [(7, 3, 9), (7, 3), (7, 4), (2,), (2, 2, 2, 2), (11, 5, 5, 1, 0, 8), (7, 3, 9, 9), (0,), (11, 5), (3, 7)]
    return ph + [(1000 + 3 * ((i * 37) % 640), i % 5) for i in range(640)]


def test_cpp_trie_equals_the_python_builder():
    from whisper_mojo_amd import _lib
    exe = os.path.join(ROOT, "tests", "cpp", "constraint_check")
    subprocess.check_call([shutil.which("g++") or shutil.which("c++"), "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "constraint_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = {ln.split()[0]: np.asarray(ln.split()[1:], np.int32) for ln in out.stdout.strip().split("\n")}
    want = dict(zip(("edge_off", "edge_id", "edge_next", "terminal"), _lib.constraint_trie(_phrases())))
    assert sorted(got) == sorted(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert want["edge_off"][1] - want["edge_off"][0] > 600  # the root's fan-out
    assert subprocess.run([exe, "dup"], capture_output=True, timeout=60).returncode == 0
