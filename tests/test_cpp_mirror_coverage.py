"""CPU: the C++ host mirror (include/whisper_mi.hpp) still compiles under -Wall -Wextra -Werror with the program that calls all of
it (tests/cpp/host_mirror_check.cpp), and every method of class Whisper has a C++ caller under tests/cpp/ or in examples/main.cpp
— so an entry added later cannot land with nothing in C++ running it.  What the callers compute is checked on the GPU
by tests/test_gpu_cpp_mirror.py."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper.mojo_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "whisper_mi.hpp")
# private helpers: reached through the public entries
EXEMPT = {"need_model", "opts", "unpack", "prompt_table", "lang_collect"}
# a member function's first line: four spaces, optional specifiers, a return type, the name, "("
METHOD = re.compile(r"^ {4}(?:template <[^>]*> )?(?:static )?(?:[\w:]+(?:<[^()]*>)?[&*]* )+(\w+)\(", re.M)


def whisper_methods():
    text = open(HEADER, encoding="utf-8").read()
    body = text[text.index("class Whisper {"):text.index("// tokenizer.mojo:4-28")]
    return sorted({n for n in METHOD.findall(body) if n != "Whisper"})


def test_the_parse_finds_the_entries_it_should():
    names = whisper_methods()
    for n in ("load", "transcribe", "transcribe_batch", "transcribe_wait", "set_alignment_heads", "transcribe_batch_tt", "transcribe_batch_lp_ns", "score",
              "nbest_table", "score_candidates", "align", "detect_language", "transcribe_submit_lang", "transcribe_long", "resample",
              "transcribe_chunked_ts", "set_timestamps", "top_k", "constraint_trie", "constraint_match", "config", "handle", "lang_collect", "opts"):
        assert n in names, n
    # 32 public entries and the five helpers today
    assert len(names) >= 37 and not {"if", "for", "check", "return", "ScoreResult", "Pend"} & set(names), names


def test_every_method_has_a_cpp_caller():
    sources = glob.glob(os.path.join(ROOT, "tests", "cpp", "*.cpp")) + [os.path.join(ROOT, "examples", "main.cpp")]
    code = "\n".join(open(p, encoding="utf-8").read() for p in sources)
    missing = [n for n in whisper_methods() if n not in EXEMPT and not re.search(r"(?:\.|->|Whisper::)" + n + r"\s*\(", code)]
    assert not missing, f"no C++ caller under tests/cpp/ or examples/ for Whisper::{missing}"


def test_the_mirror_compiles_without_warnings():
    if not os.path.exists(os.path.join(CSRC, "libwhispermi.so")):
        pytest.skip("libwhispermi.so not built")
    exe = os.path.join(ROOT, "tests", "cpp", "host_mirror_check_werror")
    r = subprocess.run([shutil.which("g++") or shutil.which("c++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "host_mirror_check.cpp"), "-o", exe, "-L", CSRC, "-lwhispermi", "-Wl,-rpath," + CSRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)  # no mode: ends before anything touches the GPU
    assert r.returncode == 2
