"""The per-position forms of the plan kernel and the first scatter pass (pangaea_amd/csrc/mini_forms.hpp), on the host.

The header compiles as plain C++; tests/minimizer_forms_main.cpp is built from it here with the host compiler and compares,
position by position, what the kernels compute -- the minimizer value from left-aligned canonical M-mers and the tree of
minima, the mask of positions whose value equals their predecessor's, the region bytes of the plan's packed column -- with the
definition written out naively: the smallest mhash(min(M-mer, its reverse complement)) over the k-mer's central window, as
``mini_minimizer_of`` has it.  Every k from 13 to 31 (M = 11 and 13, windows of 3 to 9, delays 0 to 5), a few thousand random
word pairs each, and the edge words: all-A, all-T, alternating AT, words whose oldest and newest M-mers are reverse complements.
Built with the address and undefined-behaviour sanitizers where the compiler has them (host code with its own main)."""
import os
import shutil
import subprocess

import pytest

from .conftest import ROOT

SRC = os.path.join(ROOT, "tests", "minimizer_forms_main.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "pangaea_amd", "csrc"), "-I", os.path.join(ROOT, "include")]


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++, g++, clang++ or $CXX)")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("minimizer_forms") / "minimizer_forms")
    base = [_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *INCLUDES, SRC, "-o", out]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout or r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower():
        r = subprocess.run(base, capture_output=True, text=True)           # a compiler without the sanitizer runtimes
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_forms_agree_with_the_definition_at_every_position(program):
    r = subprocess.run([program, "3000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-3000:] + r.stderr[-3000:]
    # 19 k x (49 + 112 + 16 + 3000 + 750 word pairs) x 32 positions
    assert int(r.stdout.split()[1]) == 19 * (49 + 112 + 16 + 3000 + 750) * 32


def test_the_program_notices_a_wrong_hash_constant(program, tmp_path):
    """the comparison is not vacuous: the same program built against a header whose mhash multiplier is off by two fails"""
    hdr = open(os.path.join(ROOT, "pangaea_amd", "csrc", "mini_forms.hpp")).read()
    assert hdr.count("0xC2B2AFu") == 1
    (tmp_path / "mini_forms.hpp").write_text(hdr.replace("0xC2B2AFu", "0xC2B2B1u"))
    out = str(tmp_path / "wrong")
    r = subprocess.run([_compiler(), "-std=c++17", "-O1", "-I", str(tmp_path), *INCLUDES, SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([out, "50"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "the definition gives" in r.stdout
