"""The stand-alone program of the host rule preparation (tests/rules_host_main.cpp over
csrc/pii_rules_host.h), built once per test run with the host compiler under the address and
undefined-behaviour sanitizers, and a runner for it: shared by test_rules_host, test_exclusion_host and
test_text_excl_host.  The program exits 0 whether it accepts or rejects a blob; a sanitizer report is
the only failure."""
import os
import shutil
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "rules_host_main.cpp")
_exe = None


def program(tmp_path_factory) -> str:
    global _exe
    if _exe is None:
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        assert cxx, "no host C++ compiler found (g++, c++ or clang++)"
        exe = str(tmp_path_factory.mktemp("rules_host") / "rules_host_main")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
        _exe = exe
    return _exe


def runner(tmp_path_factory, tag: str):
    """go(name, blob) -> the program's output line for that blob"""
    exe = program(tmp_path_factory)
    d = tmp_path_factory.mktemp(tag)

    def go(name: str, blob: bytes) -> str:
        path = d / (name + ".bin")
        path.write_bytes(blob)
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        return r.stdout.strip()
    return go
