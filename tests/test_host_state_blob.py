"""The checkpoint blob's header checks (stark_amd/csrc/state_blob.h) on the host, under the address
and undefined-behaviour sanitizers: tools/state_blob_check.cpp is compiled as a stand-alone program
and run as its own process.  Nothing is preloaded and nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _sanitizing_compiler(tmp):
    """The first C++ compiler here that links and runs a program with both sanitizer runtimes."""
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for cxx in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        exe = shutil.which(cxx)
        if not exe:
            continue
        out = tmp / "probe"
        if subprocess.run([exe, *SAN, "-o", str(out), str(probe)], capture_output=True).returncode == 0 and \
                subprocess.run([str(out)], capture_output=True).returncode == 0:
            return exe
    return None


def test_state_blob_check_under_sanitizers(tmp_path):
    cxx = _sanitizing_compiler(tmp_path)
    if cxx is None:
        pytest.skip("no C++ compiler with the address and undefined-behaviour sanitizer runtimes")
    exe = tmp_path / "state_blob_check"
    cc = subprocess.run([cxx, *SAN, "-g", "-o", str(exe), os.path.join(ROOT, "tools", "state_blob_check.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 miss(es)" in run.stdout and "MISS" not in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
