"""The radix sort's host-side arithmetic (rdfind_amd/csrc/radix_host.hpp: pass count, digit widths, histogram layout, the
host histogram of keys in segments) as a stand-alone program under the host sanitizers: tools/radix_host_check.cpp is
compiled with -fsanitize=address,undefined and run on its own (no GPU, nothing preloaded)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_radix_host_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ or c++): the project's own build needs one"
    exe = tmp_path / "radix_host_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "radix_host_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "radix_host_check ok" in r.stdout
