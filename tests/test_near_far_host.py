"""Host check of the near / far threshold arithmetic (include/gunrock/hip/kernels/near_far.hxx):
tests/cpp/near_far_tests.cpp built as a stand-alone program with the address and undefined-behaviour
sanitizers on the host code, and run.  No GPU, no HIP."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_near_far_host_checks_under_sanitizers(tmp_path):
    # clang links the sanitizer runtime statically; g++ is told to
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    clang = rocm_clang if os.path.exists(rocm_clang) else shutil.which("clang++")
    gxx = shutil.which("g++")
    assert clang or gxx, "no C++ compiler"
    cmd = [clang] if clang else [gxx, "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "near_far_tests")
    subprocess.run(cmd + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "tests", "cpp", "near_far_tests.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
