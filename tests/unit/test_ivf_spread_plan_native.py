"""The chunk schedule of the in-place IVF spread (csrc/include/ivf_spread_plan.h)
is host code: tests/native/ivf_spread_plan_test.cpp replays it with a host
loop in place of the kernel launch over a few hundred random shapes, against
std::stable_sort, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer. This test builds and runs that program."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_spread_plan_under_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "ivf_spread_plan_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "csrc", "include"),
                    os.path.join(ROOT, "tests", "native", "ivf_spread_plan_test.cpp"), "-o", exe], check=True)
    # (the leak check needs ptrace, which a sandboxed runner may not have; bounds and UB are the point here)
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "400 shapes, 0 failures" in out.stdout
