"""The compile line of the C++ shim drivers tests/cxx/*_shim_test.cpp: plain g++ over include/ and include/shim/ against
libcoslam_hip.so, the way a C++ caller of the library builds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_shim_test(name, out_dir, hip_runtime=True):
    """Compiles tests/cxx/<name> into out_dir and returns the executable's path.  hip_runtime: the driver calls the HIP runtime itself
    (platform define, ROCm's headers, -lamdhip64); False for a driver that only goes through the library."""
    src, exe = os.path.join(ROOT, "tests", "cxx", name), os.path.join(str(out_dir), os.path.splitext(name)[0])
    libdir = os.path.join(ROOT, "coslam_amd", "lib")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "shim")]
    link = ["-L", libdir, "-lcoslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    if hip_runtime:
        cmd = ["g++", "-std=c++11", "-O1", "-D__HIP_PLATFORM_AMD__", *inc, "-I/opt/rocm/include", src, *link, "-lamdhip64", "-o", exe]
    else:
        cmd = ["g++", "-std=c++11", "-O1", *inc, src, *link, "-o", exe]
    subprocess.check_call(cmd)
    return exe
