"""tests/devcheck/sort.hip -> libmot_sort.so (hipcc, gfx950, the product's flags) or libmot_sort_emu.so (the host: g++, or the clang++ beside hipcc, against
tests/emu/hipemu.h). TEST INFRASTRUCTURE: the device-wide radix sort of csrc/mot_sort.h, driven directly (tests/sort_cases.py); not part of libmot_hip.so."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "csrc")
SRC = os.path.join(HERE, "sort.hip")
LIB = os.path.join(HERE, "libmot_sort.so")
LIB_EMU = os.path.join(HERE, "libmot_sort_emu.so")
HEADERS = ("mot_wave.h", "mot_wave_sync.h", "mot_sort.h")


def _stale(lib):
    deps = [SRC, os.path.abspath(__file__), os.path.join(ROOT, "include", "mot.h")] + [os.path.join(CSRC, h) for h in HEADERS]
    return not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps)


def _hipcc():
    return next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)


def _run(cmd, out):
    r = subprocess.run(cmd + ["-o", out + ".tmp"], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr)
    os.replace(out + ".tmp", out)
    return out


def build(force=False, extra_flags=(), out=None):
    """extra_flags / out: a deliberately different build beside the default one (a mutant for checking the tests themselves), never the default library"""
    if out is None and not force and not _stale(LIB):
        return LIB
    hipcc = _hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math",
           "-fno-gpu-flush-denormals-to-zero"] + list(extra_flags) + ["-I", CSRC, SRC]   # the product's flags: the same device functions, compiled the same way
    return _run(cmd, out or LIB)


def host_compiler():
    """g++ if present, else the clang++ that ships beside hipcc"""
    gxx = shutil.which("g++")
    if gxx:
        return gxx
    hipcc = _hipcc()
    for c in ([os.path.join(os.path.dirname(os.path.realpath(hipcc)), "clang++"), os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "clang++")] if hipcc else []) + \
            ["/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]:
        if os.path.exists(c):
            return c
    raise RuntimeError("no host C++ compiler (g++, or clang++ beside hipcc)")


def build_emu(force=False, extra_flags=(), out=None):
    if out is None and not force and not _stale(LIB_EMU):
        return LIB_EMU
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-DMOT_HIPEMU=1"] + list(extra_flags) + ["-x", "c++", "-include",
           os.path.join(ROOT, "tests", "emu", "hipemu.h"), "-I", CSRC, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable", SRC]
    return _run(cmd, out or LIB_EMU)


if __name__ == "__main__":
    print(build(force=True))
    print(build_emu(force=True))
