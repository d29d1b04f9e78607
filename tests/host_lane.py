"""Compiles a driver for the per-lane device code (3dtk_amd/csrc/query_lane.h and ann_lane.h under tests/host_lane_shim.h) for
the host and loads it: the CPU-tier tests that execute the device walks on kd_build.cpp's host tree, or on the oracle's ANN tree."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(driver_source, tmp_path, name):
    """driver_source: C++ after `#include "host_lane_shim.h"`; returns the loaded library, host_tree_create / _destroy typed"""
    csrc = os.path.join(ROOT, "3dtk_amd", "csrc")
    cc = tmp_path / (name + ".cc")
    cc.write_text('#include "host_lane_shim.h"\n' + driver_source)
    so = str(tmp_path / ("lib" + name + ".so"))
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                        "-I" + csrc, "-I" + os.path.join(ROOT, "tests"), str(cc), os.path.join(csrc, "kd_build.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(so)
    L.host_tree_create.restype = C.c_void_p
    L.host_tree_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    L.host_tree_destroy.argtypes = [C.c_void_p]
    return L
