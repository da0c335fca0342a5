"""The plan of the weight-only MXFP4 linear (csrc/mxfp4w_plan.h) on the CPU: tests/host/mxfp4w_plan_check.cpp replays
the kernels' index arithmetic and checks the route rule and the workspace sizes; it is built here with the host compiler
(under AddressSanitizer + UBSan where it has them) and run directly: no Python code runs under a sanitizer."""
import os
import subprocess

from conftest import PKG, ROOT
from fp8_cases import host_compiler


def run_host_check(tmp_dir, name):
    """build tests/host/<name>.cpp and run it; returns the number of checks it made"""
    exe = str(tmp_dir / name)
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:  # a compiler without the sanitizer runtimes: the plain build
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return int(r.stdout.split()[-1])


def test_lane_maps_clamps_routes_and_workspace_sizes(tmp_path):
    assert run_host_check(tmp_path, "mxfp4w_plan_check") > 1000
