"""Thermo_buoy (swthermo = "buoy") through the C++ host layer (microhh_amd/host/mhh_host.h, mhh_host_rccl.h): tests/cpp/buoy_step.cpp
checks, on the device, that thermo.exec + advec.exec + diff.exec give the bits of diff.exec_with_advec(..., &thermo) (flat and sloped
forms), that the N2 of b inside exec_viscosity gives the bits of get_thermo_field("N2") through a pointer, and that the overlapped
slab sub-step (halo_visc_rhs, one rank) matches the single-GPU sub-step. Built here with hipcc into a temporary directory."""
import os
import subprocess
import tempfile

import pytest

import common as cm

CPP = os.path.join(cm.ROOT, "tests", "cpp")
LIBDIR = os.path.join(cm.ROOT, "microhh_amd")


def _compile(out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", out, os.path.join(CPP, "buoy_step.cpp"),
                    "-L" + LIBDIR, "-lmhh_hip", "-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath," + LIBDIR], check=True)


def test_buoy_host_program_compiles():
    """not gpu: the program and the host headers it drives build against the library."""
    with tempfile.TemporaryDirectory() as tmp:
        _compile(os.path.join(tmp, "buoy_step"))


@pytest.mark.gpu
def test_cpp_host_thermo_buoy_substep():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "buoy_step")
        _compile(exe)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "buoy_step ok" in r.stdout, r.stdout + r.stderr
