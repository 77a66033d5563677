"""Thermo_buoy (swthermo = "buoy") through the C++ host layer (microhh_amd/host/mhh_host.h, mhh_host_rccl.h): tests/cpp/buoy_step.cpp
checks, on the device, that thermo.exec + advec.exec + diff.exec give the bits of diff.exec_with_advec(..., &thermo) (flat and sloped
forms), that the N2 of b inside exec_viscosity gives the bits of get_thermo_field("N2") through a pointer, and that the overlapped
slab sub-step (halo_visc_rhs, one rank) matches the single-GPU sub-step. Built here with hipcc into a temporary directory."""
import pytest

import hostprog


def test_buoy_host_program_compiles():
    """not gpu: the program and the host headers it drives build against the library."""
    hostprog.compile("buoy_step", libs=("rccl",))


@pytest.mark.gpu
def test_cpp_host_thermo_buoy_substep():
    hostprog.run(hostprog.compile("buoy_step", libs=("rccl",)), timeout=300)
