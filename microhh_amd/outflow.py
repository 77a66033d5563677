"""Boundary_outflow on the host side: the driver of csrc/boundary_outflow.h behind HotPath(..., outflow=Outflow({...})).

Open lateral boundaries for scalars (src/boundary_outflow.cxx; Boundary::set_prognostic_outflow_bcs, src/boundary.cxx:464-469):
Outflow(scalars={index: profile_of_ktot_values, ...}, west="inflow", east="outflow", south="outflow", north="outflow") names the
scalars of [boundary] scalar_outflow by their index among the HotPath's scalars, each with its <name>_inflow profile, and the four
flow_direction[...] entries. Momentum and the pressure solve stay periodic, as in the reference. On a fourth-order grid the
directions and the profiles are ignored (inflow with value 0 at West, outflow at East, North and South cyclic).

A sub-step calls exec() directly after the cyclic fills (src/model.cxx:347) and, with an immersed boundary, once more after its scalar
ghost cells (:383); with `outflow` the step is the plain sequence on a slab too, since the fill has to follow the halo exchange that
the overlapped sub-step hides. On a y-slab West and East act on every rank, South on rank 0 and North on rank npy-1 only.

update() replaces an inflow profile between steps: the swtimedep_outflow of the reference, which its GPU path refuses
(src/boundary.cxx:431). The new values are copied into the SAME device buffer on the step's stream, so a graph of capture_step()
stays valid and sees them at its next replay. The interpolation in time (Timedep) is the caller's.

evisc on a slab: with slim halos the slab evaluates evisc on the ghost rows next to the slab from the fields there, where the
reference fills those rows cyclically from the interior evisc. Both agree while the fields are periodic; once the scalar that feeds
N2 (scalar 0 under dry, moist and buoy thermodynamics) is open at South or North they differ, so with scalar 0 among the open
scalars HotPath switches evisc_local_ghosts off and evisc is exchanged like any field.
"""
import ctypes as C

import numpy as np

from . import capi

WEST, EAST, SOUTH, NORTH = 1, 2, 4, 8            # MHH_OUTFLOW_* of include/mhh_hip.h
DIRECTIONS = {"outflow": 0, "inflow": 1}


def profile_table(lib, grid, profile):
    """The kcells table of ktot inflow values, ghost levels zero (src/boundary.cxx:421-424)."""
    prof = np.ascontiguousarray(profile, dtype=grid.np_dtype)
    if prof.shape != (grid.ktot,):
        raise ValueError("outflow: an inflow profile holds ktot = %d values" % grid.ktot)
    tab = np.empty(grid.kcells, dtype=grid.np_dtype)
    capi.check(lib.mhh_boundary_outflow_profile_host(grid.host_struct(), prof.ctypes.data, tab.ctypes.data), lib)
    return tab


def edges_of(npy, rank):
    """The edges rank `rank` of npy slab ranks owns: mpicoordx == 0 == npx-1 always, South on rank 0, North on rank npy-1."""
    return WEST | EAST | (SOUTH if rank == 0 else 0) | (NORTH if rank == npy - 1 else 0)


def exec_fields(lib, G, order, fields, profiles, dirs, mask, stream=None):
    """mhh_boundary_outflow_exec on raw addresses: fields and profiles are sequences of device pointers."""
    n = len(fields)
    fa = (C.c_void_p * max(1, n))(*fields)
    pa = (C.c_void_p * max(1, n))(*profiles)
    da = (C.c_int * 4)(*dirs)
    capi.check(lib.mhh_boundary_outflow_exec(G, order, fa, n, pa, da, mask, stream), lib)


class Outflow:
    def __init__(self, scalars, west="inflow", east="outflow", south="outflow", north="outflow"):
        self.scalars = {int(k): v for k, v in dict(scalars).items()}
        self.directions = dict(west=west, east=east, south=south, north=north)

    def bind(self, hp):
        self.hp = hp
        for name, d in self.directions.items():
            if d not in DIRECTIONS:
                raise ValueError("outflow: Inflow direction \"%s\" is invalid (%s)" % (d, name))
        for n in self.scalars:
            if not 0 <= n < len(hp.s):
                raise ValueError("outflow: scalar %d of %d" % (n, len(hp.s)))
        self.dirs = [DIRECTIONS[self.directions[e]] for e in ("west", "east", "south", "north")]
        self.order = int(hp.cfg["order"])
        self.mask = edges_of(hp.npy, hp.rank)
        self.index = sorted(self.scalars)
        torch = hp.torch
        self.tables = {n: torch.from_numpy(profile_table(hp.lib, hp.grid, self.scalars[n])).to(hp.device) for n in self.index}
        self._fields = (C.c_void_p * max(1, len(self.index)))(*[hp.s[n].data_ptr() for n in self.index])
        self._profiles = (C.c_void_p * max(1, len(self.index)))(*[self.tables[n].data_ptr() for n in self.index])
        self._dirs = (C.c_int * 4)(*self.dirs)
        return self

    def exec(self):
        """boundary->set_prognostic_outflow_bcs (src/model.cxx:347, :383): at most two launches for all open scalars."""
        hp = self.hp
        capi.check(hp.lib.mhh_boundary_outflow_exec(hp.G, self.order, self._fields, len(self.index), self._profiles, self._dirs, self.mask, hp.stream), hp.lib)

    def update(self, index, profile):
        """A new inflow profile (ktot values) for scalar `index`, copied into the table's device buffer on the current stream."""
        hp = self.hp
        if int(index) not in self.tables:
            raise ValueError("outflow: scalar %d is not open" % int(index))
        tab = hp.torch.from_numpy(profile_table(hp.lib, hp.grid, profile))
        self.scalars[int(index)] = np.array(profile, dtype=hp.grid.np_dtype)
        self.tables[int(index)].copy_(tab)
